// image_stats_ref.cc — CPU restatement of the reference's image statistics and intensity scaling on single-channel float
// images with an optional validity mask (the PixelMask), serial and in raster order, written from the reference's text.
// Test infrastructure only; built with the oracle's flags (no contraction, no fast-math).  Every function names the lines
// it restates.  Images are packed rows of `w` floats; mask: uint8, non-zero = valid, NULL = every pixel valid.
// sc, sr: 0, 0 = every pixel, else the sampling grid of otsu_threshold's second overload (ImageThresh.h:156-166).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

namespace {

struct Visit {      // the pixels a pass visits, in its order
  const float* img; const uint8_t* mask; int w, h, sc, sr;
  template <class F> void each(F f) const {
    if (!sc) {
      for (int row = 0; row < h; row++)
        for (int col = 0; col < w; col++)
          if (!mask || mask[(size_t)row * w + col]) f(img[(size_t)row * w + col]);
      return;
    }
    const double row_ratio = double(h - 1.0) / double(sr - 1.0);      // ImageThresh.h:156-157
    const double col_ratio = double(w - 1.0) / double(sc - 1.0);
    for (int sample_row = 0; sample_row < sr; sample_row++) {
      const int row = round(sample_row * row_ratio);                  // :163
      for (int sample_col = 0; sample_col < sc; sample_col++) {
        const int col = round(sample_col * col_ratio);                // :166
        if (!mask || mask[(size_t)row * w + col]) f(img[(size_t)row * w + col]);
      }
    }
  }
};

// math::Histogram (src/vw/Math/Statistics.cc:34-76) with saturate = true.  A bin argument that is NaN is counted apart and an
// argument beyond int saturates by its sign: the reference's conversion to int is undefined for both.
struct Histogram {
  int num_bins, max_bin;
  double min_value, range, bin_width;
  uint64_t* bins; uint64_t total = 0, nans = 0;
  Histogram(int n, double mn, double mx, uint64_t* b) : num_bins(n), max_bin(n - 1), min_value(mn), bins(b) {
    range = mx - mn;                      // :48
    bin_width = range / num_bins;         // :49
  }
  void add_value(double value) {
    const double a = max_bin * ((value - min_value) / range);       // :59
    if (a != a) { nans++; return; }
    const double r = round(a);
    int bin = r < 0 ? 0 : r >= num_bins ? max_bin : static_cast<int>(r);      // :61-72
    bins[bin] += 1;
    ++total;
  }
};

// Histogram::get_percentile, Statistics.cc:85-104; -1: illegal percentile, -2: "Illegal histogram encountered"
int get_percentile(const uint64_t* bins, int num_bins, uint64_t num_values, double percentile) {
  if ((percentile < 0) || (percentile > 1.0) || percentile != percentile) return -1;
  double sum = static_cast<double>(num_values);
  double running_percentile = 0;
  for (int i = 0; i < num_bins; ++i) {
    double this_percent = (double)bins[i] / sum;
    running_percentile += this_percent;
    if (running_percentile >= percentile) return i;
  }
  return -2;
}

// ChannelClampFunctor, ChannelNormalizeFunctor, ChannelThresholdFunctor of src/vw/Image/Algorithms.h with channel_type float
struct Clamp {
  float m_low, m_high;
  float operator()(float value) const {      // :43-47
    if (value > m_high) return m_high;
    else if (value < m_low) return m_low;
    else return value;
  }
};
struct Normalize {
  float m_old_min, m_new_min;
  double m_old_to_new_ratio;
  Normalize(float old_min, float old_max, float new_min, float new_max) : m_old_min(old_min), m_new_min(new_min) {      // :111-119
    if (old_max == old_min) m_old_to_new_ratio = 0.0;
    else m_old_to_new_ratio = (new_max - new_min) / (double)(old_max - old_min);
  }
  float operator()(float value) const { return (float)((value - m_old_min) * m_old_to_new_ratio + m_new_min); }      // :122-125
};
struct Threshold {
  float m_thresh, m_low, m_high;
  float operator()(float val) const { return (val > m_thresh) ? m_high : m_low; }      // :205-207
};

// pixel_cast<uint8>: the C conversion where it is defined; NaN and negatives 0, 256 and above 255 where it is not
uint8_t to_u8(float v) { return v >= 256.f ? 255 : v >= 0.f ? (uint8_t)v : 0; }

void store(int out_type, void* out, size_t i, float v) {
  if (out_type == 0) static_cast<float*>(out)[i] = v;
  else if (out_type == 1) static_cast<uint8_t*>(out)[i] = to_u8(v);
  else static_cast<float*>(out)[i] = (float)to_u8(v);
}

void find_min_max(const Visit& V, double& min_val, double& max_val, long long* counts) {      // Statistics.h:113-127, ImageThresh.h:160-174
  max_val = -std::numeric_limits<double>::max();
  min_val = -max_val;
  long long n = 0, nan = 0;
  V.each([&](float px) {
    double val = px;
    n++;
    if (val != val) nan++;
    if (val < min_val) min_val = val;
    if (val > max_val) max_val = val;
  });
  if (counts) { counts[0] = n; counts[1] = nan; }
}

}  // namespace

extern "C" {

int isr_find_min_max(const float* img, int w, int h, const uint8_t* mask, int sc, int sr, double* out, long long* counts) {
  find_min_max(Visit{img, mask, w, h, sc, sr}, out[0], out[1], counts);
  return 0;
}

// min_max_channel_values (Statistics.h:98-108) over MinMaxAccumulator<float> (Math/Functors.h:355-372); -1: no valid samples
int isr_min_max_channel_values(const float* img, int w, int h, const uint8_t* mask, int sc, int sr, double* out) {
  float m_minval = 0, m_maxval = 0;
  bool m_valid = false;
  Visit{img, mask, w, h, sc, sr}.each([&](float arg) {
    if (!m_valid) {
      m_minval = m_maxval = arg;
      m_valid = true;
    } else {
      if (arg < m_minval) m_minval = arg;
      if (m_maxval < arg) m_maxval = arg;
    }
  });
  if (!m_valid) return -1;
  out[0] = m_minval; out[1] = m_maxval;
  return 0;
}

// {count, sum, sum of squares}: MeanAccumulator / StdDevAccumulator (Functors.h:478-481, :502-506), raster order
int isr_moments(const float* img, int w, int h, const uint8_t* mask, int sc, int sr, double* out) {
  double mom1_accum = 0, mom2_accum = 0, num_samples = 0;
  Visit{img, mask, w, h, sc, sr}.each([&](float arg) {
    mom1_accum += arg;
    mom2_accum += (double)arg * arg;
    num_samples += 1.0;
  });
  out[0] = num_samples; out[1] = mom1_accum; out[2] = mom2_accum;
  return 0;
}
int isr_mean(const double* m, double* out) {      // Functors.h:483-486
  if (!m[0]) return -1;
  *out = m[1] / m[0];
  return 0;
}
int isr_stddev(const double* m, double* out) {    // Functors.h:509-512
  if (!m[0]) return -1;
  *out = sqrt(m[2] / m[0] - (m[1] / m[0]) * (m[1] / m[0]));
  return 0;
}

// vw::histogram, ImageThresh.h:53-73; counts: num_bins bins, the total, the NaN count
int isr_histogram(const float* img, int w, int h, const uint8_t* mask, int sc, int sr, int num_bins, double min_val, double max_val,
                  int accumulate, uint64_t* counts, double* bin_width) {
  if (num_bins <= 0) return -1;
  if (max_val == min_val) max_val = min_val + 1.0;      // :61-62
  if (!accumulate) memset(counts, 0, ((size_t)num_bins + 2) * 8);
  Histogram hist(num_bins, min_val, max_val, counts);
  Visit{img, mask, w, h, sc, sr}.each([&](float px) {
    double val = px;
    hist.add_value(val);
  });
  counts[num_bins] += hist.total;
  counts[num_bins + 1] += hist.nans;
  if (bin_width) *bin_width = hist.bin_width;
  return 0;
}

int isr_get_percentile(const uint64_t* counts, int num_bins, uint64_t total, double percentile) {
  return get_percentile(counts, num_bins, total, percentile);
}

// What the two overloads of otsu_threshold do with their histogram; min_val, max_val after `if (max_val == min_val) max_val++`.
double isr_otsu_counts(const uint64_t* counts, int num_bins, uint64_t total, double min_val, double max_val, int overload) {
  if (overload == 1) {      // ImageThresh.h:97-144
    double sum = static_cast<double>(total);
    if (sum == 0.0) return 0.0;
    double totalAccum = 0.0;
    for (int i = 0; i < num_bins; i++) totalAccum += i * ((double)counts[i] / sum);
    std::vector<double> V;
    V.assign(num_bins, 0.0);
    double leftProb = 0.0, leftAccum = 0.0, rightProb = 0.0, rightAccum = 0.0;
    for (int i = 0; i < num_bins; i++) {
      leftProb += (double)counts[i] / sum;
      leftAccum += i * ((double)counts[i] / sum);
      rightProb = 1.0 - leftProb;
      rightAccum = totalAccum - leftAccum;
      if (leftProb == 0 || rightProb == 0.0) continue;
      double leftMean = leftAccum / leftProb;
      double rightMean = rightAccum / rightProb;
      V[i] = leftProb * rightProb * (leftMean - rightMean) * (leftMean - rightMean);
    }
    double maxV = *std::max_element(V.begin(), V.end());
    double indexSum = 0, numIndices = 0;
    for (size_t i = 0; i < V.size(); i++) {
      if (V[i] == maxV) {
        indexSum += i;
        numIndices++;
      }
    }
    double meanIndex = indexSum / numIndices;
    double normalized_index = meanIndex / (num_bins - 1.0);
    return min_val + normalized_index * (max_val - min_val);
  }
  // ImageThresh.h:204-238
  std::int64_t num_valid = (std::int64_t)total;
  if (num_valid == 0) return 0.0;
  double mu = 0, scale = 1.0 / double(num_valid);
  for (int i = 0; i < num_bins; i++) mu += i * (double)counts[i];
  mu *= scale;
  double mu1 = 0, q1 = 0;
  double max_sigma = 0, max_pos = 0;
  for (int i = 0; i < num_bins; i++) {
    double p_i, q2, mu2, sigma;
    p_i = (double)counts[i] * scale;
    mu1 *= q1;
    q1 += p_i;
    q2 = 1.0 - q1;
    if (std::min(q1, q2) < FLT_EPSILON || std::max(q1, q2) > 1.0 - FLT_EPSILON) continue;
    mu1 = (mu1 + i * p_i) / q1;
    mu2 = (mu - q1 * mu1) / q2;
    sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2);
    if (sigma > max_sigma) {
      max_sigma = sigma;
      max_pos = i;
    }
  }
  return (max_val - min_val) * (max_pos / (num_bins - 1.0)) + min_val;
}

// otsu_threshold(view) (overload 1: 256 bins, every pixel) and otsu_threshold(view, num_sample_rows, num_sample_cols, num_bins)
// (overload 2; sc = sr = 0 stands for cols and rows).  ImageThresh.h:80-145, :151-239.
double isr_otsu_threshold(const float* img, int w, int h, const uint8_t* mask, int sc, int sr, int num_bins, int overload) {
  if (overload == 1) { num_bins = 256; sc = sr = 0; }
  else if (!sc) { sc = w; sr = h; }
  const Visit V{img, mask, w, h, sc, sr};
  double min_val, max_val;
  find_min_max(V, min_val, max_val, nullptr);
  if (max_val == min_val) max_val++;
  std::vector<uint64_t> counts((size_t)num_bins + 2, 0);
  Histogram hist(num_bins, min_val, max_val, counts.data());
  V.each([&](float px) { hist.add_value(px); });
  return isr_otsu_counts(counts.data(), num_bins, hist.total, min_val, max_val, overload);
}

// median_channel_value over destructive_median (Functors.h:393-398) and destructive_percentile (:424-444) on the valid pixels
// as std::vector<float>.  kind 0: sorted[k]; 1: the median; 2: the percentile.  -1: no valid samples (or an illegal percentile).
int isr_order_statistic(const float* img, int w, int h, const uint8_t* mask, int kind, double arg, double* out) {
  std::vector<float> vec;
  Visit{img, mask, w, h, 0, 0}.each([&](float px) { vec.push_back(px); });
  int len = vec.size();
  if (!len) return -1;
  std::sort(vec.begin(), vec.end());
  if (kind == 1) {
    *out = len % 2 ? vec[len / 2] : (vec[len / 2 - 1] + vec[len / 2]) / 2.0;
  } else if (kind == 2) {
    if (!(arg >= 0 && arg <= 100.0)) return -1;
    int index = ceil((arg / 100.0) * double(len));
    index--;
    if (index < 0) index = 0;
    if (index >= len) index = len - 1;
    *out = vec[index];
  } else {
    *out = vec[arg >= (double)len ? len - 1 : (int)arg];
  }
  return 0;
}

// clamp (Algorithms.h:50-61), normalize (:171-188), normalize(clamp()), threshold (:210-); params as vwgpu_image_rescale takes them.
// out_type 0: float, 1: pixel_cast<uint8>, 2: that uint8 as a float.
int isr_rescale(const float* img, int w, int h, int mode, const double* p, int out_type, void* out) {
  const size_t n = (size_t)w * h;
  if (mode == 0) {
    const Clamp c{(float)p[0], (float)p[1]};
    for (size_t i = 0; i < n; ++i) store(out_type, out, i, c(img[i]));
  } else if (mode == 1) {
    const Normalize f((float)p[0], (float)p[1], (float)p[2], (float)p[3]);
    for (size_t i = 0; i < n; ++i) store(out_type, out, i, f(img[i]));
  } else if (mode == 2) {
    const Clamp c{(float)p[0], (float)p[1]};
    const Normalize f((float)p[2], (float)p[3], (float)p[4], (float)p[5]);
    for (size_t i = 0; i < n; ++i) store(out_type, out, i, f(c(img[i])));
  } else if (mode == 3) {
    const Threshold t{(float)p[0], (float)p[1], (float)p[2]};
    for (size_t i = 0; i < n; ++i) store(out_type, out, i, t(img[i]));
  } else {
    return -1;
  }
  return 0;
}

// percentile_scale_convert, ImageThresh.h:243-270; params {min, max, low_value, high_value}, bins {low_bin, high_bin}.
// -2: get_percentile throws (no valid pixel).
int isr_percentile_scale_convert(const float* img, int w, int h, const uint8_t* mask, double low_percentile, double high_percentile,
                                 int num_bins, int out_type, void* out, double* params, int* bins) {
  const Visit V{img, mask, w, h, 0, 0};
  double min_val = -1.0, max_val = -1.0;
  find_min_max(V, min_val, max_val, nullptr);
  std::vector<uint64_t> counts((size_t)num_bins + 2, 0);
  double hist_max = max_val;
  if (hist_max == min_val) hist_max = min_val + 1.0;      // :61-62
  Histogram hist(num_bins, min_val, hist_max, counts.data());
  V.each([&](float px) { hist.add_value(px); });
  const int low_bin = get_percentile(counts.data(), num_bins, hist.total, low_percentile);
  const int high_bin = get_percentile(counts.data(), num_bins, hist.total, high_percentile);
  if (low_bin < 0 || high_bin < 0) return low_bin < 0 ? low_bin : high_bin;
  double bin_width = hist.bin_width;
  double low_value = ((size_t)low_bin + 1) * bin_width + min_val;
  double high_value = ((size_t)high_bin + 1) * bin_width + min_val;
  const Clamp c{(float)low_value, (float)high_value};
  const Normalize f((float)low_value, (float)high_value, (float)0.0, (float)255.0);
  for (size_t i = 0; i < (size_t)w * h; ++i) store(out_type, out, i, f(c(img[i])));
  if (params) { params[0] = min_val; params[1] = max_val; params[2] = low_value; params[3] = high_value; }
  if (bins) { bins[0] = low_bin; bins[1] = high_bin; }
  return 0;
}

// u8_convert, ImageThresh.h:274-286; -2: no valid (non-NaN) pixel, where the bounds would be +-DBL_MAX
int isr_u8_convert(const float* img, int w, int h, const uint8_t* mask, int out_type, void* out, double* params) {
  double min_val, max_val;
  long long counts[2];
  find_min_max(Visit{img, mask, w, h, 0, 0}, min_val, max_val, counts);
  if (counts[0] == counts[1]) return -2;
  if (params) { params[0] = min_val; params[1] = max_val; }
  if (max_val == min_val) max_val = min_val + 1.0;
  const Clamp c{(float)min_val, (float)max_val};
  const Normalize f((float)min_val, (float)max_val, (float)0.0, (float)255.0);
  for (size_t i = 0; i < (size_t)w * h; ++i) store(out_type, out, i, f(c(img[i])));
  if (params) { params[2] = min_val; params[3] = max_val; }
  return 0;
}

// normalize(image, low, high), AutoNormalize.h:33-49: UnaryCompoundFunctor applies the functor to the value of an invalid pixel
// too (PixelMask.h:514-523), so every pixel is converted; -1: no valid samples
int isr_auto_normalize(const float* img, int w, int h, const uint8_t* mask, double low, double high, float* out, double* params) {
  double mm[2];
  if (isr_min_max_channel_values(img, w, h, mask, 0, 0, mm)) return -1;
  const Normalize f((float)mm[0], (float)mm[1], (float)low, (float)high);
  for (size_t i = 0; i < (size_t)w * h; ++i) out[i] = f(img[i]);
  if (params) { params[0] = mm[0]; params[1] = mm[1]; params[2] = (float)low; params[3] = (float)high; }
  return 0;
}

}  // extern "C"
