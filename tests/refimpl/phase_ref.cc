// phase_ref.cc — TEST INFRASTRUCTURE ONLY: a sequential CPU restatement of vw::stereo::phase_subpixel
// (PyramidSubpixelView with SUBPIXEL_PHASE, src/vw/Stereo/SubpixelView.cc:33-224, 275-289) and of its refiner
// subpixel_phase_2d / phase_correlation_subpixel / partial_upsample_dft (src/vw/Stereo/PhaseSubpixelView.cc:42-326) with
// fftshift and pad_fourier_transform (src/vw/Image/Fourier.cc:91-164).  The pyramid helpers come from the FAST_AFFINE
// restatement (affine_ref.cc, included).
//
// The reference's DFTs are OpenCV's, whose summation order is not reproducible; this file follows the arithmetic the
// project defines, written independently of the kernel:
//   - direct sums, one std::fma chain per output in ascending k; twiddles are double cos / sin of 2 pi k / n rounded to
//     float; a complex step (a + ib)(c + is) accumulates re += a c, then re += -b s, im += a s, then im += b c;
//   - the forward DFT transforms rows, then columns; the inverse (real output, DFT_SCALE) transforms the rows of the padded
//     spectrum over its columns, then takes the real part over its rows, and skips the entries pad_fourier_transform leaves
//     zero (they can only change the sign of a zero);
//   - partial_upsample_dft's kernels are std::exp of the reference's complex<float> expression;
//   - a maximum is the first element in row-major order strictly greater than a running maximum from -inf (index 0 if none);
//   - cv::magnitude is std::sqrt(float(re * re) + float(im * im)).
// get_dft first converts each patch to 8 bits with percentile_scale_convert (Fourier.cc:36-75, ImageThresh.h:244-268):
// percentile_u8 below, with the uint8 cast and int(round(...)) spelled as x86's cvtt conversions (NaN -> INT_MIN).
#include <climits>
#include <complex>
#include <limits>
#include <thread>

#include "affine_ref.cc"

namespace {

// fftshift (Fourier.cc:91-133) of a rows x cols image of ch floats per pixel
void fftshift(const float* in, int rows, int cols, int ch, bool reverse, float* out) {
  int cxo = cols / 2, cyo = rows / 2, cxi = cxo, cyi = cyo;
  if (cols % 2 != 0) ++cxi;
  if (rows % 2 != 0) ++cyi;
  if (reverse) {
    std::swap(cxo, cxi);
    std::swap(cyo, cyi);
  }
  // quadrant q of the input (origin ix, iy, size qw x qh) goes to the opposite quadrant's origin of the output
  const int qs[4][6] = {{0, 0, cxi, cyi, cxo, cyo},                           // q0_in -> q3_out
                        {cxi, 0, cols - cxi, cyi, 0, cyo},                    // q1_in -> q2_out
                        {0, cyi, cxi, rows - cyi, cxo, 0},                    // q2_in -> q1_out
                        {cxi, cyi, cols - cxi, rows - cyi, 0, 0}};            // q3_in -> q0_out
  for (const auto& q : qs)
    for (int y = 0; y < q[3]; ++y)
      for (int x = 0; x < q[2]; ++x)
        for (int c = 0; c < ch; ++c)
          out[((size_t)(q[5] + y) * cols + q[4] + x) * ch + c] = in[((size_t)(q[1] + y) * cols + q[0] + x) * ch + c];
}

// pad_fourier_transform (Fourier.cc:135-164), complex rows x cols -> new_h x new_w
std::vector<float> pad_fourier_transform(const std::vector<float>& in, int rows, int cols, int new_w, int new_h) {
  if (new_w == cols && new_h == rows) return in;
  std::vector<float> temp((size_t)new_w * new_h * 2, 0.0f), shifted(in.size()), out(temp.size());
  fftshift(in.data(), rows, cols, 2, false, shifted.data());
  const int cdx = (new_w / 2 + 1) - (cols / 2 + 1), cdy = (new_h / 2 + 1) - (rows / 2 + 1);
  const float scale = static_cast<float>(new_w * new_h) / static_cast<float>(cols * rows);
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x)
      for (int c = 0; c < 2; ++c) temp[((size_t)(cdy + y) * new_w + cdx + x) * 2 + c] = shifted[((size_t)y * cols + x) * 2 + c];
  fftshift(temp.data(), new_h, new_w, 2, true, out.data());
  for (auto& v : out) v = v * scale;
  return out;
}

struct Twiddle {
  std::vector<float> c, s;
  explicit Twiddle(int n) : c(n), s(n) {
    for (int k = 0; k < n; ++k) {
      const double ang = 2.0 * M_PI * (double)k / (double)n;
      c[k] = (float)std::cos(ang);
      s[k] = (float)std::sin(ang);
    }
  }
};

// static_cast<int>(double) as x86's cvttsd2si computes it: truncation; NaN and out-of-range values give INT_MIN
int cvtt(double x) { return (x >= -2147483648.0 && x < 2147483648.0) ? (int)x : INT_MIN; }

// percentile_scale_convert(input, out, 0.02, 0.98, 256) (ImageThresh.h:244-268), out as floats 0..255
void percentile_u8(const float* in, int n, float* out) {
  double min_val = -1.0, max_val = -1.0;
  max_val = -std::numeric_limits<double>::max();  // find_image_min_max (Image/Statistics.h:114-128)
  min_val = -max_val;
  for (int i = 0; i < n; ++i) {
    const double val = in[i];
    if (val < min_val) min_val = val;
    if (val > max_val) max_val = val;
  }
  // histogram(input, 256, min_val, max_val) (ImageThresh.h:52-70): its own copy of max_val
  const double hmax = max_val == min_val ? min_val + 1.0 : max_val;
  const int num_bins = 256, max_bin = num_bins - 1;
  const double range = hmax - min_val, bin_width = range / num_bins;
  std::vector<double> bins(num_bins, 0.0);
  for (int i = 0; i < n; ++i) {  // Histogram::add_value, saturate (Math/Statistics.cc:57-76)
    int bin = cvtt(std::round(max_bin * (((double)in[i] - min_val) / range)));
    if (bin < 0) bin = 0;
    if (bin >= num_bins) bin = max_bin;
    bins[bin] += 1.0;
  }
  auto percentile = [&](double p) -> size_t {  // Histogram::get_percentile (Statistics.cc:85-104)
    const double sum = static_cast<double>(n);
    double running = 0;
    for (int i = 0; i < num_bins; ++i) {
      running += bins[i] / sum;
      if (running >= p) return i;
    }
    return max_bin;  // the reference throws here; unreachable for 0.02 / 0.98
  };
  const size_t low_bin = percentile(0.02), high_bin = percentile(0.98);
  const double low_value = (low_bin + 1) * bin_width + min_val, high_value = (high_bin + 1) * bin_width + min_val;
  // clamp(input, low, high) with float bounds, normalize(., low, high, 0, 255) with float arguments, pixel_cast<uint8>
  const float lo = (float)low_value, hi = (float)high_value, new_min = 0.0f, new_max = 255.0f;
  const double ratio = hi == lo ? 0.0 : (new_max - new_min) / (double)(hi - lo);
  for (int i = 0; i < n; ++i) {
    float c = in[i];
    if (c > hi) c = hi;
    else if (c < lo) c = lo;
    const float norm = (float)((c - lo) * ratio + new_min);
    out[i] = (float)(uint8_t)(cvtt(norm) & 0xff);
  }
}

// get_dft of a real rows x cols patch: the 8-bit conversion, then the DFT; complex, interleaved
std::vector<float> dft_forward(const float* patch, int R, int C) {
  std::vector<float> u8((size_t)R * C);
  percentile_u8(patch, R * C, u8.data());
  const float* a = u8.data();
  const Twiddle tc(C), tr(R);
  std::vector<float> t((size_t)R * C * 2), f((size_t)R * C * 2);
  for (int y = 0; y < R; ++y)
    for (int v = 0; v < C; ++v) {
      float re = 0.0f, im = 0.0f;
      for (int x = 0; x < C; ++x) {
        const int k = (v * x) % C;
        re = std::fma(a[y * C + x], tc.c[k], re);
        im = std::fma(a[y * C + x], -tc.s[k], im);
      }
      t[2 * (y * C + v)] = re;
      t[2 * (y * C + v) + 1] = im;
    }
  for (int u = 0; u < R; ++u)
    for (int v = 0; v < C; ++v) {
      float re = 0.0f, im = 0.0f;
      for (int y = 0; y < R; ++y) {  // (a + ib)(c - is)
        const int k = (u * y) % R;
        const float a2 = t[2 * (y * C + v)], b2 = t[2 * (y * C + v) + 1], c = tr.c[k], s = -tr.s[k];
        re = std::fma(a2, c, re);
        re = std::fma(-b2, s, re);
        im = std::fma(a2, s, im);
        im = std::fma(b2, c, im);
      }
      f[2 * (u * C + v)] = re;
      f[2 * (u * C + v) + 1] = im;
    }
  return f;
}

// cv::minMaxLoc's location as defined here
int first_max(const std::vector<float>& v) {
  float best = -INFINITY;
  int idx = -1;
  for (size_t i = 0; i < v.size(); ++i)
    if (v[i] > best) {
      best = v[i];
      idx = (int)i;
    }
  return idx < 0 ? 0 : idx;
}

// fftshift(0 .. n-1, reverse = true) - floor(n / 2) (partial_upsample_dft's frequency vector)
std::vector<int> frequencies(int n) {
  std::vector<float> idx(n), sh(n);
  for (int i = 0; i < n; ++i) idx[i] = (float)i;
  fftshift(idx.data(), 1, n, 1, true, sh.data());
  std::vector<int> f(n);
  for (int i = 0; i < n; ++i) f[i] = (int)(sh[i] - std::floor(n / 2));
  return f;
}

std::complex<float> upsample_kernel(int m, int n, int upscale) {
  const std::complex<float> neg_i(0, -1);
  const float two_pi = 2.0 * M_PI;
  const std::complex<float> constant = neg_i * two_pi / static_cast<float>(n * upscale);
  return std::exp(std::complex<float>((float)m, 0.0f) * constant);
}

// partial_upsample_dft (PhaseSubpixelView.cc:42-101): row_kernel * input * col_kernel, returned up_h x up_w complex
std::vector<float> partial_upsample_dft(const std::vector<float>& in, int R, int C, int up_h, int up_w, int upscale, int row_off,
                                        int col_off) {
  const std::vector<int> fc = frequencies(C), fr = frequencies(R);
  std::vector<std::complex<float>> ck((size_t)C * up_w), rk((size_t)up_h * R);
  for (int i = 0; i < C; ++i)
    for (int j = 0; j < up_w; ++j) ck[(size_t)i * up_w + j] = upsample_kernel(fc[i] * (j - col_off), C, upscale);
  for (int i = 0; i < up_h; ++i)
    for (int j = 0; j < R; ++j) rk[(size_t)i * R + j] = upsample_kernel((i - row_off) * fr[j], R, upscale);
  auto cmac = [](float& re, float& im, float a, float b, float c, float s) {  // += (a + ib)(c + is)
    re = std::fma(a, c, re);
    re = std::fma(-b, s, re);
    im = std::fma(a, s, im);
    im = std::fma(b, c, im);
  };
  std::vector<float> o1((size_t)up_h * C * 2), out((size_t)up_h * up_w * 2);
  for (int i = 0; i < up_h; ++i)
    for (int c = 0; c < C; ++c) {
      float re = 0.0f, im = 0.0f;
      for (int r = 0; r < R; ++r) {
        const std::complex<float> e = rk[(size_t)i * R + r];
        cmac(re, im, e.real(), e.imag(), in[2 * (r * C + c)], in[2 * (r * C + c) + 1]);
      }
      o1[2 * (i * C + c)] = re;
      o1[2 * (i * C + c) + 1] = im;
    }
  for (int i = 0; i < up_h; ++i)
    for (int j = 0; j < up_w; ++j) {
      float re = 0.0f, im = 0.0f;
      for (int c = 0; c < C; ++c) {
        const std::complex<float> e = ck[(size_t)c * up_w + j];
        cmac(re, im, o1[2 * (i * C + c)], o1[2 * (i * C + c) + 1], e.real(), e.imag());
      }
      out[2 * (i * up_w + j)] = re;
      out[2 * (i * up_w + j) + 1] = im;
    }
  return out;
}

// phase_correlation_subpixel (PhaseSubpixelView.cc:103-229) of two rows x cols patches
void phase_correlation(const float* left, const float* right, int R, int C, int pad_factor, float* offset) {
  const std::vector<float> fl = dft_forward(left, R, C), fr = dft_forward(right, R, C);
  std::vector<float> x((size_t)R * C * 2);  // mulSpectrums(L, R, conjB = true)
  for (int i = 0; i < R * C; ++i) {
    x[2 * i] = fl[2 * i] * fr[2 * i] + fl[2 * i + 1] * fr[2 * i + 1];
    x[2 * i + 1] = fl[2 * i + 1] * fr[2 * i] - fl[2 * i] * fr[2 * i + 1];
  }
  const int W = 2 * C, H = 2 * R;
  const std::vector<float> p = pad_fourier_transform(x, R, C, W, H);
  // the entries pad_fourier_transform placed (the others are zero)
  std::vector<float> ones((size_t)R * C * 2, 1.0f);
  const std::vector<float> placed = pad_fourier_transform(ones, R, C, W, H);
  std::vector<int> rows_used, cols_used;
  for (int u = 0; u < H; ++u)
    if (placed[2 * ((size_t)u * W)] != 0.0f || placed[2 * ((size_t)u * W + 1)] != 0.0f) rows_used.push_back(u);
  for (int v = 0; v < W; ++v)
    if (placed[2 * (size_t)v] != 0.0f) cols_used.push_back(v);
  const Twiddle t2c(W), t2r(H);
  std::vector<float> g((size_t)H * W * 2, 0.0f), conv((size_t)H * W);
  for (int u : rows_used)
    for (int xx = 0; xx < W; ++xx) {
      float re = 0.0f, im = 0.0f;
      for (int v : cols_used) {  // (a + ib)(c + is)
        const int k = (int)(((long long)v * xx) % W);
        const float a = p[2 * ((size_t)u * W + v)], b = p[2 * ((size_t)u * W + v) + 1];
        re = std::fma(a, t2c.c[k], re);
        re = std::fma(-b, t2c.s[k], re);
        im = std::fma(a, t2c.s[k], im);
        im = std::fma(b, t2c.c[k], im);
      }
      g[2 * ((size_t)u * W + xx)] = re;
      g[2 * ((size_t)u * W + xx) + 1] = im;
    }
  const float invs = (float)(1.0 / (4.0 * R * C));
  for (int y = 0; y < H; ++y)
    for (int xx = 0; xx < W; ++xx) {
      float acc = 0.0f;
      for (int u : rows_used) {
        const int k = (int)(((long long)u * y) % H);
        acc = std::fma(g[2 * ((size_t)u * W + xx)], t2r.c[k], acc);
        acc = std::fma(-g[2 * ((size_t)u * W + xx) + 1], t2r.s[k], acc);
      }
      conv[(size_t)y * W + xx] = acc * invs;
    }
  const int loc = first_max(conv), lx = loc % W, ly = loc / W;
  float initial_shift_x = (lx < W / 2) ? lx : (lx - W);
  float initial_shift_y = (ly < H / 2) ? ly : (ly - H);
  initial_shift_x /= 2.0f;
  initial_shift_y /= 2.0f;
  if (pad_factor <= 2) {
    offset[0] = initial_shift_x;
    offset[1] = initial_shift_y;
    return;
  }
  const float UPSAMPLE_REGION_FACTOR = 1.5;
  // ::round / ::ceil / ::floor of double (Math/Functions.h brings the C library's into namespace vw)
  float shift_x = ::round((double)(initial_shift_x * pad_factor)) / pad_factor;
  float shift_y = ::round((double)(initial_shift_y * pad_factor)) / pad_factor;
  const float dft_shift = ::floor(::ceil((double)(pad_factor * UPSAMPLE_REGION_FACTOR)) / 2);
  const int up = ::ceil((double)(pad_factor * UPSAMPLE_REGION_FACTOR));
  std::vector<float> nc(x.size());  // mulSpectrums(R, L, conjB = true)
  for (int i = 0; i < R * C; ++i) {
    nc[2 * i] = fr[2 * i] * fl[2 * i] + fr[2 * i + 1] * fl[2 * i + 1];
    nc[2 * i + 1] = fr[2 * i + 1] * fl[2 * i] - fr[2 * i] * fl[2 * i + 1];
  }
  const std::vector<float> pu =
      partial_upsample_dft(nc, R, C, up, up, pad_factor, (int)(dft_shift - shift_y * pad_factor), (int)(dft_shift - shift_x * pad_factor));
  std::vector<float> mag((size_t)up * up);
  for (size_t i = 0; i < mag.size(); ++i) {
    const float re2 = pu[2 * i] * pu[2 * i], im2 = pu[2 * i + 1] * pu[2 * i + 1];
    mag[i] = std::sqrt(re2 + im2);
  }
  const int l2 = first_max(mag);
  const int my = (int)(l2 / up - dft_shift), mx = (int)(l2 % up - dft_shift);
  shift_y = shift_y + static_cast<float>(my) / static_cast<float>(pad_factor);
  shift_x = shift_x + static_cast<float>(mx) / static_cast<float>(pad_factor);
  offset[0] = shift_x;
  offset[1] = shift_y;
}

int floor_i(double v) {  // math::impl::_floor
  if (v < 0) {
    const int iv = (int)v;
    return (double)iv == v ? iv : iv - 1;
  }
  return (int)v;
}

// BicubicInterpolation (Interpolation.h:138-185) over ZeroEdgeExtension
float bicubic_zero(const FImg& r, double i, double j) {
  const int x = floor_i(i), y = floor_i(j);
  if (x == i && y == j) return r.zero_ext(x, y);
  const double normx = i - x, normy = j - y;
  const double s0 = ((2 - normx) * normx - 1) * normx, t0 = ((2 - normy) * normy - 1) * normy;
  const double s1 = (3 * normx - 5) * normx * normx + 2, t1 = (3 * normy - 5) * normy * normy + 2;
  const double s2 = ((4 - 3 * normx) * normx + 1) * normx, t2 = ((4 - 3 * normy) * normy + 1) * normy;
  const double s3 = (normx - 1) * normx * normx, t3 = (normy - 1) * normy * normy;
  double row = s0 * r.zero_ext(x - 1, y - 1);
  row += s1 * r.zero_ext(x, y - 1);
  row += s2 * r.zero_ext(x + 1, y - 1);
  row += s3 * r.zero_ext(x + 2, y - 1);
  double result = t0 * row;
  row = s0 * r.zero_ext(x - 1, y);
  row += s1 * r.zero_ext(x, y);
  row += s2 * r.zero_ext(x + 1, y);
  row += s3 * r.zero_ext(x + 2, y);
  result += t1 * row;
  row = s0 * r.zero_ext(x - 1, y + 1);
  row += s1 * r.zero_ext(x, y + 1);
  row += s2 * r.zero_ext(x + 1, y + 1);
  row += s3 * r.zero_ext(x + 2, y + 1);
  result += t2 * row;
  row = s0 * r.zero_ext(x - 1, y + 2);
  row += s1 * r.zero_ext(x, y + 2);
  row += s2 * r.zero_ext(x + 1, y + 2);
  row += s3 * r.zero_ext(x + 2, y + 2);
  result += t3 * row;
  result *= 0.25;
  return (float)result;
}

// subpixel_phase_2d (PhaseSubpixelView.cc:231-326), use_second_refinement = true.  Pixels are independent; rows are split
// over nthreads threads.
void phase_2d(DImg& D, const FImg& L, const FImg& R, int kw, int kh, int rx0, int ry0, int rx1, int ry1, int accuracy,
              int nthreads, long long* stats) {
  const float SUBPIXEL_MAX_TRANSLATION = 3.0;
  const int khh = kh / 2, khw = kw / 2;
  const int y0 = std::max(ry0 - 1, khh), y1 = std::min(L.h - khh, ry1 + 1);
  const int x0 = std::max(rx0 - 1, khw), x1 = std::min(L.w - khw, rx1 + 1);
  if (y1 <= y0 || x1 <= x0) return;
  std::vector<long long> refined(nthreads, 0), invalidated(nthreads, 0);
  auto work = [&](int tid) {
    std::vector<float> lp((size_t)kw * kh), rp((size_t)kw * kh);
    for (int y = y0 + tid; y < y1; y += nthreads)
      for (int x = x0; x < x1; ++x) {
        const size_t p = D.at(x, y);
        if (!D.v[p]) continue;
        const int wx = x - khw, wy = y - khh;
        const int rwx = wx + (int)D.dx[p], rwy = wy + (int)D.dy[p];  // + Vector2i(disparity)
        for (int j = 0; j < kh; ++j)
          for (int i = 0; i < kw; ++i) {
            lp[(size_t)j * kw + i] = L.at(wx + i, wy + j);
            rp[(size_t)j * kw + i] = R.zero_ext(rwx + i, rwy + j);  // bilinear at integer positions: the pixel
          }
        float d[2], d2[2];
        phase_correlation(lp.data(), rp.data(), kh, kw, accuracy / 2, d);
        for (int j = 0; j < kh; ++j)
          for (int i = 0; i < kw; ++i) rp[(size_t)j * kw + i] = bicubic_zero(R, (double)(rwx + i) - (double)d[0], (double)(rwy + j) - (double)d[1]);
        phase_correlation(lp.data(), rp.data(), kh, kw, accuracy, d2);
        d[0] += d2[0];
        d[1] += d2[1];
        ++refined[tid];
        if (norm_2(d, 2) > SUBPIXEL_MAX_TRANSLATION || std::isnan(d[0]) || std::isnan(d[1])) {
          D.v[p] = 0;
          ++invalidated[tid];
        } else {
          D.dx[p] -= d[0];
          D.dy[p] -= d[1];
        }
      }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < nthreads; ++t) pool.emplace_back(work, t);
  work(0);
  for (auto& t : pool) t.join();
  if (stats)
    for (int t = 0; t < nthreads; ++t) {
      stats[0] += refined[t];
      stats[1] += invalidated[t];
    }
}

}  // namespace

extern "C" {

void phr_fftshift(const float* in, int rows, int cols, int ch, int reverse, float* out) {
  fftshift(in, rows, cols, ch, reverse != 0, out);
}

void phr_pad_fourier_transform(const float* in, int rows, int cols, int new_w, int new_h, float* out) {
  const std::vector<float> v(in, in + (size_t)rows * cols * 2);
  const std::vector<float> o = pad_fourier_transform(v, rows, cols, new_w, new_h);
  std::memcpy(out, o.data(), o.size() * 4);
}

void phr_percentile_u8(const float* in, int n, float* out) { percentile_u8(in, n, out); }

void phr_phase_correlation(const float* left, const float* right, int rows, int cols, int pad_factor, float* offset) {
  phase_correlation(left, right, rows, cols, pad_factor, offset);
}

// One call = PyramidSubpixelView(SUBPIXEL_PHASE)::prerasterize(bbox) for each of the ntiles boxes {x, y, w, h}, written
// into out3 (w x h x 3); as afr_pyramid_subpixel (affine_ref.cc).  Returns 0, -1 on bad arguments.
// stats (may be NULL, 3 entries): [0] += pixels refined, [1] += pixels invalidated, [2] += tiles.
int phr_phase_subpixel(const float* disp3, int w, int h, const float* left, const float* right, int rw, int rh, int mode,
                       float width, int kx, int ky, int max_levels, int accuracy, const int* tiles, int ntiles, float* out3,
                       int nthreads, long long* stats) {
  if (!disp3 || !left || !right || !out3 || w <= 0 || h <= 0 || rw <= 0 || rh <= 0) return -1;
  if (kx < 1 || ky < 1 || !(kx & 1) || !(ky & 1)) return -1;
  if (nthreads < 1) nthreads = 1;
  if (max_levels < 0) max_levels = 0;
  for (int t = 0; t < ntiles; ++t) {
    const int bx = tiles[4 * t], by = tiles[4 * t + 1], bw = tiles[4 * t + 2], bh = tiles[4 * t + 3];
    if (bw <= 0 || bh <= 0 || bx < 0 || by < 0 || bx + bw > w || by + bh > h) return -1;
  }
  for (int t = 0; t < ntiles; ++t) {
    const int bx = tiles[4 * t], by = tiles[4 * t + 1], bw = tiles[4 * t + 2], bh = tiles[4 * t + 3];
    // get_disparity_range (SubpixelView.cc:42) over the tile's valid pixels (tile_range.h)
    int rng[4];
    tile_disparity_range(disp3, w, tiles + 4 * t, rng);
    const int sminx = rng[0], sminy = rng[1], smaxx = rng[2], smaxy = rng[3];
    const int pw = bw + (smaxx - sminx) + 2 * kx, ph = bh + (smaxy - sminy) + 2 * ky;
    const int lx0 = bx - kx, ly0 = by - ky, rx0 = bx + sminx - kx, ry0 = by + sminy - ky;
    FImg L, R;
    L.resize(pw, ph);
    R.resize(pw, ph);
    if (vwo_prefilter_region(left, w, h, mode, width, lx0, ly0, pw, ph, L.p.data())) return -1;
    if (vwo_prefilter_region(right, rw, rh, mode, width, rx0, ry0, pw, ph, R.p.data())) return -1;
    DImg D;
    D.resize(pw, ph);
    for (int y = 0; y < ph; ++y)
      for (int x = 0; x < pw; ++x) {
        const int sx = lx0 + x, sy = ly0 + y;
        const size_t o = D.at(x, y);
        float vx = 0, vy = 0;
        uint8_t vv = 0;
        if (sx >= 0 && sy >= 0 && sx < w && sy < h) {
          const float* q = disp3 + ((size_t)sy * w + sx) * 3;
          vx = q[0];
          vy = q[1];
          vv = q[2] != 0.0f;
        }
        D.dx[o] = vx - (float)sminx;
        D.dy[o] = vy - (float)sminy;
        D.v[o] = vv;
      }
    std::vector<FImg> lp, rp;
    std::vector<int> roi;
    DImg ds = D;
    for (int i = 0; i < max_levels; ++i) {
      if (i > 0) {
        lp.push_back(subsample2(lp.back()));
        rp.push_back(subsample2(rp.back()));
        ds = disparity_subsample(ds);
        const size_t b = roi.size() - 4;
        roi.insert(roi.end(), {roi[b] / 2, roi[b + 1] / 2, roi[b + 2] / 2, roi[b + 3] / 2});
      } else {
        lp.push_back(subsample2(L));
        rp.push_back(subsample2(R));
        ds = disparity_subsample(D);
        roi.insert(roi.end(), {kx / 2, ky / 2, (kx + bw) / 2, (ky + bh) / 2});
      }
    }
    for (int i = max_levels - 1; i >= 0; --i) {
      phase_2d(ds, lp[i], rp[i], kx, ky, roi[4 * i], roi[4 * i + 1], roi[4 * i + 2], roi[4 * i + 3], accuracy, nthreads, stats);
      const int W = i > 0 ? lp[i - 1].w : pw, H = i > 0 ? lp[i - 1].h : ph;
      ds = upsample_crop(ds, W, H);
    }
    phase_2d(ds, L, R, kx, ky, kx, ky, kx + bw, ky + bh, accuracy, nthreads, stats);
    for (int y = by; y < by + bh; ++y)
      for (int x = bx; x < bx + bw; ++x) {
        const size_t k = ds.at(x - bx + kx, y - by + ky);
        float* o = out3 + ((size_t)y * w + x) * 3;
        if (ds.v[k]) {
          o[0] = ds.dx[k] + (float)sminx;
          o[1] = ds.dy[k] + (float)sminy;
          o[2] = 1.0f;
        } else {
          o[0] = o[1] = o[2] = 0.0f;
        }
      }
    if (stats) stats[2] += 1;
  }
  return 0;
}

}  // extern "C"
