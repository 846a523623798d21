// disparity_filters_ref.cc — CPU restatement (test infrastructure) of the disparity post-filters of
// src/vw/Stereo/Algorithms.{h,cc}: disparity_median_filter (Algorithms.cc:26-67, Math/Functors.h:393-398),
// disparity_neighbor_filter (Algorithms.cc:69-110), texture_measure (Algorithms.h:144-209) and
// texture_preserving_disparity_filter<float> (Algorithms.h:215-281).  Dependency-free; built with -ffp-contract=off.
//
// The three disparity filters begin with `disparity_out = disparity_in`, a shallow ImageView copy: both names then share
// one buffer and the raster-order loops read what they have already written.  semantics 0 ("reference") restates that
// literally: the filter runs in place on the caller's buffer and `out` receives a copy of it afterwards.  semantics 1
// ("snapshot") reads the unmodified input and writes a fresh image.  Every box {x, y, w, h} is filtered as an image of
// its own (its own border, edge extension and raster order); boxes must not overlap; pixels outside every box are copied.
// Layouts: disparity (rows, cols, 3) float32 or int32 {dx, dy, valid != 0}; images (rows, cols) float32.
// Outside the reference's contract, and left unchanged here: a median window with a NaN among its valid disparities, a
// pixel whose texture or window-size product is not finite.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

namespace {

struct Box {
  int x, y, w, h;
};

bool boxes_ok(const int* b, int n, int w, int h) {
  if (n < 0 || (n > 0 && !b)) return false;
  for (int i = 0; i < n; ++i) {
    const int* p = b + 4 * i;
    if (p[2] <= 0 || p[3] <= 0 || p[0] < 0 || p[1] < 0 || p[0] > w - p[2] || p[1] > h - p[3]) return false;
    for (int j = 0; j < i; ++j) {
      const int* q = b + 4 * j;
      if (p[0] < q[0] + q[2] && q[0] < p[0] + p[2] && p[1] < q[1] + q[3] && q[1] < p[1] + p[3]) return false;
    }
  }
  return true;
}

template <class F>
void for_boxes(const int* boxes, int n, int threads, F f) {
  const int nt = std::max(1, std::min(threads, n));
  std::vector<std::thread> pool;
  for (int t = 0; t < nt; ++t)
    pool.emplace_back([=] {
      for (int i = t; i < n; i += nt) f(Box{boxes[4 * i], boxes[4 * i + 1], boxes[4 * i + 2], boxes[4 * i + 3]}, t);
    });
  for (auto& th : pool) th.join();
}

// one box of an image of 3-word pixels, read from `src` and written to `dst` (the same buffer in reference semantics)
template <class T>
struct View {
  const T* src;
  T* dst;
  long long stride;   // pixels per image row
  Box b;
  const T* at(int c, int r) const { return src + ((long long)(b.y + r) * stride + b.x + c) * 3; }
  T* out(int c, int r) const { return dst + ((long long)(b.y + r) * stride + b.x + c) * 3; }
  const T* clamped(int c, int r) const { return at(std::min(std::max(c, 0), b.w - 1), std::min(std::max(r, 0), b.h - 1)); }
};

template <class T>
bool valid(const T* p) { return p[2] != 0; }

// a pixel is "changed" when the value written differs from the one it replaces in dx, dy or validity
long long put(float* o, float dx, float dy) {
  const bool same = o[2] != 0 && o[0] == dx && o[1] == dy;
  o[0] = dx; o[1] = dy; o[2] = 1.0f;
  return same ? 0 : 1;
}

double median_of(std::vector<double>& v) {   // math::destructive_median
  const int len = (int)v.size();
  std::sort(v.begin(), v.end());
  return len % 2 ? v[len / 2] : (v[len / 2 - 1] + v[len / 2]) / 2.0;
}

long long median_box(const View<float>& V, int k) {
  const int half = (k - 1) / 2;
  long long changed = 0;
  std::vector<double> dx, dy;
  for (int row = half; row < V.b.h - half; ++row)
    for (int col = half; col < V.b.w - half; ++col) {
      if (!valid(V.at(col, row))) continue;
      dx.clear(); dy.clear();
      bool nan = false;
      for (int r = row - half; r <= row + half; ++r)
        for (int c = col - half; c <= col + half; ++c) {
          const float* p = V.at(c, r);
          if (!valid(p)) continue;
          nan = nan || std::isnan(p[0]) || std::isnan(p[1]);
          dx.push_back(p[0]);
          dy.push_back(p[1]);
        }
      if (dx.empty() || nan) continue;
      const double mx = median_of(dx), my = median_of(dy);
      changed += put(V.out(col, row), (float)mx, (float)my);
    }
  return changed;
}

long long neighbor_box(const View<int32_t>& V) {
  static const int off[8][2] = {{-1, -1}, {0, -1}, {1, -1}, {-1, 0}, {1, 0}, {-1, 1}, {0, 1}, {1, 1}};
  long long changed = 0;
  for (int row = 1; row < V.b.h - 1; ++row)
    for (int col = 1; col < V.b.w - 1; ++col) {
      int32_t vals[8][3];
      for (int i = 0; i < 8; ++i) {
        const int32_t* p = V.at(col + off[i][0], row + off[i][1]);
        vals[i][0] = p[0]; vals[i][1] = p[1]; vals[i][2] = p[2] != 0;
      }
      int max_count = 0, max_index = 0;
      for (int i = 0; i < 8; ++i) {
        if (!vals[i][2]) continue;
        int count = 0;
        for (int j = 0; j < 8; ++j)
          if (vals[i][0] == vals[j][0] && vals[i][1] == vals[j][1] && vals[i][2] == vals[j][2]) ++count;
        if (count > max_count) {
          max_count = count;
          max_index = i;
        }
      }
      if (max_count < 5) continue;
      int32_t* o = V.out(col, row);
      const bool same = o[2] != 0 && o[0] == vals[max_index][0] && o[1] == vals[max_index][1];
      o[0] = vals[max_index][0]; o[1] = vals[max_index][1]; o[2] = 1;
      changed += same ? 0 : 1;
    }
  return changed;
}

long long smooth_box(const View<float>& V, const float* tex, long long tstride, float texture_max, int max_kernel) {
  const float texture_scale = max_kernel / texture_max;
  long long changed = 0;
  for (int row = 0; row < V.b.h; ++row)
    for (int col = 0; col < V.b.w; ++col) {
      const float t = tex[(long long)(V.b.y + row) * tstride + V.b.x + col];
      if (!valid(V.at(col, row)) || t < 0) continue;
      float adjusted = texture_max - t;
      if (adjusted < 0) adjusted = 0;
      const float prod = adjusted * texture_scale;
      if (!std::isfinite(t) || !std::isfinite(prod)) continue;   // undefined in the reference (floor -> int)
      int ks = (int)std::floor(prod);
      if (ks % 2 == 0) ks += 1;
      if (ks < 3 || ks > max_kernel) continue;
      const int half = (ks - 1) / 2;
      double sx = 0, sy = 0, count = 0;
      for (int r = row - half; r <= row + half; ++r)
        for (int c = col - half; c <= col + half; ++c) {
          const float* p = V.clamped(c, r);
          if (!valid(p)) continue;
          sx += p[0];
          sy += p[1];
          count += 1.0;
        }
      if (count < 1.0) continue;
      changed += put(V.out(col, row), (float)(sx / count), (float)(sy / count));
    }
  return changed;
}

// derivative_filter(img, 1, 0) / (img, 0, 1) at a pixel of the box (Filter.h:275-308): kernel {0.5, 0, -0.5}, constant
// edge extension, the three products added from 0 in float
float deriv(const float* img, long long stride, const Box& b, int c, int r, int dc, int dr) {
  auto I = [&](int cc, int rr) {
    cc = std::min(std::max(cc, 0), b.w - 1);
    rr = std::min(std::max(rr, 0), b.h - 1);
    return img[(long long)(b.y + rr) * stride + b.x + cc];
  };
  float s = 0.0f;
  s = s + -0.5f * I(c - dc, r - dr);
  s = s + 0.0f * I(c, r);
  s = s + 0.5f * I(c + dc, r + dr);
  return s;
}

void texture_box(const float* img, long long stride, const Box& b, int k, double gw, double sw, float* out, float* mx) {
  const int half = (k - 1) / 2;
  std::vector<float> g((size_t)b.w * b.h);
  for (int r = 0; r < b.h; ++r)
    for (int c = 0; c < b.w; ++c)
      g[(size_t)r * b.w + c] = std::fabs(deriv(img, stride, b, c, r, 1, 0)) + std::fabs(deriv(img, stride, b, c, r, 0, 1));
  auto cl = [](int v, int n) { return std::min(std::max(v, 0), n - 1); };
  for (int row = 0; row < b.h; ++row)
    for (int col = 0; col < b.w; ++col) {
      double mean = 0, count = 0;
      for (int r = row - half; r <= row + half; ++r)
        for (int c = col - half; c <= col + half; ++c) {
          mean += img[(long long)(b.y + cl(r, b.h)) * stride + b.x + cl(c, b.w)];
          count += 1.0;
        }
      mean /= count;
      double grad = 0, sd = 0;
      for (int r = row - half; r <= row + half; ++r)
        for (int c = col - half; c <= col + half; ++c) {
          const int cc = cl(c, b.w), rr = cl(r, b.h);
          grad += g[(size_t)rr * b.w + cc];
          const double d = img[(long long)(b.y + rr) * stride + b.x + cc] - mean;
          sd += d * d;   // pow(x, 2) is expanded to a multiply
        }
      grad = grad / (2.0 * count);
      sd = std::sqrt(sd / count);
      const float score = (float)(grad * gw + sd * sw);
      out[(long long)(b.y + row) * stride + b.x + col] = score;
      if (score > *mx) *mx = score;
    }
}

template <class T, class F>
int run(T* disp, int w, int h, int semantics, const int* boxes, int n, T* out, int threads, long long* changed, F f) {
  if (!disp || !out || w <= 0 || h <= 0 || semantics < 0 || semantics > 1 || !boxes_ok(boxes, n, w, h)) return 1;
  const size_t bytes = (size_t)w * h * 3 * sizeof(T);
  if (semantics == 1) std::memcpy(out, disp, bytes);
  std::vector<long long> part((size_t)std::max(threads, 1), 0);
  for_boxes(boxes, n, threads, [&](Box b, int t) {
    View<T> V{disp, semantics == 1 ? out : disp, w, b};
    part[(size_t)t] += f(V);
  });
  if (semantics == 0) std::memcpy(out, disp, bytes);
  if (changed) {
    *changed = 0;
    for (long long p : part) *changed += p;
  }
  return 0;
}

}  // namespace

extern "C" {

int dfr_median(float* disp, int w, int h, int kernel_size, int semantics, const int* boxes, int n, float* out, int threads,
               long long* changed) {
  return run(disp, w, h, semantics, boxes, n, out, threads, changed, [=](const View<float>& V) {
    return kernel_size < 3 ? 0LL : median_box(V, kernel_size);
  });
}

int dfr_neighbor(int32_t* disp, int w, int h, int semantics, const int* boxes, int n, int32_t* out, int threads,
                 long long* changed) {
  return run(disp, w, h, semantics, boxes, n, out, threads, changed, [=](const View<int32_t>& V) { return neighbor_box(V); });
}

int dfr_smooth(float* disp, int w, int h, const float* texture, float texture_max, int max_kernel_size, int semantics,
               const int* boxes, int n, float* out, int threads, long long* changed) {
  if (!texture) return 1;
  return run(disp, w, h, semantics, boxes, n, out, threads, changed, [=](const View<float>& V) {
    return (max_kernel_size < 3 || texture_max <= 0) ? 0LL : smooth_box(V, texture, w, texture_max, max_kernel_size);
  });
}

// out: (rows, cols) float32, zero outside the boxes; *max_score: the largest score written (0 when none)
int dfr_texture(const float* img, int w, int h, int kernel_size, double gradient_weight, double stddev_weight, const int* boxes,
                int n, float* out, int threads, float* max_score) {
  if (!img || !out || w <= 0 || h <= 0 || kernel_size < 1 || !boxes_ok(boxes, n, w, h)) return 1;
  std::memset(out, 0, (size_t)w * h * sizeof(float));
  std::vector<float> part((size_t)std::max(threads, 1), 0.0f);
  for_boxes(boxes, n, threads, [&](Box b, int t) {
    texture_box(img, w, b, kernel_size, gradient_weight, stddev_weight, out, &part[(size_t)t]);
  });
  if (max_score) {
    *max_score = 0.0f;
    for (float p : part) *max_score = std::max(*max_score, p);
  }
  return 0;
}

}  // extern "C"
