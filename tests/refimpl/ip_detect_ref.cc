// CPU restatement of the interest-point detectors and descriptors that ipfind uses without OpenCV (test infrastructure
// only): IntegralImage, the box filter and the OBALoG interest planes, the extrema / threshold / Harris loops of
// IntegralAutoGainDetector and IntegralInterestPointDetector with their order and cull, AssignOrientation,
// SGradDescriptorGenerator and SGrad2DescriptorGenerator on a zero-extended crop.  Literal serial loops, one point and one
// pixel after the other, nothing shared with the kernels except the OBALoG numbers (ip_obalog.h, entered once) and the
// atan2f form (ip_atan2.h), which can be switched to libm's atan2f.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../visionworkbench_amd/csrc/ip_atan2.h"
#include "../../visionworkbench_amd/csrc/ip_obalog.h"

namespace {

long long g_harris_outside = 0;      // Harris reads that left the interest plane, over every call so far

struct Img {
  const float* p; long long stride; int w, h;
  float at(int x, int y) const { return p[(long long)y * stride + x]; }
};

void integral_of(const Img& src, float* out) {
  const int W = src.w + 1;
  for (int x = 0; x <= src.w; ++x) out[x] = 0;
  for (int y = 1; y <= src.h; ++y) out[(long long)y * W] = 0;
  for (int iy = 0; iy < src.h; ++iy)
    for (int ix = 0; ix < src.w; ++ix) {
      float* p = out + (long long)(iy + 1) * W + (ix + 1);
      *p = src.at(ix, iy) + *(p - 1) + *(p - W) - *(p - W - 1);
    }
}

struct Box { int sx, sy, w, h; float weight; };

float box_at(const float* I, int W, int x, int y, const Box* box, int n) {
  float result = 0;
  for (int b = 0; b < n; ++b) {
    const float* p = I + (long long)y * W + x;
    float box_sum = 0;
    p += (long long)box[b].sy * W + box[b].sx;
    box_sum += *p;
    p += box[b].w;
    box_sum -= *p;
    p += (long long)box[b].h * W - box[b].w;
    box_sum -= *p;
    p += box[b].w;
    box_sum += *p;
    result += box[b].weight * box_sum;
  }
  return result;
}

void box_filter(const float* I, int w, int h, const Box* box, int n, float* out, bool absolute) {
  int m = 0;
  for (int b = 0; b < n; ++b) m = std::max(m, std::max(box[b].w, box[b].h));
  const int pb = m >> 1, W = w + 1;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      float v = 0;
      if (!(x < pb || x >= W - pb - 1 || y < pb || y >= (h + 1) - pb - 1)) v = box_at(I, W, x, y, box, n);
      out[(long long)y * w + x] = absolute ? std::fabs(v) : v;
    }
}

void obalog_boxes(int scale, Box* box) {
  for (int b = 0; b < IPO_BOXES; ++b) {
    const ipo_box t = ipo_box_of(scale, b);
    box[b] = Box{-(t.w >> 1), -(t.h >> 1), t.w, t.h, (float)t.weight};
  }
}

void gaussian_2_9(double* g) {
  double sum = 0.0, tap;
  const double z = 1 / (std::sqrt(2.0) * 2.0);
  for (int i = 1; i <= 4; ++i) {
    tap = std::erf((i + 0.5) * z) - std::erf((i - 0.5) * z);
    sum += tap;
    g[4 + i] = g[4 - i] = tap;
  }
  sum *= 2.0;
  tap = std::erf(0.5 * z) - std::erf(-0.5 * z);
  sum += tap;
  g[4] = tap;
  const double norm = 1.0 / sum;
  for (int i = 0; i < 9; ++i) g[i] *= norm;
}

struct Plane {
  std::vector<float> v; int w, h;
  float at(int x, int y) const {
    if (x < 0 || y < 0 || x >= w || y >= h) { ++g_harris_outside; return 0; }
    return v[(long long)y * w + x];
  }
};

struct Point { float x, y; int ix, iy; float orientation, scale, interest; };

bool threshold(const Point& ip, const Plane& P, float scale, double thr, const double* g) {
  if (ip.interest < thr) return false;
  const int step = (int)scale, offset = 4 * step;
  float sum_Lx_2 = 0, sum_Ly_2 = 0, sum_LxLy = 0;
  for (int y = ip.iy - offset, iy = 0; y <= ip.iy + offset; y += step, iy++)
    for (int x = ip.ix - offset, ix = 0; x <= ip.ix + offset; x += step, ix++) {
      const float Lx = P.at(x - 1, y) - P.at(x + 1, y);
      const float Ly = P.at(x, y - 1) - P.at(x, y + 1);
      const float weight = g[ix] * g[iy];
      sum_Lx_2 += Lx * Lx * weight;
      sum_Ly_2 += Ly * Ly * weight;
      sum_LxLy += Lx * Ly * weight;
    }
  const float trace = sum_Lx_2 + sum_Ly_2;
  const float det = sum_Lx_2 * sum_Ly_2 - sum_LxLy * sum_LxLy;
  return (trace * trace) / det < 12;
}

bool is_extrema(const Plane& lo, const Plane& mid, const Plane& hi, int x, int y) {
  const float m = mid.v[(long long)y * mid.w + x];
  auto at = [&](const Plane& p, int dx, int dy) { return p.v[(long long)(y + dy) * p.w + (x + dx)]; };
  if (m <= at(lo, 0, 0)) return false;
  if (m <= at(hi, 0, 0)) return false;
  const int ring[8][2] = {{-1, -1}, {0, -1}, {1, -1}, {1, 0}, {1, 1}, {0, 1}, {-1, 1}, {-1, 0}};
  for (int s = 0; s < 8; ++s)
    if (m <= at(lo, ring[s][0], ring[s][1]) || m <= at(mid, ring[s][0], ring[s][1]) || m <= at(hi, ring[s][0], ring[s][1])) return false;
  return true;
}

// BilinearInterpolation over ConstantEdgeExtension (edge 1) or ZeroEdgeExtension (edge 0)
struct View {
  const float* p; int w, h, edge;
  float px(int x, int y) const {
    if (edge) { x = x < 0 ? 0 : x >= w ? w - 1 : x; y = y < 0 ? 0 : y >= h ? h - 1 : y; }
    else if (x < 0 || y < 0 || x >= w || y >= h) return 0;
    return p[(long long)y * w + x];
  }
  float operator()(double i, double j) const {
    const int x = (int)std::floor(i), y = (int)std::floor(j);
    if (x == i && y == j) return px(x, y);
    const float normx = float(i) - float(x), normy = float(j) - float(y), norm1mx = 1 - normx, norm1my = 1 - normy;
    float result = px(x, y) * norm1mx;
    result += px(x + 1, y) * normx;
    result *= norm1my;
    float row = px(x, y + 1) * norm1mx;
    row += px(x + 1, y + 1) * normx;
    result += row * normy;
    return result;
  }
};

float hhaar(const View& I, double x, double y, float size) {
  float response;
  const float half_size = size / 2.0;
  const float top = float(y) - half_size;
  const float left = float(x) - half_size;
  response = -I(left, top);
  response += 2 * I(left + half_size, top);
  response -= I(left + size, top);
  response += I(left, top + size);
  response -= 2 * I(left + half_size, top + size);
  response += I(left + size, top + size);
  return response;
}

float vhaar(const View& I, double x, double y, float size) {
  float response;
  const float half_size = size / 2.0;
  const float top = float(y) - half_size;
  const float left = float(x) - half_size;
  response = -I(left, top);
  response += I(left + size, top);
  response += 2 * I(left, top + half_size);
  response -= 2 * I(left + size, top + half_size);
  response -= I(left, top + size);
  response += I(left + size, top + size);
  return response;
}

float atan2_of(float y, float x, bool libm) { return libm ? atan2f(y, x) : ipa_atan2f(y, x); }

float orientation_of(const View& I, int ix, int iy, float scale, bool libm) {
  float h_response[169], v_response[169], angle[169];
  int m = 0;
  for (int i = -6; i <= 6; i++)
    for (int j = -6; j <= 6; j++) {
      const float distance_2 = i * i + j * j;
      if (distance_2 > 36) continue;
      const float weight = std::exp((double)(-distance_2 / 8)) / 5.0133;
      const double lx = (double)ix + (double)scale * (double)i, ly = (double)iy + (double)scale * (double)j;
      h_response[m] = weight * hhaar(I, lx, ly, scale * 4);
      v_response[m] = weight * vhaar(I, lx, ly, scale * 4);
      angle[m] = atan2_of(v_response[m], h_response[m], libm);
      m++;
    }
  static const float pi_6 = M_PI / 6.0;
  static const float two_pi = 2 * M_PI;
  float sumx, sumy, mod, greatest_mod = 0, greatest_ori = 0;
  for (float a = 0; a < two_pi; a += 0.5) {
    sumx = sumy = 0;
    for (int idx = 0; idx < m; idx++)
      if ((angle[idx] > a - pi_6 && angle[idx] < a + pi_6) || (angle[idx] + two_pi > a - pi_6 && angle[idx] + two_pi < a + pi_6) ||
          (angle[idx] - two_pi > a - pi_6 && angle[idx] - two_pi < a + pi_6)) {
        sumx += h_response[idx];
        sumy += v_response[idx];
      }
    mod = sumx * sumx + sumy * sumy;
    if (mod > greatest_mod) {
      greatest_mod = mod;
      greatest_ori = atan2_of(sumy, sumx, libm);
    }
  }
  return greatest_ori;
}

}  // namespace

extern "C" {

void idr_integral(const float* src, int w, int h, long long stride, float* out) { integral_of(Img{src, stride, w, h}, out); }

// boxes: int[n][4] = start x, start y, width, height
float idr_box_at(const float* integral, int w, int x, int y, int n, const int* boxes, const float* weights) {
  std::vector<Box> b(n);
  for (int k = 0; k < n; ++k) b[k] = Box{boxes[4 * k], boxes[4 * k + 1], boxes[4 * k + 2], boxes[4 * k + 3], weights[k]};
  return box_at(integral, w + 1, x, y, b.data(), n);
}

void idr_box_filter(const float* integral, int w, int h, int n, const int* boxes, const float* weights, float* out) {
  std::vector<Box> b(n);
  for (int k = 0; k < n; ++k) b[k] = Box{boxes[4 * k], boxes[4 * k + 1], boxes[4 * k + 2], boxes[4 * k + 3], weights[k]};
  box_filter(integral, w, h, b.data(), n, out, false);
}

void idr_plane(const float* integral, int w, int h, int scale, float* out) {
  Box b[IPO_BOXES];
  obalog_boxes(scale, b);
  box_filter(integral, w, h, b, IPO_BOXES, out, true);
}

long long idr_harris_outside() { return g_harris_outside; }

float idr_atan2f(float y, float x, int libm) { return atan2_of(y, x, libm != 0); }

float idr_haar(const float* integral, int iw, int ih, double x, double y, float size, int vertical) {
  const View I{integral, iw, ih, 1};
  return vertical ? vhaar(I, x, y, size) : hhaar(I, x, y, size);
}

float idr_orientation(const float* integral, int iw, int ih, int ix, int iy, float scale, int libm) {
  return orientation_of(View{integral, iw, ih, 1}, ix, iy, scale, libm != 0);
}

// process_image of the detector on the w x h crop at (x0, y0) of img, the points shifted by (x0, y0).  detector 0 = IAGD,
// 1 = OBALoG.  out: seven arrays of `cap` elements; stats = {extrema, passed, written}.  Returns written, or -1 when it exceeds cap.
int idr_detect(const float* img, long long stride, int x0, int y0, int w, int h, int detector, int scales, double thr, int max_points,
               int desired, int libm, int cap, float* ox, float* oy, int* oix, int* oiy, float* oori, float* oscale, float* ointerest,
               int* stats) {
  std::vector<float> integral((size_t)(w + 1) * (h + 1));
  integral_of(Img{img + (long long)y0 * stride + x0, stride, w, h}, integral.data());
  double g[9];
  gaussian_2_9(g);
  std::vector<Plane> planes(scales);
  for (int s = 0; s < scales; ++s) {
    planes[s].w = w; planes[s].h = h; planes[s].v.resize((size_t)w * h);
    idr_plane(integral.data(), w, h, s, planes[s].v.data());
  }
  std::vector<Point> points;
  stats[0] = stats[1] = stats[2] = 0;
  const int shift = detector == 1 ? 2 : 1;
  for (int scale = 2; scale < scales; scale++) {
    const Plane &lo = planes[scale - 2], &mid = planes[scale - 1], &hi = planes[scale];
    std::vector<Point> scale_points;
    const int cols = w - 2, rows = h - 2;
    for (int r = 0; r < rows; r++)
      for (int c = 0; c < cols; c++)
        if (is_extrema(lo, mid, hi, c + 1, r + 1)) {
          Point p{};
          p.x = float(c + shift); p.y = float(r + shift); p.ix = int(p.x); p.iy = int(p.y);
          p.scale = float(ipo_sigma(scale - 1)); p.interest = mid.v[(long long)(r + 1) * w + (c + 1)];
          scale_points.push_back(p);
        }
    stats[0] += (int)scale_points.size();
    float threshold_lvl = 0;
    if (detector == 0) {
      float imin = mid.v[0], imax = mid.v[0];
      for (float v : mid.v) { if (v < imin) imin = v; if (v > imax) imax = v; }
      threshold_lvl = imin + 0.001 * (imax - imin);
    }
    for (const Point& p : scale_points) {
      if (detector == 0 && p.interest < threshold_lvl) continue;
      if (!threshold(p, mid, float(ipo_sigma(scale - 1)), detector == 0 ? 0.0 : thr, g)) continue;
      points.push_back(p);
    }
  }
  stats[1] = (int)points.size();
  int curr_max_points = max_points;
  if (desired > 0) curr_max_points = desired;
  const auto by_interest = [](const Point& a, const Point& b) { return b.interest < a.interest; };
  if (detector == 1) {
    if (curr_max_points > 0) {
      std::stable_sort(points.begin(), points.end(), by_interest);
      if (curr_max_points < (int)points.size()) points.resize(curr_max_points);
    }
    const View I{integral.data(), w + 1, h + 1, 1};
    for (Point& p : points) p.orientation = orientation_of(I, p.ix, p.iy, p.scale, libm != 0);
  } else if (curr_max_points < (int)points.size() && curr_max_points > 0) {
    std::stable_sort(points.begin(), points.end(), by_interest);
    points.resize(curr_max_points);
  }
  stats[2] = (int)points.size();
  if ((int)points.size() > cap) return -1;
  for (size_t i = 0; i < points.size(); ++i) {
    Point p = points[i];
    p.x += x0; p.ix += x0; p.y += y0; p.iy += y0;
    ox[i] = p.x; oy[i] = p.y; oix[i] = p.ix; oiy[i] = p.iy; oori[i] = p.orientation; oscale[i] = p.scale; ointerest[i] = p.interest;
  }
  return (int)points.size();
}

// One generator call on crop(edge_extend(img, ZeroEdgeExtension()), crop): kind 0 = SGrad (180 floats), 1 = SGrad2 (128).
// x, y are image coordinates and are re-based to the crop as floats.
void idr_describe(const float* img, long long stride, int w, int h, const int* crop, int n, const float* xs, const float* ys,
                  const float* scales, const float* oris, int kind, float* desc) {
  const int cx = crop[0], cy = crop[1], cw = crop[2], ch = crop[3];
  std::vector<float> image((size_t)cw * ch);
  for (int y = 0; y < ch; ++y)
    for (int x = 0; x < cw; ++x) {
      const int gx = x + cx, gy = y + cy;
      image[(size_t)y * cw + x] = gx >= 0 && gy >= 0 && gx < w && gy < h ? img[(long long)gy * stride + gx] : 0.0f;
    }
  if (kind == 0) {
    const int S = 42;
    static const int box_strt[5] = {17, 15, 9, 6, 0}, box_size[5] = {2, 4, 8, 10, 14}, box_half[5] = {1, 2, 4, 5, 7};
    const View src{image.data(), cw, ch, 0};
    for (int k = 0; k < n; ++k) {
      float ptx = xs[k], pty = ys[k];
      ptx -= cx; pty -= cy;
      const float half_size = ((float)(S - 1)) / 2.0f;
      const float scaling = 1.0f / scales[k];
      const double c = cos((double)(-oris[k])), s = sin((double)(-oris[k]));
      const double ma = scaling * c, mb = -scaling * s, mc = scaling * s, md = scaling * c;
      const double mx = scaling * (s * pty - c * ptx) + half_size, my = -scaling * (s * ptx + c * pty) + half_size;
      const double det = ma * md - mb * mc;
      const double ai = md / det, bi = -mb / det, ci = -mc / det, di = ma / det;
      float support[S * S], iimage[(S + 1) * (S + 1)];
      for (int j = 0; j < S; ++j)
        for (int i = 0; i < S; ++i) {
          const double px = i - mx, py = j - my;
          support[j * S + i] = src(ai * px + bi * py, ci * px + di * py);
        }
      integral_of(Img{support, S, S, S}, iimage);
      const int W = S + 1;
      auto block = [&](int tx, int ty, int bx, int by) {
        float result = 0;
        result = iimage[ty * W + tx];
        result += iimage[by * W + bx];
        result -= iimage[by * W + tx];
        result -= iimage[ty * W + bx];
        return result;
      };
      float* first = desc + (size_t)k * 180;
      float* fill = first;
      float sqr_length = 0;
      for (int sc = 0; sc < 5; sc++) {
        const float inv_bh2 = 1 / float(box_half[sc] * box_half[sc]);
        for (int i = 0; i < 3; i++)
          for (int j = 0; j < 3; j++) {
            const int tx = box_strt[sc] + i * box_size[sc], ty = box_strt[sc] + j * box_size[sc], bh = box_half[sc];
            float minor_quad[4];
            minor_quad[0] = block(tx, ty, tx + bh, ty + bh);
            minor_quad[1] = block(tx + bh, ty, tx + 2 * bh, ty + bh);
            minor_quad[2] = block(tx, ty + bh, tx + bh, ty + 2 * bh);
            minor_quad[3] = block(tx + bh, ty + bh, tx + 2 * bh, ty + 2 * bh);
            *fill = (minor_quad[0] - minor_quad[2]) * inv_bh2; sqr_length += (*fill) * (*fill); fill++;
            *fill = (minor_quad[1] - minor_quad[3]) * inv_bh2; sqr_length += (*fill) * (*fill); fill++;
            *fill = (minor_quad[0] - minor_quad[1]) * inv_bh2; sqr_length += (*fill) * (*fill); fill++;
            *fill = (minor_quad[2] - minor_quad[3]) * inv_bh2; sqr_length += (*fill) * (*fill); fill++;
          }
      }
      float sqr_length_inv = 1.0f / std::sqrt(float(sqr_length));
      if (!std::isnormal(sqr_length_inv)) sqr_length_inv = 0.0f;
      for (; first != fill; first++) (*first) *= sqr_length_inv;
    }
    return;
  }
  std::vector<float> integral((size_t)(cw + 1) * (ch + 1));
  integral_of(Img{image.data(), cw, cw, ch}, integral.data());
  const View I{integral.data(), cw + 1, ch + 1, 1};
  static const double box[16][3] = {{-2, -2, 1}, {2, -2, 1}, {2, 2, 1}, {-2, 2, 1}, {-3.75, -3.75, 1.25}, {0, -3.75, 1.25},
                                    {3.75, -3.75, 1.25}, {3.75, 0, 1.25}, {3.75, 3.75, 1.25}, {0, 3.75, 1.25}, {-3.75, 3.75, 1.25},
                                    {-3.75, 0, 1.25}, {-6.4, 0, 1.6}, {0, -6.4, 1.6}, {6.4, 0, 1.6}, {0, 6.4, 1.6}};
  static const double q = 0.707106781186547;
  static const double hist[8][2] = {{0, 1}, {q, q}, {1, 0}, {q, -q}, {0, -1}, {-q, -q}, {-1, 0}, {-q, q}};
  static const double samp[9][2] = {{-1, -1}, {-1, 0}, {-1, 1}, {0, -1}, {0, 0}, {0, 1}, {1, -1}, {1, 0}, {1, 1}};
  for (int k = 0; k < n; ++k) {
    float ipx = xs[k], ipy = ys[k];
    ipx -= cx; ipy -= cy;
    float* d = desc + (size_t)k * 128;
    for (int i = 0; i < 128; ++i) d[i] = 0;
    unsigned write_idx = 0;
    const float scale = scales[k];
    const float co = cos((double)oris[k]);
    const float si = sin((double)oris[k]);
    const double rot[2][2] = {{co, -si}, {si, co}};
    for (int ce = 0; ce < 16; ++ce) {
      double responses[18][2];
      unsigned s_write_idx = 0;
      for (int of = 0; of < 9; ++of) {
        const double vx = box[ce][2] * samp[of][0] + box[ce][0], vy = box[ce][2] * samp[of][1] + box[ce][1];
        const double sr[2][2] = {{scale * rot[0][0], scale * rot[0][1]}, {scale * rot[1][0], scale * rot[1][1]}};
        const double loc[2] = {sr[0][0] * vx + sr[0][1] * vy, sr[1][0] * vx + sr[1][1] * vy};
        const float size = 2 * scale * box[ce][2];
        const double hh = hhaar(I, loc[0] + ipx, loc[1] + ipy, size);
        responses[s_write_idx][0] = rot[0][0] * hh + rot[0][1] * 0.0;
        responses[s_write_idx][1] = rot[1][0] * hh + rot[1][1] * 0.0;
        s_write_idx++;
        const double vv = vhaar(I, loc[0] + ipx, loc[1] + ipy, size);
        responses[s_write_idx][0] = rot[0][0] * 0.0 + rot[0][1] * vv;
        responses[s_write_idx][1] = rot[1][0] * 0.0 + rot[1][1] * vv;
        s_write_idx++;
      }
      for (int b = 0; b < 8; ++b) {
        for (int i = 0; i < 18; ++i) {
          const double dot = hist[b][0] * responses[i][0] + hist[b][1] * responses[i][1];
          if (dot > 0) d[write_idx] += dot;
        }
        write_idx++;
      }
    }
    auto norm_2 = [&]() {
      double result = 0.0;
      for (int i = 0; i < 128; ++i) result += d[i] * d[i];
      return std::sqrt((double)static_cast<float>(result));
    };
    float distance = norm_2();
    for (int i = 0; i < 128; ++i) d[i] /= distance;
    for (int i = 0; i < 128; ++i)
      if (d[i] > 0.2) d[i] = 0.2;
    distance = norm_2();
    for (int i = 0; i < 128; ++i) d[i] /= distance;
  }
}

}  // extern "C"
