// CPU restatement of vw::transform for the closed-form 2-D maps (test infrastructure only): the map functors of
// src/vw/Math/Transform.h:231-443, the edge extensions of src/vw/Image/EdgeExtension.tcc:47-272, the interpolations of
// src/vw/Image/Interpolation.h:75-225 over PixelMask<float> (src/vw/Image/PixelMask.h:321-345, :424-433), TransformView
// and TransformViewNoData (src/vw/Image/Transform.h:362-365, :430-437).  Written from those definitions as objects that
// mirror the reference's layering (a masked pixel type, an edge-extended view, an interpolator over it, a functor
// chain), not from the library's kernels.  Build: make -f transform_ref.mk (no FMA contraction, no fast-math).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

namespace {

// ---- the descriptor the tests hand to both sides (the layout of vwgpu_transform) ------------------------------------
struct Desc {
  int kind, inverted;
  double fwd[9], rev[9];
};
enum { K_IDENTITY, K_TRANSLATE, K_RESAMPLE, K_AFFINE, K_HOMOGRAPHY };
enum { NEAREST, BILINEAR, BICUBIC };
enum { E_ZERO, E_VALUE, E_CONSTANT, E_PERIODIC, E_CYLINDRICAL, E_REFLECT, E_LINEAR };
enum { C_INTEGER = 1, C_ALL_INSIDE = 2, C_SOME_OUTSIDE = 4, C_NAN_HUGE = 8, C_NODATA = 16, C_OTHER_TAP = 32 };

struct Vec2 { double x, y; };

// ---- Math/Transform.h --------------------------------------------------------------------------------------------------
struct Functor {
  virtual ~Functor() {}
  virtual Vec2 forward(Vec2 p) const = 0;
  virtual Vec2 reverse(Vec2 p) const = 0;
};
struct Identity : Functor {
  Vec2 forward(Vec2 p) const override { return p; }
  Vec2 reverse(Vec2 p) const override { return p; }
};
struct Translate : Functor {
  double tx, ty;
  Translate(double x, double y) : tx(x), ty(y) {}
  Vec2 forward(Vec2 p) const override { return Vec2{p.x + tx, p.y + ty}; }
  Vec2 reverse(Vec2 p) const override { return Vec2{p.x - tx, p.y - ty}; }
};
struct Resample : Functor {
  double fx, fy;
  Resample(double x, double y) : fx(x), fy(y) {}
  Vec2 forward(Vec2 p) const override { return Vec2{p.x * fx, p.y * fy}; }
  Vec2 reverse(Vec2 p) const override { return Vec2{p.x / fx, p.y / fy}; }
};
struct Affine : Functor {
  double a, b, c, d, ai, bi, ci, di, x, y;
  Vec2 forward(Vec2 p) const override { return Vec2{a * p.x + b * p.y + x, c * p.x + d * p.y + y}; }
  Vec2 reverse(Vec2 p) const override {
    double px = p.x - x;
    double py = p.y - y;
    return Vec2{ai * px + bi * py, ci * px + di * py};
  }
};
struct Homography : Functor {
  double H[9], Hi[9];
  static Vec2 apply(const double* m, Vec2 p) {
    double w = m[6] * p.x + m[7] * p.y + m[8];
    return Vec2{(m[0] * p.x + m[1] * p.y + m[2]) / w, (m[3] * p.x + m[4] * p.y + m[5]) / w};
  }
  Vec2 forward(Vec2 p) const override { return apply(H, p); }
  Vec2 reverse(Vec2 p) const override { return apply(Hi, p); }
};
struct Inverse : Functor {
  std::shared_ptr<Functor> tx;
  explicit Inverse(std::shared_ptr<Functor> t) : tx(t) {}
  Vec2 forward(Vec2 p) const override { return tx->reverse(p); }
  Vec2 reverse(Vec2 p) const override { return tx->forward(p); }
};
struct Composition : Functor {
  std::shared_ptr<Functor> tx1, tx2;
  Composition(std::shared_ptr<Functor> a, std::shared_ptr<Functor> b) : tx1(a), tx2(b) {}
  Vec2 forward(Vec2 p) const override { return tx1->forward(tx2->forward(p)); }
  Vec2 reverse(Vec2 p) const override { return tx2->reverse(tx1->reverse(p)); }
};

std::shared_ptr<Functor> functor_of(const Desc& d) {
  std::shared_ptr<Functor> f;
  switch (d.kind) {
    case K_IDENTITY: f = std::make_shared<Identity>(); break;
    case K_TRANSLATE: f = std::make_shared<Translate>(d.fwd[0], d.fwd[1]); break;
    case K_RESAMPLE: f = std::make_shared<Resample>(d.fwd[0], d.fwd[1]); break;
    case K_AFFINE: {
      auto a = std::make_shared<Affine>();
      a->a = d.fwd[0]; a->b = d.fwd[1]; a->c = d.fwd[2]; a->d = d.fwd[3];
      a->ai = d.rev[0]; a->bi = d.rev[1]; a->ci = d.rev[2]; a->di = d.rev[3];
      a->x = d.fwd[4]; a->y = d.fwd[5];
      f = a;
      break;
    }
    case K_HOMOGRAPHY: {
      auto h = std::make_shared<Homography>();
      std::memcpy(h->H, d.fwd, sizeof(h->H));
      std::memcpy(h->Hi, d.rev, sizeof(h->Hi));
      f = h;
      break;
    }
    default: return nullptr;
  }
  if (d.inverted) f = std::make_shared<Inverse>(f);
  return f;
}
// compose(steps[0], compose(steps[1], ...))
std::shared_ptr<Functor> chain_of(const Desc* steps, int n) {
  if (!steps || n < 1 || n > 4) return nullptr;
  std::shared_ptr<Functor> f = functor_of(steps[n - 1]);
  if (!f) return nullptr;
  for (int k = n - 2; k >= 0; --k) {
    std::shared_ptr<Functor> g = functor_of(steps[k]);
    if (!g) return nullptr;
    f = std::make_shared<Composition>(g, f);
  }
  return f;
}

bool all_finite(const double* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}
bool make_affine(const double m[4], double x, double y, Desc* out) {
  // the plain adjugate of a 2 x 2 matrix over its determinant
  double det = m[0] * m[3] - m[1] * m[2];
  if (det == 0 || !std::isfinite(det)) return false;
  Desc d;
  std::memset(&d, 0, sizeof(d));
  d.kind = K_AFFINE;
  for (int i = 0; i < 4; ++i) d.fwd[i] = m[i];
  d.rev[0] = m[3] / det;
  d.rev[1] = -m[1] / det;
  d.rev[2] = -m[2] / det;
  d.rev[3] = m[0] / det;
  d.fwd[4] = d.rev[4] = x;
  d.fwd[5] = d.rev[5] = y;
  *out = d;
  return true;
}

// ---- PixelMask<float> and the views ------------------------------------------------------------------------------------
template <class T>
struct Masked {
  T v;
  bool ok;
};
typedef Masked<float> MPix;
// the arithmetic of PixelMask: the child's arithmetic, valid only if both operands are
template <class T> Masked<T> operator+(Masked<T> a, Masked<T> b) { return Masked<T>{a.v + b.v, a.ok && b.ok}; }
template <class T> Masked<T> operator-(Masked<T> a, Masked<T> b) { return Masked<T>{a.v - b.v, a.ok && b.ok}; }
Masked<float> operator*(Masked<float> a, float s) { return Masked<float>{a.v * s, a.ok}; }
Masked<double> operator*(double s, Masked<float> a) { return Masked<double>{s * a.v, a.ok}; }
Masked<double> operator*(double s, Masked<double> a) { return Masked<double>{s * a.v, a.ok}; }

struct Image {
  const float* px;
  const uint8_t* mask;   // may be null: all valid
  int cols, rows;
  MPix operator()(int i, int j) const { return MPix{px[(size_t)j * cols + i], !mask || mask[(size_t)j * cols + i] != 0}; }
};

struct EdgeView {
  Image im;
  int kind;
  MPix value;   // ValueEdgeExtension's pixel
  mutable bool left;   // bookkeeping for the tests: a pixel outside the image was asked for
  bool inside(int i, int j) const { return i >= 0 && j >= 0 && i < im.cols && j < im.rows; }
  MPix operator()(int i, int j) const {
    if (!inside(i, j)) left = true;
    switch (kind) {
      case E_ZERO: return inside(i, j) ? im(i, j) : MPix{0.0f, false};
      case E_VALUE: return inside(i, j) ? im(i, j) : value;
      case E_CONSTANT:
        return im((i < 0) ? 0 : (i >= im.cols) ? (im.cols - 1) : i, (j < 0) ? 0 : (j >= im.rows) ? (im.rows - 1) : j);
      case E_PERIODIC: {
        int32_t d_i = i, d_j = j;
        d_i %= im.cols;
        if (d_i < 0) d_i += im.cols;
        d_j %= im.rows;
        if (d_j < 0) d_j += im.rows;
        return im(d_i, d_j);
      }
      case E_CYLINDRICAL: {
        int32_t d_i = i;
        d_i %= im.cols;
        if (d_i < 0) d_i += im.cols;
        int32_t d_j = (j < 0) ? 0 : (j >= im.rows) ? (im.rows - 1) : j;
        return im(d_i, d_j);
      }
      case E_REFLECT: {
        int32_t d_i = i, d_j = j;
        if (d_i < 0) d_i = -d_i;
        int32_t vcm1 = im.cols - 1;
        d_i %= 2 * vcm1;
        if (d_i > vcm1) d_i = 2 * vcm1 - d_i;
        if (d_j < 0) d_j = -d_j;
        int32_t vrm1 = im.rows - 1;
        d_j %= 2 * vrm1;
        if (d_j > vrm1) d_j = 2 * vrm1 - d_j;
        return im(d_i, d_j);
      }
      default: return linear(i, j);
    }
  }
  // LinearEdgeExtension on the float channel (masked images are not extended linearly here)
  MPix linear(int32_t i, int32_t j) const {
    auto view = [this](int x, int y) { return im(x, y).v; };
    int32_t vcm1 = im.cols - 1;
    int32_t vrm1 = im.rows - 1;
    float r;
    if (i < 0) {
      if (j < 0) r = view(0, 0) - i * (view(0, 0) - view(1, 0)) - j * (view(0, 0) - view(0, 1));
      else if (j > vrm1) r = view(0, vrm1) - i * (view(0, vrm1) - view(1, vrm1)) + (j - vrm1) * (view(0, vrm1) - view(0, vrm1 - 1));
      else r = view(0, j) - i * (view(0, j) - view(1, j));
    } else if (i > vcm1) {
      if (j < 0) r = view(vcm1, 0) + (i - vcm1) * (view(vcm1, 0) - view(vcm1 - 1, 0)) - j * (view(vcm1, 0) - view(vcm1, 1));
      else if (j > vrm1)
        r = view(vcm1, vrm1) + (i - vcm1) * (view(vcm1, vrm1) - view(vcm1 - 1, vrm1)) + (j - vrm1) * (view(vcm1, vrm1) - view(vcm1, vrm1 - 1));
      else r = view(vcm1, j) + (i - vcm1) * (view(vcm1, j) - view(vcm1 - 1, j));
    } else {
      if (j < 0) r = view(i, 0) - j * (view(i, 0) - view(i, 1));
      else if (j > vrm1) r = view(i, vrm1) + (j - vrm1) * (view(i, vrm1) - view(i, vrm1 - 1));
      else r = view(i, j);
    }
    return MPix{r, true};
  }
};

int32_t round_i(double val) { return val < 0 ? int32_t(val - 0.5) : int32_t(val + 0.5); }
int32_t floor_i(double val) { return int32_t(std::floor(val)); }

// the interpolation view; *integer tells whether the integer-position shortcut was taken
MPix interpolate(const EdgeView& view, int interp, double i, double j, bool* integer) {
  *integer = false;
  if (interp == NEAREST) {
    int32_t x = round_i(i), y = round_i(j);
    return view(x, y);
  }
  int32_t x = floor_i(i), y = floor_i(j);
  if (x == i && y == j) {
    *integer = true;
    return view(x, y);
  }
  if (interp == BILINEAR) {
    float normx = float(i) - float(x), normy = float(j) - float(y), norm1mx = 1 - normx, norm1my = 1 - normy;
    MPix result = view(x, y) * norm1mx;
    result = result + view(x + 1, y) * normx;
    result = result * norm1my;
    MPix row = view(x, y + 1) * norm1mx;
    row = row + view(x + 1, y + 1) * normx;
    result = result + row * normy;
    return result;
  }
  double normx = i - x, normy = j - y;
  double s0 = ((2 - normx) * normx - 1) * normx;     double t0 = ((2 - normy) * normy - 1) * normy;
  double s1 = (3 * normx - 5) * normx * normx + 2;   double t1 = (3 * normy - 5) * normy * normy + 2;
  double s2 = ((4 - 3 * normx) * normx + 1) * normx; double t2 = ((4 - 3 * normy) * normy + 1) * normy;
  double s3 = (normx - 1) * normx * normx;           double t3 = (normy - 1) * normy * normy;
  const double t[4] = {t0, t1, t2, t3};
  Masked<double> result{0, true};
  for (int r = 0; r < 4; ++r) {
    Masked<double> row = s0 * view(x - 1, y - 1 + r);
    row = row + s1 * view(x, y - 1 + r);
    row = row + s2 * view(x + 1, y - 1 + r);
    row = row + s3 * view(x + 2, y - 1 + r);
    result = r == 0 ? t[0] * row : result + t[r] * row;
  }
  result.v *= 0.25;
  return MPix{float(result.v), result.ok};
}

}  // namespace

extern "C" {

int tfr_desc_size() { return (int)sizeof(Desc); }

int tfr_make(int kind, const double* params, int n, Desc* out) {
  if (!out || n < 0 || n > 9 || (n > 0 && !params) || !all_finite(params, n)) return -1;
  Desc d;
  std::memset(&d, 0, sizeof(d));
  d.kind = kind;
  if (kind == K_IDENTITY) {
    if (n != 0) return -1;
  } else if (kind == K_TRANSLATE || kind == K_RESAMPLE) {
    if (n != 2) return -1;
    if (kind == K_RESAMPLE && (params[0] == 0 || params[1] == 0)) return -1;
    for (int i = 0; i < 2; ++i) d.fwd[i] = d.rev[i] = params[i];
  } else if (kind == K_AFFINE) {
    if (n != 6 || !make_affine(params, params[4], params[5], &d)) return -1;
  } else if (kind == K_HOMOGRAPHY) {
    if (n != 9) return -1;
    const double *m = params;
    // the plain adjugate of a 3 x 3 matrix over its determinant, as HomographyTransform of the package spells it
    double adj[9] = {m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                     m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                     m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]};
    double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    if (det == 0 || !std::isfinite(det)) return -1;
    for (int i = 0; i < 9; ++i) {
      d.fwd[i] = m[i];
      d.rev[i] = adj[i] / det;
    }
  } else {
    return -1;
  }
  *out = d;
  return 0;
}

// RotateTransform (Math/Transform.h:351-362)
int tfr_rotate(double theta, double cx, double cy, Desc* out) {
  if (!out || !std::isfinite(theta) || !std::isfinite(cx) || !std::isfinite(cy)) return -1;
  double c = std::cos(theta), s = std::sin(theta);
  double rotate[4] = {c, -s, s, c};
  double rhs0 = cx - (rotate[0] * cx + rotate[1] * cy);
  double rhs1 = cy - (rotate[2] * cx + rotate[3] * cy);
  return make_affine(rotate, rhs0, rhs1, out) ? 0 : -1;
}

int tfr_invert(const Desc* in, Desc* out) {
  if (!in || !out || in->kind < 0 || in->kind > K_HOMOGRAPHY || (in->inverted != 0 && in->inverted != 1)) return -1;
  Desc d = *in;
  d.inverted = !in->inverted;
  *out = d;
  return 0;
}

int tfr_points(const Desc* steps, int n, int direction, const double* points, long long count, double* out) {
  if (count < 0 || (count > 0 && (!points || !out)) || (direction != 0 && direction != 1)) return -1;
  for (int k = 0; steps && k < n && k < 4; ++k)
    if (steps[k].inverted != 0 && steps[k].inverted != 1) return -1;
  std::shared_ptr<Functor> f = chain_of(steps, n);
  if (!f) return -1;
  for (long long i = 0; i < count; ++i) {
    Vec2 p{points[2 * i], points[2 * i + 1]};
    Vec2 q = direction == 0 ? f->forward(p) : f->reverse(p);
    out[2 * i] = q.x;
    out[2 * i + 1] = q.y;
  }
  return 0;
}

// transform(image, chain, w, h, edge, interp) / transform_nodata rasterised over the box (x0, y0, w, h).  mask may be null;
// omask and cls are always written.  cls: C_* bits per pixel.
int tfr_image(const float* src, int sw, int sh, const uint8_t* mask, const Desc* steps, int n, int interp, int edge, float edge_value,
              int edge_valid, int nodata, float nodata_value, int nodata_valid, int w, int h, int x0, int y0, float* out, uint8_t* omask,
              int32_t* cls) {
  std::shared_ptr<Functor> f = chain_of(steps, n);
  if (!f || !src || !out || !omask || !cls || sw <= 0 || sh <= 0 || w <= 0 || h <= 0) return -1;
  if (interp < NEAREST || interp > BICUBIC || edge < E_ZERO || edge > E_LINEAR) return -1;
  if (edge == E_REFLECT && (sw < 2 || sh < 2)) return -1;
  if (edge == E_LINEAR && (sw < 2 || sh < 2)) return -1;
  if (edge == E_LINEAR && mask) return -2;
  EdgeView view{Image{src, mask, sw, sh}, edge, MPix{edge_value, edge_valid != 0}, false};
  const int b = interp == BICUBIC ? 2 : 1;   // pixel_buffer
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      Vec2 rv = f->reverse(Vec2{double((long long)x0 + x), double((long long)y0 + y)});
      MPix r;
      int c = 0;
      if (nodata && (rv.x < b - 1 || rv.x >= sw - b || rv.y < b - 1 || rv.y >= sh - b)) {
        r = MPix{nodata_value, nodata_valid != 0};
        c = C_NODATA;
      } else if (!(rv.x >= -1073741824.0 && rv.x <= 1073741824.0 && rv.y >= -1073741824.0 && rv.y <= 1073741824.0)) {
        r = MPix{0.0f, false};   // the int32 conversion is undefined in the reference: 0 and invalid by the project's rule
        c = C_NAN_HUGE;
      } else {
        bool integer;
        view.left = false;
        r = interpolate(view, interp, rv.x, rv.y, &integer);
        c = (integer ? C_INTEGER : 0) | (view.left ? C_SOME_OUTSIDE : C_ALL_INSIDE);
        if (!r.ok && view(round_i(rv.x), round_i(rv.y)).ok) c |= C_OTHER_TAP;
      }
      out[(size_t)y * w + x] = r.v;
      omask[(size_t)y * w + x] = r.ok ? 255 : 0;
      cls[(size_t)y * w + x] = c;
    }
  return 0;
}

}  // extern "C"
