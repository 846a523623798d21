// triangulate_view.cc — the C++ surface of triangulation (vwlite vw::stereo::stereo_triangulate, StereoModel,
// UniverseRadiusFunc with the cameras of vw/Camera.h), as a reference user would call it.
//   triangulate_view view     pinhole|cahv|tsai d.bin w h xyz.bin           ImageView<Vector3> pc = stereo_triangulate(d, &c1, &c2)
//   triangulate_view boxes    pinhole|cahv|tsai d.bin w h xyz.bin           the same view rasterised box by box into crops
//   triangulate_view model    pinhole|cahv|tsai d.bin w h xyz.bin err.bin   StereoModel(&c1, &c2)(d, error)
//   triangulate_view universe p.bin w h ox oy oz near far out.bin           UniverseRadiusFunc on Vector3 points; prints the counters
// d.bin holds w x h float {dx, dy, valid} pixels, the other files raw doubles.  The cameras are the pairs of
// tests/refimpl/triangulate_ref.py: baseline 1 along x, 2.5 degrees of toe-in; pinhole: f = 500, principal point at the
// image centre; cahv: the same pair as CAHV models; tsai: f = 512, principal point (32, 22), the two Tsai lenses.
// Exit status: 0 done, 1 any error.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <vw/Camera.h>
#include <vw/Stereo.h>

namespace {
using namespace vw;
typedef PixelMask<Vector2f> PixelF;

template <class T>
bool read_raw(const char* path, T* data, size_t n) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  const size_t got = std::fread(data, sizeof(T), n, f);
  std::fclose(f);
  return got == n;
}
template <class T>
bool write_raw(const char* path, const T* data, size_t n) {
  std::FILE* f = std::fopen(path, "wb");
  if (!f) return false;
  const size_t put = std::fwrite(data, sizeof(T), n, f);
  return std::fclose(f) == 0 && put == n;
}

Matrix3x3 rot_y(double deg) {
  const double a = deg * (M_PI / 180.0);
  Matrix3x3 r;
  r(0, 0) = std::cos(a); r(0, 2) = std::sin(a); r(1, 1) = 1; r(2, 0) = -std::sin(a); r(2, 2) = std::cos(a);
  return r;
}
Vector3 column(Matrix3x3 const& r, int c, double s = 1.0) { return Vector3(s * r(0, c), s * r(1, c), s * r(2, c)); }
Vector3 axpy(double f, Vector3 const& x, double c, Vector3 const& a) { return Vector3(f * x[0] + c * a[0], f * x[1] + c * a[1], f * x[2] + c * a[2]); }

struct Pair {
  std::shared_ptr<camera::CameraModel> c1, c2;
};
Pair make_pair(std::string const& kind, int w, int h) {
  Pair p;
  const Matrix3x3 r1 = rot_y(2.5), r2 = rot_y(-2.5);
  const Vector3 o1(0, 0, 0), o2(1, 0, 0);
  if (kind == "tsai") {
    const camera::TsaiLensDistortion wild(-256.0 / 3.0, 0.0, 0.0, 0.0, 0.0), mild(-0.28, 0.09, 1.1e-3, -6e-4, 0.013);
    p.c1.reset(new camera::PinholeModel(o1, r1, 512.0, 512.0, 32.0, 22.0, &wild));
    p.c2.reset(new camera::PinholeModel(o2, r2, 512.0, 512.0, 32.0, 22.0, &mild));
    return p;
  }
  const double f = 500.0, cu = w / 2.0, cv = h / 2.0;
  if (kind == "cahv") {
    p.c1.reset(new camera::CAHVModel(o1, column(r1, 2), axpy(f, column(r1, 0), cu, column(r1, 2)), axpy(f, column(r1, 1), cv, column(r1, 2))));
    p.c2.reset(new camera::CAHVModel(o2, column(r2, 2), axpy(f, column(r2, 0), cu, column(r2, 2)), axpy(f, column(r2, 1), cv, column(r2, 2))));
    return p;
  }
  p.c1.reset(new camera::PinholeModel(o1, r1, f, f, cu, cv));
  p.c2.reset(new camera::PinholeModel(o2, r2, f, f, cu, cv));
  return p;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s view|boxes|model|universe ...\n", argv[0]);
    return 2;
  }
  const std::string mode = argv[1];
  try {
    if (mode == "universe" && argc == 11) {
      const int w = std::atoi(argv[3]), h = std::atoi(argv[4]);
      ImageView<Vector3> pts(w, h);
      if (!read_raw(argv[2], reinterpret_cast<double*>(pts.data()), (size_t)w * h * 3)) return 1;
      stereo::UniverseRadiusFunc func(Vector3(std::atof(argv[5]), std::atof(argv[6]), std::atof(argv[7])), std::atof(argv[8]), std::atof(argv[9]));
      ImageView<Vector3> out = func(pts);
      if (!write_raw(argv[10], reinterpret_cast<const double*>(out.data()), (size_t)w * h * 3)) return 1;
      std::printf("rejected %lld of %lld\n", (long long)func.rejected_points(), (long long)func.total_points());
    } else if ((mode == "view" || mode == "boxes") && argc == 7) {
      const int w = std::atoi(argv[4]), h = std::atoi(argv[5]);
      ImageView<PixelF> d(w, h);
      if (!read_raw(argv[3], reinterpret_cast<float*>(d.data()), (size_t)w * h * 3)) return 1;
      const Pair p = make_pair(argv[2], w, h);
      ImageView<Vector3> pc(w, h);
      if (mode == "view") {
        pc = stereo::stereo_triangulate(d, p.c1.get(), p.c2.get());
      } else {
        // an uneven tiling, box by box, as a block rasteriser would ask for it
        stereo::StereoView<ImageView<PixelF>> view = stereo::stereo_triangulate(d, p.c1.get(), p.c2.get());
        for (int y = 0; y < h; y += 17)
          for (int x = 0; x < w; x += 29) {
            const BBox2i box(x, y, std::min(29, w - x), std::min(17, h - y));
            view.rasterize(crop(pc, box), box);
          }
      }
      if (!write_raw(argv[6], reinterpret_cast<const double*>(pc.data()), (size_t)w * h * 3)) return 1;
    } else if (mode == "model" && argc == 8) {
      const int w = std::atoi(argv[4]), h = std::atoi(argv[5]);
      ImageView<PixelF> d(w, h);
      if (!read_raw(argv[3], reinterpret_cast<float*>(d.data()), (size_t)w * h * 3)) return 1;
      const Pair p = make_pair(argv[2], w, h);
      stereo::StereoModel model(p.c1.get(), p.c2.get());
      ImageView<double> error;
      ImageView<Vector3> pc = model(d, error);
      if (!write_raw(argv[6], reinterpret_cast<const double*>(pc.data()), (size_t)w * h * 3)) return 1;
      if (!write_raw(argv[7], error.data(), (size_t)w * h)) return 1;
    } else {
      std::fprintf(stderr, "triangulate_view: bad arguments\n");
      return 2;
    }
  } catch (std::exception const& e) {
    std::fprintf(stderr, "triangulate_view: %s\n", e.what());
    return 1;
  }
  std::printf("triangulate_view ok\n");
  return 0;
}
