// epipolar_view.cc — the C++ surface of epipolar rectification (vwlite camera::epipolar, resize_epipolar_cameras_to_fit,
// camera_transform and CameraTransform of vw/Camera.h and vw/CameraTransform.h), as a reference user would call it.
//   epipolar_view pair cams.bin left.bin lmask.bin lw lh right.bin rw rh prefix
//       cams.bin: two pinholes of 23 doubles each {center[3], rotation[9], fu, fv, cu, cv, pitch, has_lens, tsai[5]};
//       left.bin lw x lh floats with lmask.bin bytes (a PixelMask<float> image), right.bin rw x rh floats.
//       epipolar(), resize_epipolar_cameras_to_fit over the whole frames, then camera_transform: the left image as one
//       view with ValueEdgeExtension(PixelMask<float>(7.5)), the right one box by box with ZeroEdgeExtension.  Writes
//       prefix.left (floats), prefix.lmask (bytes), prefix.right (floats), prefix.epi (the two rectified descriptors) and
//       prefix.meta (doubles: the two sizes, and one perimeter point through CameraTransform::forward and back).
//   epipolar_view cahv cams.bin prefix
//       cams.bin: two CAHV models of 12 doubles {C, A, H, V}; writes prefix.epi (the two rectified descriptors).
// Exit status: 0 done, 1 any error.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <vw/Camera.h>
#include <vw/CameraTransform.h>

namespace {
using namespace vw;

template <class T>
bool read_raw(std::string const& path, T* data, size_t n) {
  std::FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  const size_t got = std::fread(data, sizeof(T), n, f);
  std::fclose(f);
  return got == n;
}
template <class T>
bool write_raw(std::string const& path, const T* data, size_t n) {
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const size_t put = std::fwrite(data, sizeof(T), n, f);
  return std::fclose(f) == 0 && put == n;
}

camera::PinholeModel pinhole(const double* p) {
  Matrix3x3 r;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r(i, j) = p[3 + i * 3 + j];
  const camera::TsaiLensDistortion lens(p[18], p[19], p[20], p[21], p[22]);
  return camera::PinholeModel(Vector3(p[0], p[1], p[2]), r, p[12], p[13], p[14], p[15], p[17] != 0 ? &lens : NULL, p[16]);
}
camera::CAHVModel cahv(const double* p) {
  return camera::CAHVModel(Vector3(p[0], p[1], p[2]), Vector3(p[3], p[4], p[5]), Vector3(p[6], p[7], p[8]), Vector3(p[9], p[10], p[11]));
}
}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  try {
    if (mode == "cahv" && argc == 4) {
      double p[24];
      if (!read_raw(argv[2], p, 24)) return 1;
      camera::CAHVModel e0, e1;
      camera::epipolar(cahv(p), cahv(p + 12), e0, e1);
      const vwgpu_camera epi[2] = {e0.descriptor(), e1.descriptor()};
      if (!write_raw(std::string(argv[3]) + ".epi", epi, 2)) return 1;
    } else if (mode == "pair" && argc == 11) {
      double p[46];
      if (!read_raw(argv[2], p, 46)) return 1;
      const int lw = std::atoi(argv[5]), lh = std::atoi(argv[6]), rw = std::atoi(argv[8]), rh = std::atoi(argv[9]);
      const std::string prefix = argv[10];
      std::vector<float> lv((size_t)lw * lh);
      std::vector<uint8> lm(lv.size());
      ImageView<PixelMask<float>> left(lw, lh);
      ImageView<float> right(rw, rh);
      if (!read_raw(argv[3], lv.data(), lv.size()) || !read_raw(argv[4], lm.data(), lm.size()) ||
          !read_raw(argv[7], right.data(), (size_t)rw * rh))
        return 1;
      for (size_t i = 0; i < lv.size(); ++i) {
        left.data()[i] = PixelMask<float>(lv[i]);
        if (!lm[i]) left.data()[i].invalidate();
      }
      const camera::PinholeModel cam1 = pinhole(p), cam2 = pinhole(p + 23);
      camera::PinholeModel epi1, epi2;
      camera::epipolar(cam1, cam2, epi1, epi2);
      Vector2i size1, size2;
      camera::resize_epipolar_cameras_to_fit(cam1, cam2, epi1, epi2, BBox2i(0, 0, lw, lh), BBox2i(0, 0, rw, rh), size1, size2);
      // the left image: one masked view, rasterised whole
      ImageView<PixelMask<float>> lo = camera::camera_transform(left, cam1, epi1, size1, ValueEdgeExtension<PixelMask<float>>(PixelMask<float>(7.5f)),
                                                                BilinearInterpolation());
      std::vector<float> lov((size_t)size1[0] * size1[1]);
      std::vector<uint8> lom(lov.size());
      for (size_t i = 0; i < lov.size(); ++i) {
        lov[i] = lo.data()[i].child();
        lom[i] = lo.data()[i].valid() != 0 ? 255 : 0;
      }
      // the right image: an uneven tiling, box by box, as a block rasteriser would ask for it
      ImageView<float> ro(size2[0], size2[1]);
      camera::CameraTransformView<ImageView<float>, camera::PinholeModel, camera::PinholeModel> view =
          camera::camera_transform(right, cam2, epi2, size2);
      for (int y = 0; y < size2[1]; y += 17)
        for (int x = 0; x < size2[0]; x += 29) {
          const BBox2i box(x, y, std::min(29, size2[0] - x), std::min(17, size2[1] - y));
          view.rasterize(crop(ro, box), box);
        }
      const camera::CameraTransform<camera::PinholeModel, camera::PinholeModel> t(cam1, epi1);
      const Vector2 fwd = t.forward(Vector2(lw - 1, 3)), back = t.reverse(fwd);
      const double meta[8] = {(double)size1[0], (double)size1[1], (double)size2[0], (double)size2[1], fwd[0], fwd[1], back[0], back[1]};
      const vwgpu_camera epi[2] = {epi1.descriptor(), epi2.descriptor()};
      if (!write_raw(prefix + ".left", lov.data(), lov.size()) || !write_raw(prefix + ".lmask", lom.data(), lom.size()) ||
          !write_raw(prefix + ".right", ro.data(), (size_t)size2[0] * size2[1]) || !write_raw(prefix + ".epi", epi, 2) ||
          !write_raw(prefix + ".meta", meta, 8))
        return 1;
    } else {
      std::fprintf(stderr, "usage: %s pair|cahv ...\n", argv[0]);
      return 2;
    }
  } catch (std::exception const& e) {
    std::fprintf(stderr, "epipolar_view: %s\n", e.what());
    return 1;
  }
  std::printf("epipolar_view ok\n");
  return 0;
}
