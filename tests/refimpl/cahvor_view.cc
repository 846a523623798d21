// cahvor_view.cc — the C++ surface of the CAHVOR and CAHVORE cameras (vwlite camera::CAHVORModel, CAHVOREModel,
// linearize_camera, linearize_camera_transform, camera_transform, CameraTransform and stereo::stereo_triangulate), as a
// reference user would call it.
//   cahvor_view cahvor|cahvore cams.bin image.bin mask.bin w h disp.bin dw dh prefix
//       cams.bin: two cameras of 23 doubles each {C, A, H, V, O, R, E, T, P} (E, T, P unused for cahvor); image.bin
//       w x h floats with mask.bin bytes (a PixelMask<float> image); disp.bin dw x dh x {dx, dy, valid} floats.
//       The first camera: linearize_camera at (w, h), linearize_camera_transform of the masked image with
//       ValueEdgeExtension(PixelMask<float>(0.5)), the float image re-distorted (camera_transform(lin -> camera), box by
//       box, zero edge), one point through CameraTransform forward and back, the model's own pixel_to_vector and
//       point_to_pixel of that point.  Both cameras: stereo_triangulate(disp).  Writes prefix.lin (the CAHV descriptor),
//       prefix.out (floats), prefix.omask (bytes), prefix.back (floats), prefix.xyz (doubles), prefix.meta (doubles: forward
//       x, y, reverse x, y, the ray, the pixel of C + 7 ray).
// Exit status: 0 done, 1 any error.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <vw/Camera.h>
#include <vw/CameraTransform.h>
#include <vw/Stereo.h>

namespace {
using namespace vw;
typedef PixelMask<Vector2f> PixelF;

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
Vector3 vec(const double* p) { return Vector3(p[0], p[1], p[2]); }
camera::CAHVORModel cahvor(const double* p) { return camera::CAHVORModel(vec(p), vec(p + 3), vec(p + 6), vec(p + 9), vec(p + 12), vec(p + 15)); }
camera::CAHVOREModel cahvore(const double* p) {
  return camera::CAHVOREModel(vec(p), vec(p + 3), vec(p + 6), vec(p + 9), vec(p + 12), vec(p + 15), vec(p + 18), (int)p[21], p[22]);
}

template <class CameraT>
int run(CameraT const& cam1, CameraT const& cam2, char** argv) {
  const int w = std::atoi(argv[5]), h = std::atoi(argv[6]), dw = std::atoi(argv[8]), dh = std::atoi(argv[9]);
  const std::string prefix = argv[10];
  std::vector<uint8> m((size_t)w * h);
  ImageView<float> plain(w, h);
  ImageView<PixelMask<float>> masked(w, h);
  ImageView<PixelF> d(dw, dh);
  if (!read_raw(argv[3], plain.data(), m.size()) || !read_raw(argv[4], m.data(), m.size()) ||
      !read_raw(argv[7], reinterpret_cast<float*>(d.data()), (size_t)dw * dh * 3))
    return 1;
  for (size_t i = 0; i < m.size(); ++i) {
    masked.data()[i] = PixelMask<float>(plain.data()[i]);
    if (!m[i]) masked.data()[i].invalidate();
  }
  const camera::CAHVModel lin = camera::linearize_camera(cam1, Vector2i(w, h), Vector2i(w, h));
  const camera::CAHVModel lin2 = camera::linearize_camera(cam1, w, h, w, h);
  if (std::memcmp(&lin.descriptor(), &lin2.descriptor(), sizeof(vwgpu_camera)) != 0) return 1;
  // the undistorted image: one masked view, rasterised whole
  camera::CameraTransformView<ImageView<PixelMask<float>>, CameraT, camera::CAHVModel> view =
      camera::linearize_camera_transform(masked, cam1, ValueEdgeExtension<PixelMask<float>>(PixelMask<float>(0.5f)), BilinearInterpolation());
  if (std::memcmp(&view.dst_camera().descriptor(), &lin.descriptor(), sizeof(vwgpu_camera)) != 0) return 1;
  ImageView<PixelMask<float>> out = view;
  std::vector<float> ov(m.size());
  std::vector<uint8> om(m.size());
  for (size_t i = 0; i < m.size(); ++i) {
    ov[i] = out.data()[i].child();
    om[i] = out.data()[i].valid() != 0 ? 255 : 0;
  }
  // and distorted again: an uneven tiling, box by box, as a block rasteriser would ask for it
  ImageView<float> back(w, h);
  camera::CameraTransformView<ImageView<float>, camera::CAHVModel, CameraT> redo = camera::camera_transform(plain, lin, cam1);
  for (int y = 0; y < h; y += 17)
    for (int x = 0; x < w; x += 29) {
      const BBox2i box(x, y, std::min(29, w - x), std::min(17, h - y));
      redo.rasterize(crop(back, box), box);
    }
  const camera::CameraTransform<CameraT, camera::CAHVModel> t(cam1, lin);
  const Vector2 p(w / 3.0, h / 4.0), fwd = t.forward(p), rev = t.reverse(fwd);
  const Vector3 ray = cam1.pixel_to_vector(p);
  const Vector2 pix = cam1.point_to_pixel(cam1.camera_center() + 7.0 * ray);
  const double meta[9] = {fwd[0], fwd[1], rev[0], rev[1], ray[0], ray[1], ray[2], pix[0], pix[1]};
  ImageView<Vector3> pc = stereo::stereo_triangulate(d, &cam1, &cam2);
  const vwgpu_camera lin_desc = lin.descriptor();
  if (!write_raw(prefix + ".lin", &lin_desc, 1) || !write_raw(prefix + ".out", ov.data(), ov.size()) ||
      !write_raw(prefix + ".omask", om.data(), om.size()) || !write_raw(prefix + ".back", back.data(), m.size()) ||
      !write_raw(prefix + ".xyz", reinterpret_cast<const double*>(pc.data()), (size_t)dw * dh * 3) || !write_raw(prefix + ".meta", meta, 9))
    return 1;
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (argc != 11 || (mode != "cahvor" && mode != "cahvore")) {
    std::fprintf(stderr, "usage: %s cahvor|cahvore cams.bin image.bin mask.bin w h disp.bin dw dh prefix\n", argv[0]);
    return 2;
  }
  try {
    double p[46];
    if (!read_raw(argv[2], p, 46)) return 1;
    const int rc = mode == "cahvor" ? run(cahvor(p), cahvor(p + 23), argv) : run(cahvore(p), cahvore(p + 23), argv);
    if (rc) return rc;
  } catch (std::exception const& e) {
    std::fprintf(stderr, "cahvor_view: %s\n", e.what());
    return 1;
  }
  std::printf("cahvor_view ok\n");
  return 0;
}
