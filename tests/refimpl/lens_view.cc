// lens_view.cc — the C++ surface of the lens distortion classes (vwlite camera::LensDistortion and its subclasses, and
// PinholeModel around them), as a reference user would call it.
//   lens_view NAME c0 c1 c2 r0 .. r8 fu fv cu cv pitch p0 p1 ...
//       NAME: TSAI, FOV, FISHEYE, BrownConrady, AdjustableTSAI or Photometrix; the camera centre, the row-major rotation,
//       the intrinsics and the pixel pitch; then the parameters of the lens.
// Prints the name of the lens and, for each of three pixels, nine doubles as hexadecimal words: undistorted_coordinates and
// distorted_coordinates of pixel * pitch, pixel_to_vector, and point_to_pixel of the point 4 along that ray.
// Exit status: 0 done, 1 any error.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <vw/Camera.h>

int main(int argc, char** argv) {
  using namespace vw;
  using namespace vw::camera;
  if (argc < 20) return 1;
  try {
    const std::string name = argv[1];
    double g[17];
    for (int i = 0; i < 17; ++i) g[i] = std::atof(argv[2 + i]);
    std::vector<double> p;
    for (int i = 19; i < argc; ++i) p.push_back(std::atof(argv[i]));
    std::unique_ptr<LensDistortion> lens;
    if (name == "TSAI") lens.reset(new TsaiLensDistortion(p.at(0), p.at(1), p.at(2), p.at(3), p.at(4)));
    else if (name == "FOV") lens.reset(new FovLensDistortion(p));
    else if (name == "FISHEYE") lens.reset(new FisheyeLensDistortion(p));
    else if (name == "BrownConrady") lens.reset(new BrownConradyDistortion(Vector2(p.at(0), p.at(1)), Vector3(p.at(2), p.at(3), p.at(4)), Vector2(p.at(5), p.at(6)), p.at(7)));
    else if (name == "AdjustableTSAI") lens.reset(new AdjustableTsaiLensDistortion(p));
    else if (name == "Photometrix") lens.reset(new PhotometrixLensDistortion(p));
    else return 1;
    Matrix3x3 rot;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) rot(i, j) = g[3 + 3 * i + j];
    const TsaiLensDistortion* as_tsai = dynamic_cast<const TsaiLensDistortion*>(lens.get());
    // a TsaiLensDistortion const* call site, as before the hierarchy, and the general one
    const PinholeModel cam = as_tsai ? PinholeModel(Vector3(g[0], g[1], g[2]), rot, g[12], g[13], g[14], g[15], as_tsai, g[16])
                                     : PinholeModel(Vector3(g[0], g[1], g[2]), rot, g[12], g[13], g[14], g[15], lens.get(), g[16]);
    std::printf("%s\n", cam.lens_distortion()->name().c_str());
    const double pix[3][2] = {{3.0, 5.0}, {32.0, 22.0}, {60.25, 40.5}};
    for (int k = 0; k < 3; ++k) {
      const Vector2 px(pix[k][0], pix[k][1]), fp(px[0] * cam.pixel_pitch(), px[1] * cam.pixel_pitch());
      const Vector2 u = cam.lens_distortion()->undistorted_coordinates(cam, fp), d = cam.lens_distortion()->distorted_coordinates(cam, fp);
      const Vector3 ray = cam.pixel_to_vector(px);
      const Vector2 back = cam.point_to_pixel(cam.camera_center() + 4.0 * ray);
      const double row[9] = {u[0], u[1], d[0], d[1], ray[0], ray[1], ray[2], back[0], back[1]};
      for (int i = 0; i < 9; ++i) {
        unsigned long long w;
        std::memcpy(&w, &row[i], 8);
        std::printf("%016llx ", w);
      }
      std::printf("\n");
    }
  } catch (std::exception const& e) {
    std::fprintf(stderr, "lens_view: %s\n", e.what());
    return 1;
  }
  return 0;
}
