// disparity_filters_view.cc — the C++ surface of the disparity post-filters (vwlite vw::stereo::disparity_median_filter,
// disparity_neighbor_filter, texture_measure, texture_preserving_disparity_filter), as a reference user would call them.
//   disparity_filters_view median   in.pfm out.pfm kernel_size snapshot
//   disparity_filters_view neighbor in.pfm out.pfm snapshot               (integer disparities stored as floats)
//   disparity_filters_view smooth   in.pfm out.pfm texture.pfm texture_max max_kernel_size snapshot
//   disparity_filters_view texture  image.pfm out.pfm kernel_size gradient_weight stddev_weight
// Disparities are {dx, dy, valid} 3-channel PFMs, images 1-channel PFMs.  In reference semantics (snapshot = 0)
// disparity_out must share disparity_in's buffer afterwards, in snapshot semantics it must not: exit status 4 otherwise.
// Exit status: 0 written, 3 NoImplErr, 1 any other error.
#include <cstdio>
#include <cstdlib>
#include <string>

#include <vw/FileIO.h>
#include <vw/Stereo.h>

int main(int argc, char** argv) {
  using namespace vw;
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s median|neighbor|smooth|texture in out ...\n", argv[0]);
    return 2;
  }
  const std::string mode = argv[1];
  try {
    if (mode == "texture" && argc == 7) {
      ImageView<float> image = DiskImageView<float>(argv[2]), out;
      stereo::texture_measure(image, out, std::atoi(argv[4]), std::atof(argv[5]), std::atof(argv[6]));
      write_image(argv[3], out);
    } else if (mode == "neighbor" && argc == 5) {
      ImageView<PixelMask<Vector2f>> f = DiskImageView<PixelMask<Vector2f>>(argv[2]);
      ImageView<PixelMask<Vector2i>> in(f.cols(), f.rows()), out;
      for (int32 y = 0; y < f.rows(); ++y)
        for (int32 x = 0; x < f.cols(); ++x) {
          in(x, y) = PixelMask<Vector2i>(Vector2i((int32)f(x, y).child()[0], (int32)f(x, y).child()[1]));
          if (!is_valid(f(x, y))) in(x, y).invalidate();
        }
      const bool snapshot = std::atoi(argv[4]) != 0;
      stereo::disparity_neighbor_filter(in, out, snapshot);
      if ((out.data() == in.data()) == snapshot) return 4;
      for (int32 y = 0; y < f.rows(); ++y)
        for (int32 x = 0; x < f.cols(); ++x) {
          f(x, y) = PixelMask<Vector2f>(Vector2f((float)out(x, y).child()[0], (float)out(x, y).child()[1]));
          if (!is_valid(out(x, y))) f(x, y).invalidate();
        }
      write_image(argv[3], f);
    } else if ((mode == "median" && argc == 6) || (mode == "smooth" && argc == 8)) {
      ImageView<PixelMask<Vector2f>> in = DiskImageView<PixelMask<Vector2f>>(argv[2]), out;
      const bool snapshot = std::atoi(argv[argc - 1]) != 0;
      if (mode == "median") {
        stereo::disparity_median_filter(in, out, std::atoi(argv[4]), snapshot);
      } else {
        ImageView<float> texture = DiskImageView<float>(argv[4]);
        stereo::texture_preserving_disparity_filter(in, out, texture, (float)std::atof(argv[5]), std::atoi(argv[6]), snapshot);
      }
      if ((out.data() == in.data()) == snapshot) return 4;
      write_image(argv[3], out);
    } else {
      std::fprintf(stderr, "disparity_filters_view: bad arguments\n");
      return 2;
    }
  } catch (NoImplErr const& e) {
    std::fprintf(stderr, "disparity_filters_view: NoImplErr: %s\n", e.what());
    return 3;
  } catch (std::exception const& e) {
    std::fprintf(stderr, "disparity_filters_view: %s\n", e.what());
    return 1;
  }
  std::printf("disparity_filters_view ok\n");
  return 0;
}
