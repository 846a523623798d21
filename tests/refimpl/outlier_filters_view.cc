// outlier_filters_view.cc — the C++ surface of the local outlier filters (vwlite vw::stereo::rm_outliers_using_mean /
// _stddev / _plane, disparity_cleanup_using_mean / _stddev, disparity_clean_using_plane, std_dev_image), as a reference
// user would call them.
//   outlier_filters_view mean|stddev|plane in.pfm out.pfm half_h half_v p0 p1 cleanup int reference_loop
//   outlier_filters_view stddev_image image.pfm out.pfm kernel_width kernel_height zero_edge
// Disparities are {dx, dy, valid} 3-channel PFMs (int = 1: converted to PixelMask<Vector2i> and back), images 1-channel
// PFMs.  Exit status: 0 written, 3 NoImplErr, 1 any other error.
#include <cstdio>
#include <cstdlib>
#include <string>

#include <vw/FileIO.h>
#include <vw/Stereo.h>

namespace {
template <class PixelT>
vw::ImageView<PixelT> filter(vw::ImageView<PixelT> const& in, std::string const& mode, int hh, int hv, double p0, double p1,
                             bool cleanup, bool reference_loop) {
  using namespace vw::stereo;
  if (mode == "mean")
    return cleanup ? disparity_cleanup_using_mean(in, hh, hv, p0, reference_loop) : rm_outliers_using_mean(in, hh, hv, p0, reference_loop);
  if (mode == "stddev") return cleanup ? disparity_cleanup_using_stddev(in, hh, hv, p0, p1) : rm_outliers_using_stddev(in, hh, hv, p0, p1);
  return cleanup ? disparity_clean_using_plane(in, hh, hv, p0, p1) : rm_outliers_using_plane(in, hh, hv, p0, p1);
}
}  // namespace

int main(int argc, char** argv) {
  using namespace vw;
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s mean|stddev|plane|stddev_image in out ...\n", argv[0]);
    return 2;
  }
  const std::string mode = argv[1];
  try {
    if (mode == "stddev_image" && argc == 7) {
      ImageView<float> image = DiskImageView<float>(argv[2]);
      ImageView<float> out = std::atoi(argv[6]) ? stereo::std_dev_image(image, std::atoi(argv[4]), std::atoi(argv[5]))
                                                : stereo::std_dev_image(image, std::atoi(argv[4]), std::atoi(argv[5]), ConstantEdgeExtension());
      write_image(argv[3], out);
    } else if ((mode == "mean" || mode == "stddev" || mode == "plane") && argc == 11) {
      ImageView<PixelMask<Vector2f>> f = DiskImageView<PixelMask<Vector2f>>(argv[2]);
      const int hh = std::atoi(argv[4]), hv = std::atoi(argv[5]);
      const double p0 = std::atof(argv[6]), p1 = std::atof(argv[7]);
      const bool cleanup = std::atoi(argv[8]) != 0, reference_loop = std::atoi(argv[10]) != 0;
      if (std::atoi(argv[9])) {
        ImageView<PixelMask<Vector2i>> in(f.cols(), f.rows());
        for (int32 y = 0; y < f.rows(); ++y)
          for (int32 x = 0; x < f.cols(); ++x) {
            in(x, y) = PixelMask<Vector2i>(Vector2i((int32)f(x, y).child()[0], (int32)f(x, y).child()[1]));
            if (!is_valid(f(x, y))) in(x, y).invalidate();
          }
        ImageView<PixelMask<Vector2i>> out = filter(in, mode, hh, hv, p0, p1, cleanup, reference_loop);
        for (int32 y = 0; y < f.rows(); ++y)
          for (int32 x = 0; x < f.cols(); ++x) {
            f(x, y) = PixelMask<Vector2f>(Vector2f((float)out(x, y).child()[0], (float)out(x, y).child()[1]));
            if (!is_valid(out(x, y))) f(x, y).invalidate();
          }
        write_image(argv[3], f);
      } else {
        write_image(argv[3], filter(f, mode, hh, hv, p0, p1, cleanup, reference_loop));
      }
    } else {
      std::fprintf(stderr, "outlier_filters_view: bad arguments\n");
      return 2;
    }
  } catch (NoImplErr const& e) {
    std::fprintf(stderr, "outlier_filters_view: NoImplErr: %s\n", e.what());
    return 3;
  } catch (std::exception const& e) {
    std::fprintf(stderr, "outlier_filters_view: %s\n", e.what());
    return 1;
  }
  std::printf("outlier_filters_view ok\n");
  return 0;
}
