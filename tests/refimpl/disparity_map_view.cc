// disparity_map_view.cc — the C++ surface of the operators of Stereo/DisparityMap.h on a finished disparity map (vwlite
// vw::stereo::get_disparity_range, disparity_range_mask, transform_disparities, disparity_subsample, disparity_upsample,
// missing_pixel_image, intersect_mask_and_data and transform(right, DisparityTransform(d))), as a reference user would
// call them.
//   disparity_map_view range      in.pfm int                         prints min.x min.y max.x max.y
//   disparity_map_view mask       in.pfm out.pfm int minx miny maxx maxy reference_bounds
//   disparity_map_view transform  in.pfm out.pfm int h00 .. h22     transform_disparities(d, HomographyTransform(H))
//   disparity_map_view subregion  in.pfm out.pfm int do_round x0 y0 t00 .. t22
//   disparity_map_view subsample|upsample in.pfm out.pfm int
//   disparity_map_view missing    in.pfm out.pfm int                 one float per pixel: r + 256 g + 65536 b
//   disparity_map_view intersect  data.pfm mask.pfm out.pfm int
//   disparity_map_view warp       right.pfm disparity.pfm out.pfm
// Disparities are {dx, dy, valid} 3-channel PFMs (int = 1: converted to PixelMask<Vector2i> and back), images 1-channel
// PFMs.  Exit status: 0 done, 1 any error.
#include <cstdio>
#include <cstdlib>
#include <string>

#include <vw/FileIO.h>
#include <vw/Stereo.h>

namespace {
using namespace vw;
typedef PixelMask<Vector2f> PixelF;
typedef PixelMask<Vector2i> PixelI;

ImageView<PixelI> to_int(ImageView<PixelF> const& f) {
  ImageView<PixelI> in(f.cols(), f.rows());
  for (int32 y = 0; y < f.rows(); ++y)
    for (int32 x = 0; x < f.cols(); ++x) {
      in(x, y) = PixelI(Vector2i((int32)f(x, y).child()[0], (int32)f(x, y).child()[1]));
      if (!is_valid(f(x, y))) in(x, y).invalidate();
    }
  return in;
}
ImageView<PixelF> to_float(ImageView<PixelI> const& d) {
  ImageView<PixelF> f(d.cols(), d.rows());
  for (int32 y = 0; y < d.rows(); ++y)
    for (int32 x = 0; x < d.cols(); ++x) {
      f(x, y) = PixelF(Vector2f((float)d(x, y).child()[0], (float)d(x, y).child()[1]));
      if (!is_valid(d(x, y))) f(x, y).invalidate();
    }
  return f;
}
ImageView<PixelF> to_float(ImageView<PixelF> const& d) { return d; }

Matrix3x3 matrix_from(char** argv) {
  Matrix3x3 m;
  for (int k = 0; k < 9; ++k) m(k / 3, k % 3) = std::atof(argv[k]);
  return m;
}

template <class PixelT>
int run(std::string const& mode, ImageView<PixelT> const& d, int argc, char** argv) {
  typedef typename PixelT::channel_type chan;
  if (mode == "range" && argc == 4) {
    stereo::BBox2f r = stereo::get_disparity_range(d);
    std::printf("%.9g %.9g %.9g %.9g\n", r.min()[0], r.min()[1], r.max()[0], r.max()[1]);
  } else if (mode == "mask" && argc == 10) {
    const PixelT mn((chan)std::atof(argv[5]), (chan)std::atof(argv[6])), mx((chan)std::atof(argv[7]), (chan)std::atof(argv[8]));
    write_image(argv[3], to_float(stereo::disparity_range_mask(d, mn, mx, std::atoi(argv[9]) != 0)));
  } else if (mode == "transform" && argc == 14) {
    write_image(argv[3], to_float(stereo::transform_disparities(d, HomographyTransform(matrix_from(argv + 5)))));
  } else if (mode == "subregion" && argc == 17) {
    const BBox2i sub(std::atoi(argv[6]), std::atoi(argv[7]), d.cols(), d.rows());
    write_image(argv[3], to_float(stereo::transform_disparities(std::atoi(argv[5]) != 0, sub, matrix_from(argv + 8), d)));
  } else if (mode == "subsample" && argc == 5) {
    write_image(argv[3], to_float(stereo::disparity_subsample(d)));
  } else if (mode == "upsample" && argc == 5) {
    write_image(argv[3], to_float(stereo::disparity_upsample(d)));
  } else if (mode == "missing" && argc == 5) {
    ImageView<stereo::PixelRGB8> rgb = stereo::missing_pixel_image(d);
    ImageView<float> out(rgb.cols(), rgb.rows());
    for (int32 y = 0; y < rgb.rows(); ++y)
      for (int32 x = 0; x < rgb.cols(); ++x) out(x, y) = (float)(rgb(x, y).r + 256 * rgb(x, y).g + 65536 * rgb(x, y).b);
    write_image(argv[3], out);
  } else {
    std::fprintf(stderr, "disparity_map_view: bad arguments\n");
    return 2;
  }
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s range|mask|transform|subregion|subsample|upsample|missing|intersect|warp ...\n", argv[0]);
    return 2;
  }
  const std::string mode = argv[1];
  int rc = 0;
  try {
    if (mode == "warp" && argc == 5) {
      ImageView<float> right = DiskImageView<float>(argv[2]);
      ImageView<PixelF> d = DiskImageView<PixelF>(argv[3]);
      write_image(argv[4], transform(right, stereo::DisparityTransform(d)));
    } else if (mode == "intersect" && argc == 6) {
      ImageView<PixelF> data = DiskImageView<PixelF>(argv[2]), mask = DiskImageView<PixelF>(argv[3]);
      if (std::atoi(argv[5])) write_image(argv[4], to_float(stereo::intersect_mask_and_data(to_int(data), to_int(mask))));
      else write_image(argv[4], stereo::intersect_mask_and_data(data, mask));
    } else {
      ImageView<PixelF> f = DiskImageView<PixelF>(argv[2]);
      const bool as_int = std::atoi(argv[mode == "range" ? 3 : 4]) != 0;
      rc = as_int ? run(mode, to_int(f), argc, argv) : run(mode, f, argc, argv);
    }
  } catch (std::exception const& e) {
    std::fprintf(stderr, "disparity_map_view: %s\n", e.what());
    return 1;
  }
  if (rc == 0) std::printf("disparity_map_view ok\n");
  return rc;
}
