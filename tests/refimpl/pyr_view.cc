// pyr_view.cc — the C++ surface of the Lucas-Kanade and Bayes-EM sub-pixel refiners (vwlite vw::stereo::lk_subpixel and
// bayes_em_subpixel, lazy PyramidSubpixelViews; PyramidSubpixelView with SUBPIXEL_PHASE) rasterised through
// block_write_image, as a reference user would write it.
//   pyr_view lk|em|phase disp.pfm left.pfm right.pfm out.pfm prefilter_mode prefilter_width kx ky max_pyramid_levels bw bh
// Exit status: 0 written, 3 NoImplErr, 1 any other error.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <vw/FileIO.h>
#include <vw/Stereo.h>

int main(int argc, char** argv) {
  using namespace vw;
  if (argc != 13) {
    std::fprintf(stderr, "usage: %s lk|em|phase disp left right out mode width kx ky levels bw bh\n", argv[0]);
    return 2;
  }
  try {
    DiskImageView<PixelMask<Vector2f>> disparity(argv[2]);
    DiskImageView<PixelGray<float>> left(argv[3]), right(argv[4]);
    const stereo::PrefilterModeType mode = (stereo::PrefilterModeType)std::atoi(argv[6]);
    const float width = (float)std::atof(argv[7]);
    const Vector2i kernel(std::atoi(argv[8]), std::atoi(argv[9]));
    const int levels = std::atoi(argv[10]);
    const Vector2i block(std::atoi(argv[11]), std::atoi(argv[12]));
    if (!std::strcmp(argv[1], "lk"))
      block_write_image(argv[5], stereo::lk_subpixel(disparity, left, right, mode, width, kernel, levels), block, 2);
    else if (!std::strcmp(argv[1], "em"))
      block_write_image(argv[5], stereo::bayes_em_subpixel(disparity, left, right, mode, width, kernel, levels), block, 2);
    else
      block_write_image(argv[5], stereo::PyramidSubpixelView(disparity, left, right, mode, width, kernel, levels,
                                                             stereo::SUBPIXEL_PHASE), block, 2);
  } catch (NoImplErr const& e) {
    std::fprintf(stderr, "pyr_view: NoImplErr: %s\n", e.what());
    return 3;
  } catch (std::exception const& e) {
    std::fprintf(stderr, "pyr_view: %s\n", e.what());
    return 1;
  }
  std::printf("pyr_view ok\n");
  return 0;
}
