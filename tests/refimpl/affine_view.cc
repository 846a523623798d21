// affine_view.cc — the C++ surface of affine sub-pixel refinement (vwlite vw::stereo::affine_subpixel, a lazy
// PyramidSubpixelView) rasterised through block_write_image, as a reference user would write it.
//   affine_view disp.pfm left.pfm right.pfm out.pfm prefilter_mode prefilter_width kx ky max_pyramid_levels block_w block_h
#include <cstdio>
#include <cstdlib>

#include <vw/FileIO.h>
#include <vw/Stereo.h>

int main(int argc, char** argv) {
  using namespace vw;
  if (argc != 12) {
    std::fprintf(stderr, "usage: %s disp left right out mode width kx ky levels bw bh\n", argv[0]);
    return 2;
  }
  try {
    DiskImageView<PixelMask<Vector2f>> disparity(argv[1]);
    DiskImageView<PixelGray<float>> left(argv[2]), right(argv[3]);
    const Vector2i kernel(std::atoi(argv[7]), std::atoi(argv[8]));
    block_write_image(argv[4],
                      stereo::affine_subpixel(disparity, left, right, (stereo::PrefilterModeType)std::atoi(argv[5]),
                                              (float)std::atof(argv[6]), kernel, std::atoi(argv[9])),
                      Vector2i(std::atoi(argv[10]), std::atoi(argv[11])), 2);
  } catch (std::exception const& e) {
    std::fprintf(stderr, "affine_view: %s\n", e.what());
    return 1;
  }
  std::printf("affine_view ok\n");
  return 0;
}
