// phase_view.cc — the C++ surface of the phase sub-pixel refiner (vwlite vw::stereo::phase_subpixel, a lazy
// PyramidSubpixelView with SUBPIXEL_PHASE and the phase accuracy) rasterised through block_write_image, as a reference
// user would write it.
//   phase_view disp.pfm left.pfm right.pfm out.pfm prefilter_mode prefilter_width kx ky max_pyramid_levels accuracy bw bh
// Exit status: 0 written, 3 NoImplErr, 1 any other error.
#include <cstdio>
#include <cstdlib>

#include <vw/FileIO.h>
#include <vw/Stereo.h>

int main(int argc, char** argv) {
  using namespace vw;
  if (argc != 13) {
    std::fprintf(stderr, "usage: %s disp left right out mode width kx ky levels accuracy bw bh\n", argv[0]);
    return 2;
  }
  try {
    DiskImageView<PixelMask<Vector2f>> disparity(argv[1]);
    DiskImageView<PixelGray<float>> left(argv[2]), right(argv[3]);
    const stereo::PrefilterModeType mode = (stereo::PrefilterModeType)std::atoi(argv[5]);
    const float width = (float)std::atof(argv[6]);
    const Vector2i kernel(std::atoi(argv[7]), std::atoi(argv[8]));
    const int levels = std::atoi(argv[9]), accuracy = std::atoi(argv[10]);
    const Vector2i block(std::atoi(argv[11]), std::atoi(argv[12]));
    block_write_image(argv[4], stereo::phase_subpixel(disparity, left, right, mode, width, kernel, levels, accuracy), block, 2);
  } catch (NoImplErr const& e) {
    std::fprintf(stderr, "phase_view: NoImplErr: %s\n", e.what());
    return 3;
  } catch (std::exception const& e) {
    std::fprintf(stderr, "phase_view: %s\n", e.what());
    return 1;
  }
  std::printf("phase_view ok\n");
  return 0;
}
