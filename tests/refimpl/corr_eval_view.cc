// corr_eval_view.cc — the C++ surface of disparity quality evaluation (vwlite vw::stereo::corr_eval, a lazy CorrEval
// view) rasterised through block_write_image, as a reference user would write it.
//   corr_eval_view left.pfm right.pfm disp.pfm out.pfm kx ky metric sample_rate round_to_int prefilter_width bw bh
// left / right are masked images ({value, valid, 0} 3-channel PFMs); out is PixelMask<float> ({value, valid, 0}).
// Exit status: 0 written, 3 NoImplErr, 1 any other error.
#include <cstdio>
#include <cstdlib>
#include <string>

#include <vw/FileIO.h>
#include <vw/Stereo.h>

int main(int argc, char** argv) {
  using namespace vw;
  if (argc != 13) {
    std::fprintf(stderr, "usage: %s left right disp out kx ky metric rate round width bw bh\n", argv[0]);
    return 2;
  }
  try {
    DiskImageView<PixelMask<float>> left(argv[1]), right(argv[2]);
    DiskImageView<PixelMask<Vector2f>> disparity(argv[3]);
    const Vector2i kernel(std::atoi(argv[5]), std::atoi(argv[6]));
    const std::string metric = argv[7];
    const int rate = std::atoi(argv[8]);
    const bool round_to_int = std::atoi(argv[9]) != 0;
    const float width = (float)std::atof(argv[10]);
    const Vector2i block(std::atoi(argv[11]), std::atoi(argv[12]));
    block_write_image(argv[4], stereo::corr_eval(left, right, disparity, kernel, metric, rate, round_to_int, 0, width),
                      block, 2);
  } catch (NoImplErr const& e) {
    std::fprintf(stderr, "corr_eval_view: NoImplErr: %s\n", e.what());
    return 3;
  } catch (std::exception const& e) {
    std::fprintf(stderr, "corr_eval_view: %s\n", e.what());
    return 1;
  }
  std::printf("corr_eval_view ok\n");
  return 0;
}
