// mosaic_view.cc — the C++ surface of the image composite (vwlite vw::mosaic::ImageComposite), as a reference user would
// call it.
//   mosaic_view channels fill_holes draft out.bin px py  [image.bin cols rows x y]...
// Every image.bin holds rows x cols pixels of `channels` float32 (2 = PixelGrayA<float>, 4 = PixelRGBA<float>); out.bin
// receives generate_patch over the whole view.  Prints "cols rows levels", the data box, the view box and the channels of
// operator()(px, py).  Exit status: 0 done, 1 any error.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <vw/Mosaic.h>

namespace {
using namespace vw;

template <class PixelT>
int run(int channels, int argc, char** argv) {
  mosaic::ImageComposite<PixelT> composite;
  composite.set_fill_holes(std::atoi(argv[2]) != 0);
  composite.set_draft_mode(std::atoi(argv[3]) != 0);
  for (int a = 7; a + 4 < argc; a += 5) {
    const int cols = std::atoi(argv[a + 1]), rows = std::atoi(argv[a + 2]);
    ImageView<PixelT> image(cols, rows);
    FILE* f = std::fopen(argv[a], "rb");
    if (!f || std::fread(image.data(), sizeof(PixelT), (size_t)cols * rows, f) != (size_t)cols * rows) {
      std::fprintf(stderr, "mosaic_view: cannot read %s\n", argv[a]);
      return 1;
    }
    std::fclose(f);
    composite.insert(image, std::atoi(argv[a + 3]), std::atoi(argv[a + 4]));
  }
  composite.prepare();
  ImageView<PixelT> out = composite.generate_patch(BBox2i(0, 0, composite.cols(), composite.rows()));
  FILE* f = std::fopen(argv[4], "wb");
  if (!f || std::fwrite(out.data(), sizeof(PixelT), (size_t)out.cols() * out.rows(), f) != (size_t)out.cols() * out.rows()) {
    std::fprintf(stderr, "mosaic_view: cannot write %s\n", argv[4]);
    return 1;
  }
  std::fclose(f);
  std::printf("%d %d %d\n", composite.cols(), composite.rows(), composite.levels());
  BBox2i const &d = composite.bbox(), &v = composite.source_data_bbox();
  std::printf("%d %d %d %d\n", d.min()[0], d.min()[1], d.max()[0], d.max()[1]);
  std::printf("%d %d %d %d\n", v.min()[0], v.min()[1], v.max()[0], v.max()[1]);
  const PixelT one = composite(std::atoi(argv[5]), std::atoi(argv[6]));
  for (int k = 0; k < channels; ++k) std::printf("%.9g%c", one[k], k + 1 < channels ? ' ' : '\n');
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 12 || (argc - 7) % 5 != 0) {
    std::fprintf(stderr, "usage: %s channels fill_holes draft out.bin px py [image.bin cols rows x y]...\n", argv[0]);
    return 2;
  }
  const int channels = std::atoi(argv[1]);
  try {
    const int rc = channels == 2 ? run<vw::PixelGrayA<float>>(2, argc, argv) : channels == 4 ? run<vw::PixelRGBA<float>>(4, argc, argv) : 2;
    if (rc) return rc;
  } catch (std::exception const& e) {
    std::fprintf(stderr, "mosaic_view: %s\n", e.what());
    return 1;
  }
  std::printf("mosaic_view ok\n");
  return 0;
}
