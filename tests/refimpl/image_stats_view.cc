// image_stats_view.cc — the C++ surface of the image statistics and intensity scaling (vwlite vw/Image.h, vw/Math.h), as a
// reference user would call them.
//   image_stats_view image.bin cols rows nodata|none prefix
// image.bin: cols x rows floats.  With a nodata value the statistics run on the PixelMask<float> image that create_mask would
// give (pixels equal to nodata invalid).  Prints one "name value" line per statistic, doubles as C99 hexadecimal floats, and
// writes prefix.psc (percentile_scale_convert, uint8), prefix.u8 (u8_convert, uint8), prefix.norm (normalize(image), float),
// prefix.clamp (clamp(image, 0.25, 0.75)) and prefix.thresh (threshold(image, 0.5, -1, 2)).  Exit status: 0 done, 1 any error.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <vw/Image.h>
#include <vw/Math.h>

namespace {
using namespace vw;

template <class T>
void dump(std::string const& path, const T* data, size_t n) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f || std::fwrite(data, sizeof(T), n, f) != n) vw_throw(IOErr() << "cannot write " << path);
  std::fclose(f);
}

template <class PixelT>
void run(ImageView<PixelT> const& image, std::string const& prefix) {
  const size_t n = (size_t)image.cols() * image.rows();
  double mn, mx;
  find_image_min_max(image, mn, mx);
  std::printf("min %a\nmax %a\n", mn, mx);
  float amn, amx;
  min_max_channel_values(image, amn, amx);
  std::printf("accumulator_min %a\naccumulator_max %a\n", (double)amn, (double)amx);
  std::printf("sum %a\nmean %a\nstddev %a\nmedian %a\n", sum_of_channel_values(image), mean_channel_value(image),
              stddev_channel_value(image), median_channel_value(image));
  math::Histogram hist;
  histogram(image, 256, mn, mx, hist);
  std::printf("total %llu\nlow_bin %zu\nhigh_bin %zu\nbin_width %a\nbin_17 %a\n", (unsigned long long)hist.get_total_num_values(),
              hist.get_percentile(0.02), hist.get_percentile(0.98), hist.get_bin_width(), hist.get_bin_value(17));
  std::printf("otsu %a\notsu_sampled %a\n", otsu_threshold(image), otsu_threshold(image, 23, 17, 64));
  ImageView<uint8> psc;
  percentile_scale_convert(image, psc);
  dump(prefix + ".psc", psc.data(), n);
  ImageView<PixelGray<uint8>> u8;
  u8_convert(image, u8);
  dump(prefix + ".u8", reinterpret_cast<const uint8*>(u8.data()), n);
  detail::GrayOperand norm = detail::gray_operand(normalize(image));
  dump(prefix + ".norm", norm.values.data(), n);
  detail::GrayOperand cl = detail::gray_operand(clamp(image, 0.25, 0.75));
  dump(prefix + ".clamp", cl.values.data(), n);
  detail::GrayOperand th = detail::gray_operand(threshold(image, 0.5, -1.0, 2.0));
  dump(prefix + ".thresh", th.values.data(), n);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: %s image.bin cols rows nodata|none prefix\n", argv[0]);
    return 2;
  }
  try {
    const int cols = std::atoi(argv[2]), rows = std::atoi(argv[3]);
    ImageView<float> raw(cols, rows);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(raw.data(), sizeof(float), (size_t)cols * rows, f) != (size_t)cols * rows) {
      std::fprintf(stderr, "image_stats_view: cannot read %s\n", argv[1]);
      return 1;
    }
    std::fclose(f);
    if (std::strcmp(argv[4], "none") == 0) {
      run(raw, argv[5]);
    } else {
      const float nodata = (float)std::atof(argv[4]);
      ImageView<PixelMask<float>> masked(cols, rows);
      for (int32 r = 0; r < rows; ++r)
        for (int32 c = 0; c < cols; ++c)
          if (raw(c, r) != nodata) masked(c, r) = PixelMask<float>(raw(c, r));
      run(masked, argv[5]);
    }
  } catch (std::exception const& e) {
    std::fprintf(stderr, "image_stats_view: %s\n", e.what());
    return 1;
  }
  std::printf("image_stats_view ok\n");
  return 0;
}
