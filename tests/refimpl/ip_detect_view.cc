// ip_detect_view.cc — the C++ surface of vw::ip detection and description (vwlite vw/InterestPoint.h), as tools/ipfind.cc
// calls it (:328-339, :395-400) apart from the disk image types.
//   ip_detect_view image.bin cols rows operator generator ip_per_tile gain prefix
//       image.bin     cols x rows floats
//       operator      obalog | iagd          generator   sgrad | sgrad2
//   Writes prefix.vwip (the described points), prefix.integral ((cols + 1) x (rows + 1) floats, IntegralImage of the image) and
//   prefix.whole.vwip (process_image of the same detector on the whole image as one tile, described by the generator's
//   operator() on the whole image).
// Exit status: 0 done, 1 any error.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <vw/InterestPoint.h>

using namespace vw;
using namespace vw::ip;

namespace {
struct Options { std::string interest_operator, descriptor_generator; int ip_per_tile; float ip_gain; };
const float IDEAL_OBALOG_THRESHOLD = .07;

template <class DetectorT>
InterestPointList whole(ImageView<float> const& image, DetectorT const& detector, Options const& opt) {
  InterestPointList ip = detector.process_image(image, opt.ip_per_tile);
  if (opt.descriptor_generator == "sgrad") {
    SGradDescriptorGenerator descriptor;
    descriptor(image, ip);
  } else {
    SGrad2DescriptorGenerator descriptor;
    descriptor(image, ip);
  }
  return ip;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 9) {
    std::fprintf(stderr, "usage: %s image.bin cols rows obalog|iagd sgrad|sgrad2 ip_per_tile gain prefix\n", argv[0]);
    return 2;
  }
  try {
    const int cols = std::atoi(argv[2]), rows = std::atoi(argv[3]);
    Options opt;
    opt.interest_operator = argv[4]; opt.descriptor_generator = argv[5];
    opt.ip_per_tile = std::atoi(argv[6]); opt.ip_gain = (float)std::atof(argv[7]);
    const std::string prefix = argv[8];
    ImageView<PixelGray<float>> image(cols, rows);
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 1;
    const size_t got = std::fread(image.data(), sizeof(float), (size_t)cols * rows, f);
    std::fclose(f);
    if (got != (size_t)cols * rows) return 1;

    InterestPointList ip, ip_whole;
    if (opt.interest_operator == "obalog") {
      // OBALoG threshold is inversely proportional to gain ..
      OBALoGInterestOperator interest_operator(IDEAL_OBALOG_THRESHOLD/opt.ip_gain);
      IntegralInterestPointDetector detector(interest_operator, opt.ip_per_tile);
      ip = detect_interest_points(vw::pixel_cast<float>(image), detector, opt.ip_per_tile);
      ip_whole = whole(ImageView<float>(vw::pixel_cast<float>(image)), detector, opt);
    } else if (opt.interest_operator == "iagd") {
      IntegralAutoGainDetector detector(opt.ip_per_tile);
      ip = detect_interest_points(vw::pixel_cast<float>(image), detector, opt.ip_per_tile);
      ip_whole = whole(ImageView<float>(vw::pixel_cast<float>(image)), detector, opt);
    } else {
      return 1;
    }
    if (opt.descriptor_generator == "sgrad") {
      SGradDescriptorGenerator descriptor;
      describe_interest_points(image, descriptor, ip);
    } else if (opt.descriptor_generator == "sgrad2") {
      SGrad2DescriptorGenerator descriptor;
      describe_interest_points(image, descriptor, ip);
    } else {
      return 1;
    }
    write_binary_ip_file(prefix + ".vwip", ip);
    write_binary_ip_file(prefix + ".whole.vwip", ip_whole);
    ImageView<float> integral = IntegralImage(image);
    f = std::fopen((prefix + ".integral").c_str(), "wb");
    if (!f) return 1;
    const size_t put = std::fwrite(integral.data(), sizeof(float), (size_t)integral.cols() * integral.rows(), f);
    if (std::fclose(f) != 0 || put != (size_t)integral.cols() * integral.rows()) return 1;
  } catch (std::exception const& e) {
    std::fprintf(stderr, "ip_detect_view: %s\n", e.what());
    return 1;
  }
  std::printf("ip_detect_view ok\n");
  return 0;
}
