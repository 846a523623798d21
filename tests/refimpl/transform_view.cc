// transform_view.cc — the C++ surface of vw::transform (vwlite vw/Transform.h), as a reference user would call it.
//   transform_view src.bin mask.bin cols rows prefix
//       src.bin cols x rows floats with mask.bin bytes (together a PixelMask<float> image).  Writes, as raw floats (and
//       bytes for prefix.NAME_mask):
//         prefix.affine     transform(src, AffineTransform, 70, 9, ReflectEdgeExtension, BicubicInterpolation)
//         prefix.chain      transform(masked, compose(Translate, Rotate, Resample), BBox2i(-20, -3, 130, 11),
//                           ValueEdgeExtension(7.5 valid)), rasterised in 32 x 8 tiles as a block rasteriser would ask
//         prefix.resample   resample(src, 0.5)          prefix.resize   resize(src, 51, 9)
//         prefix.translate  translate(src, 3, -2) (the int form)        prefix.rotate   rotate(src, 0.3, (34.5, 22))
//         prefix.nodata     transform_nodata(masked, InverseTransform<AffineTransform>, 70, 9, ConstantEdgeExtension,
//                           BicubicInterpolation, an invalid -1)
//         prefix.periodic   transform(PixelGray<float> src, HomographyTransform, 70, 9, PeriodicEdgeExtension, NearestPixelInterpolation)
//         prefix.meta       doubles: RotateTransform(pi / 2, (1, 1)) forward and reverse of (3, 1), the chain's forward and
//                           the inverse's forward of (12, 7)
// Exit status: 0 done, 1 any error.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <vw/Transform.h>

namespace {
using namespace vw;

template <class T>
bool read_raw(std::string const& path, T* data, size_t n) {
  std::FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  const size_t got = std::fread(data, sizeof(T), n, f);
  std::fclose(f);
  return got == n;
}
template <class T>
bool write_raw(std::string const& path, const T* data, size_t n) {
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const size_t put = std::fwrite(data, sizeof(T), n, f);
  return std::fclose(f) == 0 && put == n;
}
bool write_image(std::string const& path, ImageView<float> const& im) { return write_raw(path, im.data(), (size_t)im.cols() * im.rows()); }
bool write_image(std::string const& path, ImageView<PixelMask<float>> const& im) {
  const size_t n = (size_t)im.cols() * im.rows();
  std::vector<float> v(n);
  std::vector<uint8> m(n);
  for (size_t i = 0; i < n; ++i) {
    v[i] = im.data()[i].child();
    m[i] = im.data()[i].valid() != 0 ? 255 : 0;
  }
  return write_raw(path, v.data(), n) && write_raw(path + "_mask", m.data(), n);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: %s src.bin mask.bin cols rows prefix\n", argv[0]);
    return 2;
  }
  try {
    const int w = std::atoi(argv[3]), h = std::atoi(argv[4]);
    const std::string prefix = argv[5];
    ImageView<float> src(w, h);
    std::vector<uint8> mask((size_t)w * h);
    if (!read_raw(argv[1], src.data(), mask.size()) || !read_raw(argv[2], mask.data(), mask.size())) return 1;
    ImageView<PixelMask<float>> masked(w, h);
    ImageView<PixelGray<float>> gray(w, h);
    for (size_t i = 0; i < mask.size(); ++i) {
      masked.data()[i] = PixelMask<float>(src.data()[i]);
      if (!mask[i]) masked.data()[i].invalidate();
      gray.data()[i] = PixelGray<float>(src.data()[i]);
    }
    const AffineTransform shear(Matrix2x2(1.1, 0.2, -0.1, 0.9), Vector2(3.5, -2.25));
    ImageView<float> affine = transform(src, shear, 70, 9, ReflectEdgeExtension(), BicubicInterpolation());

    const BBox2i box(-20, -3, 130, 11);
    auto chain_tx = compose(TranslateTransform(2.5, -1.0), RotateTransform(0.2, Vector2(30.0, 20.0)), ResampleTransform(1.25, 0.8));
    auto view = transform(masked, chain_tx, box, ValueEdgeExtension<PixelMask<float>>(PixelMask<float>(7.5f)));
    ImageView<PixelMask<float>> chain(box.width(), box.height());
    for (int y = 0; y < box.height(); y += 8)
      for (int x = 0; x < box.width(); x += 32) {
        const BBox2i tile(x, y, std::min(32, box.width() - x), std::min(8, box.height() - y));
        view.rasterize(crop(chain, tile), tile);
      }

    ImageView<float> resampled = resample(src, 0.5);
    ImageView<float> resized = resize(src, 51, 9);
    ImageView<float> translated = translate(src, 3, -2);
    ImageView<float> rotated = rotate(src, 0.3, Vector2(34.5, 22.0));
    PixelMask<float> nodata(-1.0f);
    nodata.invalidate();
    ImageView<PixelMask<float>> with_nodata =
        transform_nodata(masked, InverseTransform<AffineTransform>(shear), 70, 9, ConstantEdgeExtension(), BicubicInterpolation(), nodata);
    Matrix3x3 H;
    const double hw[9] = {1.01, 0.02, -1.5, -0.01, 0.99, 2.0, 1e-4, -2e-4, 1.0};
    for (int i = 0; i < 9; ++i) H(i / 3, i % 3) = hw[i];
    ImageView<PixelGray<float>> periodic_gray = transform(gray, HomographyTransform(H), 70, 9, PeriodicEdgeExtension(), NearestPixelInterpolation());
    ImageView<float> periodic(70, 9);
    for (size_t i = 0; i < (size_t)70 * 9; ++i) periodic.data()[i] = periodic_gray.data()[i].v();

    const RotateTransform quarter(std::acos(-1.0) / 2, Vector2(1, 1));
    const Vector2 f = quarter.forward(Vector2(3, 1)), r = quarter.reverse(Vector2(3, 1)), cf = chain_tx.forward(Vector2(12, 7)),
                  inv = InverseTransform<AffineTransform>(shear).forward(Vector2(12, 7));
    const double meta[8] = {f[0], f[1], r[0], r[1], cf[0], cf[1], inv[0], inv[1]};
    if (resampled.cols() != int(.5 + w * 0.5) || resampled.rows() != int(.5 + h * 0.5) || resized.cols() != 51 || resized.rows() != 9 ||
        translated.cols() != w || rotated.rows() != h)
      return 1;
    if (!write_image(prefix + ".affine", affine) || !write_image(prefix + ".chain", chain) || !write_image(prefix + ".resample", resampled) ||
        !write_image(prefix + ".resize", resized) || !write_image(prefix + ".translate", translated) || !write_image(prefix + ".rotate", rotated) ||
        !write_image(prefix + ".nodata", with_nodata) || !write_image(prefix + ".periodic", periodic) || !write_raw(prefix + ".meta", meta, 8))
      return 1;
  } catch (std::exception const& e) {
    std::fprintf(stderr, "transform_view: %s\n", e.what());
    return 1;
  }
  std::printf("transform_view ok\n");
  return 0;
}
