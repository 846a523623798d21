// hole_fill_view.cc — the C++ surface of the hole filling (vwlite vw::grassfire, BlobIndexThreaded, inpaint,
// fill_holes_grass, fill_nodata_with_avg, get_blob_sizes, applyErodeView), as a reference user would call them.
//   hole_fill_view fill_holes disparity.pfm out.pfm len      fill_holes_grass(d, len)
//   hole_fill_view inpaint    disparity.pfm out.pfm len      BlobIndexThreaded(invert_mask(d), len * len); wipe_big_blobs(len); inpaint
//   hole_fill_view blobs      disparity.pfm len              prints the blob count of that index and min.x min.y max.x max.y per blob
//   hole_fill_view erode      disparity.pfm out.pfm area     applyErodeView(d, BlobIndexThreaded(d, area))
//   hole_fill_view sizes      disparity.pfm out.pfm limit    get_blob_sizes(d, 0, limit) in channel 0
//   hole_fill_view grassfire  disparity.pfm out.pfm ignore   grassfire of the validity channel in channel 0
//   hole_fill_view avg        masked.pfm out.pfm kernel      fill_nodata_with_avg on PixelMask<float> {value, valid, -}
// Disparities are {dx, dy, valid} 3-channel PFMs.  Exit status: 0 done, 1 any error.
#include <cstdio>
#include <cstdlib>
#include <string>

#include <vw/FileIO.h>
#include <vw/Image.h>

namespace {
using namespace vw;
typedef PixelMask<Vector2f> PixelF;

BlobIndexThreaded holes_of(ImageView<PixelF> const& d, int len) {
  BlobIndexThreaded bindex(invert_mask(d), len * len);
  bindex.wipe_big_blobs(len);
  return bindex;
}

template <class T>
ImageView<PixelF> in_channel_0(ImageView<T> const& v) {
  ImageView<PixelF> out(v.cols(), v.rows());
  for (int32 y = 0; y < v.rows(); ++y)
    for (int32 x = 0; x < v.cols(); ++x) out(x, y) = PixelF(Vector2f((float)v(x, y), 0.0f));
  return out;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s fill_holes|inpaint|blobs|erode|sizes|grassfire|avg ...\n", argv[0]);
    return 2;
  }
  const std::string mode = argv[1];
  try {
    if (mode == "avg" && argc == 5) {
      ImageView<PixelMask<float>> m = DiskImageView<PixelMask<float>>(argv[2]);
      write_image(argv[3], fill_nodata_with_avg(m, std::atoi(argv[4])));
    } else if (mode == "blobs" && argc == 4) {
      ImageView<PixelF> d = DiskImageView<PixelF>(argv[2]);
      BlobIndexThreaded bindex = holes_of(d, std::atoi(argv[3]));
      std::printf("%u\n", bindex.num_blobs());
      for (uint32 k = 0; k < bindex.num_blobs(); ++k) {
        BBox2i const& b = bindex.blob_bbox(k);
        std::printf("%d %d %d %d\n", b.min().x(), b.min().y(), b.max().x(), b.max().y());
      }
      return 0;
    } else if (argc == 5) {
      ImageView<PixelF> d = DiskImageView<PixelF>(argv[2]);
      const int n = std::atoi(argv[4]);
      if (mode == "fill_holes") {
        write_image(argv[3], fill_holes_grass(d, n));
      } else if (mode == "inpaint") {
        write_image(argv[3], inpaint(d, holes_of(d, n), true, PixelF()));
      } else if (mode == "erode") {
        write_image(argv[3], applyErodeView(d, BlobIndexThreaded(d, n)));
      } else if (mode == "sizes") {
        write_image(argv[3], in_channel_0(get_blob_sizes(d, 0, (uint32)n)));
      } else if (mode == "grassfire") {
        ImageView<float> v(d.cols(), d.rows());
        for (int32 y = 0; y < d.rows(); ++y)
          for (int32 x = 0; x < d.cols(); ++x) v(x, y) = d(x, y).valid();
        write_image(argv[3], in_channel_0(grassfire(v, n != 0)));
      } else {
        std::fprintf(stderr, "hole_fill_view: bad arguments\n");
        return 2;
      }
    } else {
      std::fprintf(stderr, "hole_fill_view: bad arguments\n");
      return 2;
    }
  } catch (std::exception const& e) {
    std::fprintf(stderr, "hole_fill_view: %s\n", e.what());
    return 1;
  }
  std::printf("hole_fill_view ok\n");
  return 0;
}
