// tile_range.h — TEST INFRASTRUCTURE ONLY: the search range PyramidSubpixelView::prerasterize takes of one tile,
// get_disparity_range(crop(disparity, bbox)) (src/vw/Stereo/SubpixelView.cc:42, DisparityMap.h:48-66), shared by the
// three restatements (affine_ref.cc, pyr_ref.cc, phase_ref.cc).
//
// The accumulator is PixelAccumulator<EWMinMaxAccumulator<Vector2f>> (Image/Statistics.h:193-224, :283-290): it takes
// the VALID pixels only (valid != 0), the first one sets both corners, every later one moves a corner per component;
// without any valid pixel the box is (0, 0, 0, 0).  What an invalid pixel stores never reaches the range.  The BBox2f
// becomes a BBox2i by a C cast of each corner (Math/BBox.tcc:49-50).  Valid pixels hold finite values.
#ifndef TESTS_REFIMPL_TILE_RANGE_H
#define TESTS_REFIMPL_TILE_RANGE_H

#include <cstddef>

// disp3: w x h x {dx, dy, valid} float, row-major; tile {x, y, w, h} inside it; out4 = {min x, min y, max x, max y}.
inline void tile_disparity_range(const float* disp3, int w, const int* tile, int* out4) {
  const int bx = tile[0], by = tile[1], bw = tile[2], bh = tile[3];
  float mnx = 0, mny = 0, mxx = 0, mxy = 0;
  bool any = false;
  for (int y = by; y < by + bh; ++y)
    for (int x = bx; x < bx + bw; ++x) {
      const float* q = disp3 + ((size_t)y * w + x) * 3;
      if (q[2] == 0.0f) continue;
      if (!any) {
        mnx = mxx = q[0];
        mny = mxy = q[1];
        any = true;
        continue;
      }
      if (q[0] < mnx) mnx = q[0]; else if (q[0] > mxx) mxx = q[0];
      if (q[1] < mny) mny = q[1]; else if (q[1] > mxy) mxy = q[1];
    }
  out4[0] = (int)mnx;
  out4[1] = (int)mny;
  out4[2] = (int)mxx;
  out4[3] = (int)mxy;
}

#endif
