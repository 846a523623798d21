// zone_task.h — the zone tables of the batched zone matcher (bm_zones.hip) as plain host data: what the pyramid plan
// (pyramid_plan.h) fills in and the launchers of vwgpu_internal.h take.  No HIP in here.
#pragma once
#include <cstddef>

// bm_zones.hip — one row per search zone (or per R->L zone image); see the kernels for the field meaning
struct vwgpu_zone_task {
  int ax, ay;          // origin of the zone's input crop in image A (may lie outside: coordinates are clamped)
  int bx, by;          // origin in image B of the window for disparity (0,0)
  int zw, zh;          // output size
  int sx, sy;          // search volume
  int out_off;         // pixel offset of the zone's first output pixel in the output buffer
  int out_stride;      // pixels
  int addx, addy;      // added to the winning disparity index of every pixel
  int img = 0;         // zone-matcher groups (vwgpu_zone_group): which image pair of the group the zone belongs to
};
// A launch sequence of the zone matcher over several image pairs of EQUAL geometry laid out at a fixed stride (the tiles of a
// pyramid_correlate group, pyramid.hip): image pair i = (A + i * a_stride, B + i * b_stride); zones name theirs in vwgpu_zone_task::img.
struct vwgpu_zone_group {
  int n_img = 1;
  size_t a_stride = 0, b_stride = 0;       // floats
  const int* cert_hi = nullptr;            // n_img largest exponents (certified passes; overrides the cert_hi argument)
  const int* edge_lo = nullptr;            // n_img bounds of the "cannot matter" certificate (override edge_lo / edge_hi)
  const int* edge_hi = nullptr;
};
inline size_t vwgpu_zone_row_flags(const vwgpu_zone_task* zones, int n) {
  size_t r = 0;
  for (int i = 0; i < n; ++i) r += (size_t)(zones[i].zh + 31) / 32;
  return r;
}
