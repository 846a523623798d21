// ip_integral.h — IntegralImage (src/vw/InterestPoint/IntegralImage.h:43-91) in the reference's own order, by one wave.
//
// Every word is ((src(x, y) + I(x, y + 1)) + I(x + 1, y)) - I(x, y) with each operation rounded to float, so a word needs
// its left, upper and upper-left neighbours finished: a prefix-sum scan rounds differently and gives other interest
// values.  What is parallel is the anti-diagonal.  A wave takes 64 rows at a time (a band), lane l the row y0 + l, and
// walks the band skewed: at step t lane l is at column t - l.  Its left neighbour is its own previous word, its upper
// neighbour is what lane l - 1 produced one step earlier (one DPP move across the wave), its upper-left neighbour is the
// upper one of the step before.  Lane 0 reads the last row of the previous band from memory, which the same wave wrote
// and fenced.  Source words and lane 0's row are fetched IPI_CHUNK steps ahead so that a band pays one memory latency
// per chunk, not per step.  No workgroup waits on another: a launch gives every image to one wave.
#pragma once
#include <hip/hip_runtime.h>

constexpr int IPI_CHUNK = 16;

// the value lane l - 1 holds, for lane l >= 1; lane 0 keeps its own (v_mov_b32 wave_shr:1)
__device__ inline float ipi_from_lane_below(float v) {
  const int i = __float_as_int(v);
  return __int_as_float(__builtin_amdgcn_update_dpp(i, i, 0x138, 0xf, 0xf, false));
}

// src: w x h floats, sstride apart; out: (w + 1) x (h + 1) floats, ostride apart.  GLOBAL: out is global memory (the
// band hand-over needs a device fence); otherwise LDS.  Called by all 64 lanes of one wave, converged.
template <bool GLOBAL>
__device__ inline void ipi_wave_integral(const float* src, long long sstride, int w, int h, float* out, long long ostride) {
  const int lane = threadIdx.x & 63;
  for (int x = lane; x <= w; x += 64) out[x] = 0.0f;
  for (int y = lane + 1; y <= h; y += 64) out[(long long)y * ostride] = 0.0f;
  if (GLOBAL) __threadfence(); else __threadfence_block();
  const int steps = w + 63;
  for (int y0 = 0; y0 < h; y0 += 64) {
    const int y = y0 + lane;
    const bool row = y < h;
    const float* srow = src + (long long)(row ? y : 0) * sstride;
    float* orow = out + (long long)(y + 1) * ostride;
    const float* prow = out + (long long)y0 * ostride;     // the row above the band
    float left = 0.0f, upleft = 0.0f, cur = 0.0f;
    float s[IPI_CHUNK], u[IPI_CHUNK];
    // every fetch is unconditional at a clamped, valid address: a fetch under a condition becomes a branch around it, and a
    // step that does not use its words ignores them
#pragma unroll
    for (int k = 0; k < IPI_CHUNK; ++k) {
      const int x = min(max(k - lane, 0), w - 1);
      s[k] = srow[x];
      u[k] = prow[x + 1];
    }
    for (int t0 = 0; t0 < steps; t0 += IPI_CHUNK) {
      float sn[IPI_CHUNK], un[IPI_CHUNK];
#pragma unroll
      for (int k = 0; k < IPI_CHUNK; ++k) {       // the next chunk's words, in flight during this chunk's steps
        const int x = min(max(t0 + IPI_CHUNK + k - lane, 0), w - 1);
        sn[k] = srow[x];
        un[k] = prow[x + 1];
      }
#pragma unroll
      for (int k = 0; k < IPI_CHUNK; ++k) {
        const int x = t0 + k - lane;
        const bool on = row && x >= 0 && x < w;
        float up = ipi_from_lane_below(cur);
        if (lane == 0) up = u[k];
        const float v = ((s[k] + left) + up) - upleft;
        if (on) orow[x + 1] = v;
        left = on ? v : left;
        upleft = on ? up : upleft;
        cur = on ? v : cur;
      }
#pragma unroll
      for (int k = 0; k < IPI_CHUNK; ++k) { s[k] = sn[k]; u[k] = un[k]; }
    }
    if (GLOBAL) __threadfence(); else __threadfence_block();
  }
}
