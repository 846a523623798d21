// ip_match.hip — InterestPointMatcherSimple and the index-list call of InterestPointMatcher (src/vw/InterestPoint/Matcher.h:282-386,
// :435-508) with L2NormMetric and HammingMetric (Matcher.cc:34-102) and the two constraints (:119-147), as an exact search: for every
// point of list 1 the smallest and the second smallest distance to the points of list 2 and the lowest index of the smallest, then the
// reference's accept decision.  include/vwgpu.h states what is reproduced, tests/refimpl/ip_match_ref.cc restates it, DESIGN §4.21.
//
// Schedule.  ipm_chunk_kernel: a lane is a query (a wave is 64 queries, a workgroup IPM_THREADS), blockIdx.y a chunk of list 2.  The query
// lives in SEG registers (floats, or words of four descriptor bytes); the chunk passes through LDS in tiles of IPM_TILE candidates, and
// all lanes read a candidate's element at one address (a broadcast).  IPM_CG candidates are in flight per lane, each with ONE float
// accumulator that takes its terms in the order k = 0 .. K-1: the sum over k is never split (the differences and squares of two
// adjacent elements come from one packed instruction each, the adds stay two).  K <= SEG: the query is loaded once.  K > SEG
// (L2 only, SEG = 128): K is cut into segments; per tile and segment the query registers are reloaded and a candidate's accumulator
// waits in LDS (`carry`, touched by its own lane only).  Elements past K are zeros on both sides: acc + 0 * 0 == acc for every acc the
// sum can hold.  Each workgroup leaves (first, second, index) per query and chunk; ipm_merge_kernel folds the chunks in ascending order —
// min / second-min of the union, the lower index on a tie — decides, checks the constraint, writes the outputs and counts.
#include <cmath>
#include <type_traits>

#include "vwgpu_internal.h"

namespace {

// tools builds (make ipvariant IPM_FLAGS=-D...; tools/time_ip_match.py --other) set other values; IPM_TILE is a multiple of IPM_CG
#ifndef IPM_TILE
#define IPM_TILE 32       // candidates per LDS tile
#endif
#ifndef IPM_CG
#define IPM_CG 4          // candidates in flight per lane
#endif
#ifndef IPM_CHUNK
#define IPM_CHUNK 256     // candidates per workgroup, while that gives at most IPM_MAX_CHUNKS chunks
#endif
static_assert(IPM_TILE % IPM_CG == 0 && IPM_CHUNK % IPM_TILE == 0, "a chunk is whole tiles, a tile whole candidate groups");
constexpr int IPM_THREADS = 256;
constexpr int IPM_MAX_CHUNKS = 256;
constexpr int IPM_QBATCH = 1 << 18;       // queries per launch: bounds the partial results to 12 * IPM_QBATCH * IPM_MAX_CHUNKS bytes
constexpr int IPM_MAX_K = 512;

int ipm_chunk_of(long long n2) {
  const long long per = (n2 + IPM_MAX_CHUNKS - 1) / IPM_MAX_CHUNKS;
  const long long c = (per + IPM_CHUNK - 1) / IPM_CHUNK * IPM_CHUNK;
  return (int)std::max<long long>(c, IPM_CHUNK);
}

typedef float ipm_f2 __attribute__((ext_vector_type(2)));   // two adjacent descriptor elements (SEG is even, the tile 16-byte aligned)

struct ipm_args {
  const void* d1; long long s1; int n1;   // the queries of this launch
  const void* d2; long long s2; int n2;
  int k, nseg, chunk;
  const uint8_t *p1, *p2;
  float *pf, *ps; int* pi;                // [chunks][n1]
};

template <int METRIC, int SEG, bool POL>
__global__ __launch_bounds__(IPM_THREADS) void ipm_chunk_kernel(ipm_args a) {
  constexpr bool L2 = METRIC == VWGPU_IP_METRIC_L2;
  using word = typename std::conditional<L2, float, uint32_t>::type;   // a descriptor element, or four descriptor bytes
  using sum = typename std::conditional<L2, float, int>::type;
  __shared__ __attribute__((aligned(16))) word tile[IPM_TILE * SEG];
  __shared__ uint8_t tpol[IPM_TILE];
  extern __shared__ float carry[];   // [IPM_TILE][IPM_THREADS] when nseg > 1

  const int tid = threadIdx.x;
  const long long i = (long long)blockIdx.x * IPM_THREADS + tid;
  const bool live = i < a.n1;
  const long long row = live ? i : a.n1 - 1;
  const long long jb = (long long)blockIdx.y * a.chunk;
  const long long je = jb + a.chunk < a.n2 ? jb + a.chunk : a.n2;
  const uint8_t mypol = POL ? a.p1[row] : 0;

  word q[SEG];
  auto load_query = [&](int seg) {
#pragma unroll
    for (int k = 0; k < SEG; ++k) {
      const int kk = seg * SEG + k;
      if (L2) {
        q[k] = kk < a.k ? static_cast<const word*>(a.d1)[row * a.s1 + kk] : word(0);
      } else {
        const uint8_t* r = static_cast<const uint8_t*>(a.d1) + row * a.s1;
        uint32_t w = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (kk * 4 + b < a.k) w |= (uint32_t)r[kk * 4 + b] << (8 * b);
        q[k] = word(w);
      }
    }
  };
  if (a.nseg == 1) load_query(0);

  float first = INFINITY, second = INFINITY;
  int idx = -1;
  for (long long t0 = jb; t0 < je; t0 += IPM_TILE) {
    const int cn = (int)(je - t0 < IPM_TILE ? je - t0 : IPM_TILE);
    for (int seg = 0; seg < a.nseg; ++seg) {
      __syncthreads();   // the tile of the step before has been read
      for (int e = tid; e < IPM_TILE * SEG; e += IPM_THREADS) {
        const int c = e / SEG, kk = seg * SEG + e % SEG;
        word v = word(0);
        if (c < cn) {
          if (L2) {
            if (kk < a.k) v = static_cast<const word*>(a.d2)[(t0 + c) * a.s2 + kk];
          } else {
            const uint8_t* r = static_cast<const uint8_t*>(a.d2) + (t0 + c) * a.s2;
            uint32_t w = 0;
            for (int b = 0; b < 4; ++b)
              if (kk * 4 + b < a.k) w |= (uint32_t)r[kk * 4 + b] << (8 * b);
            v = word(w);
          }
        }
        tile[e] = v;
      }
      if (POL && seg == 0 && tid < IPM_TILE) tpol[tid] = tid < cn ? a.p2[t0 + tid] : 0;
      if (a.nseg > 1) load_query(seg);
      __syncthreads();
      for (int c0 = 0; c0 < cn; c0 += IPM_CG) {
        sum acc[IPM_CG];
#pragma unroll
        for (int u = 0; u < IPM_CG; ++u) acc[u] = seg == 0 ? sum(0) : sum(carry[(c0 + u) * IPM_THREADS + tid]);
        if constexpr (L2) {
          // element pairs (k, k + 1): one packed subtract and one packed multiply (v_pk_add_f32, v_pk_mul_f32 round each half
          // on its own, as the plain forms do), then the two adds of the ONE accumulator in the order of k
#pragma unroll
          for (int k = 0; k < SEG; k += 2) {
            const ipm_f2 qq = {q[k], q[k + 1]};
#pragma unroll
            for (int u = 0; u < IPM_CG; ++u) {
              const ipm_f2 d = qq - *reinterpret_cast<const ipm_f2*>(&tile[(c0 + u) * SEG + k]);
              const ipm_f2 sq = d * d;
              acc[u] += sq.x;
              acc[u] += sq.y;
            }
          }
        } else {
#pragma unroll
          for (int k = 0; k < SEG; ++k) {
#pragma unroll
            for (int u = 0; u < IPM_CG; ++u) acc[u] += __popc(q[k] ^ tile[(c0 + u) * SEG + k]);
          }
        }
        if (seg + 1 < a.nseg) {
#pragma unroll
          for (int u = 0; u < IPM_CG; ++u) carry[(c0 + u) * IPM_THREADS + tid] = float(acc[u]);
        } else {
#pragma unroll
          for (int u = 0; u < IPM_CG; ++u) {
            if (c0 + u >= cn) continue;
            if (POL && tpol[c0 + u] != mypol) continue;
            // the serial loop of Matcher.h:479-485; a NaN or an infinite distance passes neither test
            const float d = float(acc[u]);
            if (d < first) {
              idx = (int)(t0 + c0 + u);
              second = first;
              first = d;
            } else if (d < second) {
              second = d;
            }
          }
        }
      }
    }
  }
  if (live) {
    const long long o = (long long)blockIdx.y * a.n1 + i;
    a.pf[o] = first;
    a.ps[o] = second;
    a.pi[o] = idx;
  }
}

struct ipm_merge_args {
  const float *pf, *ps; const int* pi;
  int nchunks, n1;
  vwgpu_ip_match_params P;
  const float *attr1, *attr2;   // attr1 of this launch's first query
  int32_t* index; float* dist;
  unsigned long long* counters;   // {matched, queries}, or nullptr
};

// ConstraintT::operator()(baseline_ip, test_ip) (Matcher.cc:119-147); b, t: {x, y, scale, orientation}
__device__ bool ipm_constraint(const vwgpu_ip_match_params& P, const float* b, const float* t) {
  if (P.constraint == VWGPU_IP_CONSTRAINT_SCALE_ORIENTATION) {
    const double sr = t[2] / b[2];
    double od = t[3] - b[3];
    const double pi = 3.14159265358979323846;
    if (od < -pi) od += pi * 2;
    else if (od > pi) od -= pi * 2;
    return sr >= P.bounds[0] && sr <= P.bounds[1] && od >= P.bounds[2] && od <= P.bounds[3];
  }
  const double dx = t[0] - b[0];
  const double dy = t[1] - b[1];
  return dx >= P.bounds[0] && dx <= P.bounds[1] && dy >= P.bounds[2] && dy <= P.bounds[3];
}

__global__ __launch_bounds__(IPM_THREADS) void ipm_merge_kernel(ipm_merge_args a) {
  const long long i = (long long)blockIdx.x * IPM_THREADS + threadIdx.x;
  const bool live = i < a.n1;
  int idx = -1;
  if (live) {
    float first = INFINITY, second = INFINITY;
    for (int c = 0; c < a.nchunks; ++c) {   // ascending candidates: a tie keeps the index found first
      const long long o = (long long)c * a.n1 + i;
      const float cf = a.pf[o], cs = a.ps[o];
      if (cf < first) {
        second = first < cs ? first : cs;
        first = cf;
        idx = a.pi[o];
      } else if (cf < second) {
        second = cf;   // cs >= cf
      }
    }
    if (a.P.mode == VWGPU_IP_MODE_SIMPLE) {
      const double first_pick = idx < 0 ? 1e100 : (double)first, second_pick = second == INFINITY ? 1e100 : (double)second;
      if (first_pick > a.P.threshold * second_pick) idx = -1;
    } else if (second == INFINITY) {
      idx = -1;   // num_matches_found < KNN
    } else {
      bool ok = true;
      if (a.P.constraint != VWGPU_IP_CONSTRAINT_NONE) {
        const float *qa = a.attr1 + 4 * i, *na = a.attr2 + 4 * (long long)idx;
        ok = ipm_constraint(a.P, na, qa) && (!a.P.bidirectional || ipm_constraint(a.P, qa, na));
      }
      if (!ok || !((double)first < a.P.threshold * (double)second)) idx = -1;
    }
    a.index[i] = idx;
    if (a.dist) {
      a.dist[2 * i] = first;
      a.dist[2 * i + 1] = second;
    }
  }
  if (a.counters) {
    const unsigned long long m = __popcll(__ballot(live && idx >= 0)), q = __popcll(__ballot(live));
    if ((threadIdx.x & 63) == 0 && q) {
      atomicAdd(&a.counters[0], m);
      atomicAdd(&a.counters[1], q);
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// the kernels that exist: the query registers SEG serve K <= SEG * (elements per register), L2 beyond the last row in segments
using ipm_kernel_t = void (*)(ipm_args);
struct ipm_row { int metric, seg, max_k; ipm_kernel_t plain, pol; };
#define IPM_ROW(METRIC, SEG, MAXK) {METRIC, SEG, MAXK, ipm_chunk_kernel<METRIC, SEG, false>, ipm_chunk_kernel<METRIC, SEG, true>}
const ipm_row ipm_kernels[] = {
  IPM_ROW(VWGPU_IP_METRIC_L2, 32, 32),
  IPM_ROW(VWGPU_IP_METRIC_L2, 64, 64),
  IPM_ROW(VWGPU_IP_METRIC_L2, 128, IPM_MAX_K),
  IPM_ROW(VWGPU_IP_METRIC_HAMMING, 16, 64),
  IPM_ROW(VWGPU_IP_METRIC_HAMMING, 128, IPM_MAX_K),
};
#undef IPM_ROW
const ipm_row* ipm_row_of(int metric, int k) {
  for (const ipm_row& row : ipm_kernels)
    if (row.metric == metric && k <= row.max_k) return &row;
  return nullptr;
}

struct ipm_call {
  const void* d1; int n1; ptrdiff_t s1;
  const void* d2; int n2; ptrdiff_t s2;
  int k;
  const uint8_t *p1, *p2;
  const float *a1, *a2;
  const vwgpu_ip_match_params* params;
  int32_t* index; float* dist; long long* stats;
};

int ipm_check(vwgpu_ctx* ctx, ipm_call& c) {
  const char* name = "ip_match";
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!c.d1 || !c.d2 || !c.params || !c.index) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: null pointer", name);
  if (c.n1 < 1 || c.n2 < 1 || c.k < 1) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: n1, n2 and k must be at least 1", name);
  if (c.s1 == 0) c.s1 = c.k;
  if (c.s2 == 0) c.s2 = c.k;
  if (c.s1 < c.k || c.s2 < c.k) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: row stride smaller than the descriptor length", name);
  const vwgpu_ip_match_params& P = *c.params;
  if (P.metric != VWGPU_IP_METRIC_L2 && P.metric != VWGPU_IP_METRIC_HAMMING)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: metric %d out of range", name, P.metric);
  if (P.mode != VWGPU_IP_MODE_SIMPLE && P.mode != VWGPU_IP_MODE_KNN)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: mode %d out of range", name, P.mode);
  if (P.constraint < VWGPU_IP_CONSTRAINT_NONE || P.constraint > VWGPU_IP_CONSTRAINT_POSITION)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: constraint %d out of range", name, P.constraint);
  if (std::isnan(P.threshold)) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: the threshold is NaN", name);
  if ((c.p1 != nullptr) != (c.p2 != nullptr))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: the two polarity lists go together", name);
  if (P.mode == VWGPU_IP_MODE_KNN && P.constraint != VWGPU_IP_CONSTRAINT_NONE && (!c.a1 || !c.a2))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: a constraint needs attr1 and attr2", name);
  const void* ins[] = {c.d1, c.d2, c.p1, c.p2, c.a1, c.a2};
  for (const void* in : ins)
    if (in && (in == (const void*)c.index || in == (const void*)c.dist))
      return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: an output must not be an input", name);
  if ((const void*)c.index == (const void*)c.dist) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: index and dist are one array", name);
  if (c.k > IPM_MAX_K) return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "%s: descriptors of more than %d elements are not implemented", name, IPM_MAX_K);
  return VWGPU_OK;
}

// all array pointers of `c` are device pointers here; c.stats stays a host pointer
int ipm_run(vwgpu_ctx* ctx, const ipm_call& c) {
  const vwgpu_ip_match_params& P = *c.params;
  const ipm_row* row = ipm_row_of(P.metric, c.k);
  const bool l2 = P.metric == VWGPU_IP_METRIC_L2;
  const bool simple = P.mode == VWGPU_IP_MODE_SIMPLE;
  const bool pol = simple && c.p1;
  const int per = l2 ? row->seg : row->seg * 4;   // descriptor elements per pass over the registers
  const int nseg = (c.k + per - 1) / per;
  const int chunk = ipm_chunk_of(c.n2);
  const int nchunks = (int)(((long long)c.n2 + chunk - 1) / chunk);
  const int qb = std::min(c.n1, IPM_QBATCH);
  const size_t words = (size_t)qb * nchunks;
  int rc = vwgpu_arena_reserve(ctx, &ctx->scratch, words * 12);
  if (rc) return rc;
  float* pf = static_cast<float*>(ctx->scratch.base);
  float* ps = pf + words;
  int* pi = reinterpret_cast<int*>(ps + words);
  unsigned long long* counters = nullptr;
  if (c.stats) {
    if ((rc = vwgpu_arena_reserve(ctx, &ctx->misc, 512))) return rc;
    counters = static_cast<unsigned long long*>(ctx->misc.base);
    VWGPU_HIP(ctx, hipMemsetAsync(counters, 0, 16, ctx->stream));
  }
  const size_t carry = nseg > 1 ? (size_t)IPM_TILE * IPM_THREADS * sizeof(float) : 0;
  const size_t esz = l2 ? 4 : 1;
  for (long long i0 = 0; i0 < c.n1; i0 += qb) {
    const int n = (int)std::min<long long>(qb, c.n1 - i0);
    ipm_args a{};
    a.d1 = static_cast<const char*>(c.d1) + (size_t)i0 * c.s1 * esz; a.s1 = c.s1; a.n1 = n;
    a.d2 = c.d2; a.s2 = c.s2; a.n2 = c.n2;
    a.k = c.k; a.nseg = nseg; a.chunk = chunk;
    a.p1 = pol ? c.p1 + i0 : nullptr; a.p2 = pol ? c.p2 : nullptr;
    a.pf = pf; a.ps = ps; a.pi = pi;
    const dim3 grid((unsigned)((n + IPM_THREADS - 1) / IPM_THREADS), (unsigned)nchunks);
    {
      vwgpu_prof_scope sc(ctx, l2 ? "ip_match_l2" : "ip_match_hamming");
      hipLaunchKernelGGL(pol ? row->pol : row->plain, grid, dim3(IPM_THREADS), carry, ctx->stream, a);
      VWGPU_HIP(ctx, hipGetLastError());
    }
    ipm_merge_args m{};
    m.pf = pf; m.ps = ps; m.pi = pi; m.nchunks = nchunks; m.n1 = n;
    m.P = P;
    if (simple) m.P.constraint = VWGPU_IP_CONSTRAINT_NONE;
    m.attr1 = c.a1 ? c.a1 + 4 * i0 : nullptr; m.attr2 = c.a2;
    m.index = c.index + i0; m.dist = c.dist ? c.dist + 2 * i0 : nullptr;
    m.counters = counters;
    vwgpu_prof_scope sc(ctx, "ip_match_merge");
    hipLaunchKernelGGL(ipm_merge_kernel, dim3((unsigned)((n + IPM_THREADS - 1) / IPM_THREADS)), dim3(IPM_THREADS), 0, ctx->stream, m);
    VWGPU_HIP(ctx, hipGetLastError());
  }
  if (c.stats) {
    unsigned long long got[2] = {0, 0};
    VWGPU_HIP(ctx, hipMemcpyAsync(got, counters, 16, hipMemcpyDeviceToHost, ctx->stream));
    VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    c.stats[0] = (long long)got[0];
    c.stats[1] = (long long)got[1];
  }
  return VWGPU_OK;
}

}  // namespace

// ---- extern "C" entry points (include/vwgpu.h) -------------------------------------------------------------------------

extern "C" {

int vwgpu_ip_match_chunk(int n2) { return ipm_chunk_of(n2 < 1 ? 1 : n2); }

int vwgpu_ip_match_dev(vwgpu_ctx* ctx, const void* d_desc1, int n1, ptrdiff_t stride1, const void* d_desc2, int n2, ptrdiff_t stride2,
                       int k, const uint8_t* d_pol1, const uint8_t* d_pol2, const float* d_attr1, const float* d_attr2,
                       const vwgpu_ip_match_params* params, int32_t* d_index, float* d_dist, long long* stats) {
  ipm_call c{d_desc1, n1, stride1, d_desc2, n2, stride2, k, d_pol1, d_pol2, d_attr1, d_attr2, params, d_index, d_dist, stats};
  int rc = ipm_check(ctx, c);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return ipm_run(ctx, c);
}

int vwgpu_ip_match(vwgpu_ctx* ctx, const void* desc1, int n1, ptrdiff_t stride1, const void* desc2, int n2, ptrdiff_t stride2, int k,
                   const uint8_t* pol1, const uint8_t* pol2, const float* attr1, const float* attr2,
                   const vwgpu_ip_match_params* params, int32_t* index, float* dist, long long* stats) {
  ipm_call c{desc1, n1, stride1, desc2, n2, stride2, k, pol1, pol2, attr1, attr2, params, index, dist, stats};
  int rc = ipm_check(ctx, c);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  const size_t esz = params->metric == VWGPU_IP_METRIC_L2 ? 4 : 1;
  vwgpu_stage st(ctx);
  const int q1 = st.add(desc1, k, n1, esz, c.s1, VWGPU_STAGE_IN), q2 = st.add(desc2, k, n2, esz, c.s2, VWGPU_STAGE_IN),
            o1 = st.add(pol1, n1, 1, 1, n1, VWGPU_STAGE_IN), o2 = st.add(pol2, n2, 1, 1, n2, VWGPU_STAGE_IN),
            a1 = st.add(attr1, 4, n1, 4, 4, VWGPU_STAGE_IN), a2 = st.add(attr2, 4, n2, 4, 4, VWGPU_STAGE_IN),
            xi = st.add(index, n1, 1, 4, n1, VWGPU_STAGE_OUT), xd = st.add(dist, 2, n1, 4, 2, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  ipm_call d = c;
  d.d1 = st.dev<char>(q1); d.s1 = k;
  d.d2 = st.dev<char>(q2); d.s2 = k;
  d.p1 = st.dev<uint8_t>(o1); d.p2 = st.dev<uint8_t>(o2);
  d.a1 = st.dev<float>(a1); d.a2 = st.dev<float>(a2);
  d.index = st.dev<int32_t>(xi); d.dist = st.dev<float>(xd);
  if ((rc = ipm_run(ctx, d))) return rc;
  return st.finish();
}

}  // extern "C"
