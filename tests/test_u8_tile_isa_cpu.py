"""The loads that csrc/u8_tile.h emits for gfx950, read off the compiler's assembly (no GPU needed; skipped without hipcc).

The main part of a tile is one 16-byte load per row and lane (`global_load_dwordx4` through a packed, 4-byte aligned struct of four
floats), for aligned and unaligned images alike.  An earlier form chose per row between a float4 load and four scalar loads on a run-time
flag, and the compiler merged the two arms into four `global_load_dword` with selected addresses in every row but the last.  This test
compiles a stand-alone translation unit (a few seconds; not bm_sad_u8.hip) with two probe kernels per tile height:
  probe_main<NROWS>  stage_u8_main_issue + stage_u8_main_finish only: exactly NROWS wide loads, no single-dword load;
  probe_rows<NROWS>  stage_u8_rows: at least NROWS wide loads, and the only single-dword loads are the four pixels of patch_right_edge's
                     scalar tail.
NROWS = 22 and 14 are the 7x7 tiles of 16 and 8 rows."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NROWS = (22, 14)

PROBE = r"""
#include "u8_tile.h"
using namespace vwgpu_u8;
template <int NR>
__global__ void __launch_bounds__(256) probe_rows(const float* img, ptrdiff_t stride, int w, int h, int x0, int y0, int ndw, int pitch,
                                                  u32* out, int* flag) {
  extern __shared__ u32 lds[];
  u32 acc = 0;
  stage_u8_rows<NR>(img, stride, w, h, x0, y0, ndw, pitch, lds, threadIdx.x, 256, acc);
  __syncthreads();
  for (int i = threadIdx.x; i < NR * pitch; i += 256) out[i] = lds[i];
  if (acc) *flag = 1;
}
template <int NR>
__global__ void __launch_bounds__(256) probe_main(const float* img, ptrdiff_t stride, int w, int h, int x0, int y0, int ndw, int pitch,
                                                  u32* out, int* flag) {
  extern __shared__ u32 lds[];
  u32 acc = 0;
  U8MainLoads<NR> ld;
  stage_u8_main_issue<NR>(img, stride, w, h, x0, y0, ndw, threadIdx.x, ld);
  stage_u8_main_finish<NR>(w, h, x0, y0, ndw, pitch, lds, threadIdx.x, ld, acc);
  __syncthreads();
  for (int i = threadIdx.x; i < NR * pitch; i += 256) out[i] = lds[i];
  if (acc) *flag = 1;
}
#define PROBES(NR) \
  template __global__ void probe_rows<NR>(const float*, ptrdiff_t, int, int, int, int, int, int, u32*, int*); \
  template __global__ void probe_main<NR>(const float*, ptrdiff_t, int, int, int, int, int, int, u32*, int*);
PROBES(22)
PROBES(14)
"""


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{(probe name, NROWS): list of instruction mnemonics} of the probe translation unit."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc is not installed")
    d = tmp_path_factory.mktemp("u8_tile_isa")
    src, asm = str(d / "probe.hip"), str(d / "probe.s")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S",
                           "-I" + os.path.join(ROOT, "visionworkbench_amd", "csrc"), src, "-o", asm], stderr=subprocess.DEVNULL)
    out, cur = {}, None
    for line in open(asm):
        m = re.match(r"^_Z\d+(probe_rows|probe_main)ILi(\d+)E\S*:", line)
        if m:
            cur = out.setdefault((m.group(1), int(m.group(2))), [])
            continue
        if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            cur = None
        if cur is not None and line.startswith("\t") and not line.startswith(("\t;", "\t.")):
            cur.append(line.split()[0])
    assert sorted(out) == sorted((p, n) for p in ("probe_main", "probe_rows") for n in NROWS), sorted(out)
    return out


def _loads(ops):
    wide = sum(op == "global_load_dwordx4" for op in ops)
    single = sum(op == "global_load_dword" for op in ops)
    other = sum(op.startswith(("global_load", "buffer_load", "flat_load")) for op in ops) - wide - single
    return wide, single, other


@pytest.mark.parametrize("nrows", NROWS)
def test_main_part_is_one_wide_load_per_row(kernels, nrows):
    wide, single, other = _loads(kernels[("probe_main", nrows)])
    assert (wide, single, other) == (nrows, 0, 0), "main part of %d rows: %d dwordx4, %d dword, %d other loads" % (nrows, wide, single, other)


@pytest.mark.parametrize("nrows", NROWS)
def test_whole_tile_has_scalar_loads_in_the_edge_patch_only(kernels, nrows):
    """stage_u8_rows: the main part (NROWS) and the remainder columns (4 in flight) load 16 bytes each; what is left are the four
    pixels of the straddling group in patch_right_edge."""
    wide, single, other = _loads(kernels[("probe_rows", nrows)])
    assert wide >= nrows + 4, "%d rows: %d dwordx4" % (nrows, wide)
    assert single <= 4 and other == 0, "%d rows: %d dword and %d other loads outside the wide ones" % (nrows, single, other)
