// What the two dense MTTKRP kernels share (nmfmu_ntf_mttkrp.hip: exact fp32; nmfmu_ntf_mttkrp_x3.hip: split bf16): the kernel
// arguments, the slice table of a run, the split of the contraction into parts of whole stages, the checks of the two entries
// and the launch of the kernel that adds the slab's parts.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/nmfmu.h"
#include "nmfmu_ntf_host.h"
#include "nmfmu_wmu_tile.h"

namespace nmfmu {

struct MkArgs {
  const float* V;
  int64_t sO, sA;
  int rows, nB, C;
  const float *Pa, *Pb;
  int rank, part_len;
  float* out;      // + part * pstride: the part's plane [rows][RP]
  int64_t pstride;
};

// the slice table of the 32-step run at wc: lane l & 31 holds a = (wc + l) / nB (0 past the part).  Called by every lane.
__device__ __forceinline__ int mk_slices(int wc, int cend, int nB, int lane) {
  const int c = wc + (lane & 31);
  return c < cend ? c / nB : 0;
}

// ---- the split: parts of whole stages ------------------------------------------------------------------------------------------
inline int mk_stage(int tile) { return tile ? 4 * kWmBK : kWmBK; }
inline int mk_stages(int contraction, int tile) { return (contraction + mk_stage(tile) - 1) / mk_stage(tile); }
// nsplit == 0: the parts the fused tile of this arrangement would take; no empty part, only the last one may be short
inline int mk_split(int rows, int contraction, int r_pad, int nsplit, int tile) {
  const int want = nsplit > 0 ? nsplit
                              : (tile ? nmfmu_ntf_short_nsplit(rows, contraction, r_pad) : nmfmu_ntf_nsplit(rows, contraction, r_pad));
  const int stages = mk_stages(contraction, tile);
  const int n = std::max(1, std::min(want, stages));
  const int per = (stages + n - 1) / n;
  return (stages + per - 1) / per;
}
inline int mk_part_len(int contraction, int parts, int tile) {
  return (mk_stages(contraction, tile) + parts - 1) / parts * mk_stage(tile);
}

// a checked call: the kernel's arguments, its grid (row tiles, 1, parts) and the walk
struct MkPlan {
  MkArgs a;
  dim3 grid;
  int parts, outer;
};

// NMFMU_OK and the plan, or the answer nmfmu_ntf_mttkrp and nmfmu_ntf_mttkrp_x3 give before any device work
inline int mk_plan(const float* V, int I, int J, int K, int mode, const float* pa, const float* pb, int rank, int r_pad, int nsplit,
                   int tile, float* ws, float* num, MkPlan* pl) {
  if (!ws || !num || nsplit < 0 || tile < 0 || tile > 1) return NMFMU_ERR_ARG;
  if (const int rc = wmu_check(pb && I > 0 && J > 0 && K > 0 && mode >= 0 && mode <= 2, V, num, pa, rank, r_pad, true)) return rc;
  const NtfMode md = ntf_mode(I, J, K, mode);
  if ((int64_t)md.nA * md.nB > kNtfMaxContraction) return NMFMU_ERR_UNSUPPORTED;
  const int rows = md.rows, contraction = md.nA * md.nB;
  const int parts = mk_split(rows, contraction, r_pad, nsplit, tile);
  if (parts > kNtfMaxParts) return NMFMU_ERR_UNSUPPORTED;      // a forced split
  pl->a = MkArgs{V, md.sO, md.sA, rows, md.nB, contraction, pa, pb, rank, mk_part_len(contraction, parts, tile),
                 parts == 1 ? num : ws, (int64_t)rows * r_pad};
  pl->grid = dim3((rows + (tile ? 32 : kWmRows) - 1) / (tile ? 32 : kWmRows), 1, parts);
  pl->parts = parts, pl->outer = md.outer;
  return NMFMU_OK;
}

// mk_finish_kernel (nmfmu_ntf_mttkrp.hip) on the slab: num = the parts' planes added in part order.  parts > 1.
void mk_finish_launch(const float* ws, int parts, int64_t plane, float* num, hipStream_t st);

}  // namespace nmfmu
