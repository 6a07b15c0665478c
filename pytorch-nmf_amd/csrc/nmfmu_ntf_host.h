// Host code the two dense NTF tiles share (nmfmu_ntf.hip: 128 owner rows per workgroup; nmfmu_ntf_short.hip: 32): the limits,
// a half-step's view of the tensor, the argument checks of the entries and the launch of the finishing kernel.  No device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nmfmu.h"
#include "nmfmu_mu_terms.h"
#include "nmfmu_wmu_tile.h"

namespace nmfmu {

constexpr int kNtfTargetWgs = 512;          // two workgroups on each of the 256 CUs
constexpr int kNtfMaxContraction = 1 << 30; // flat steps are ints; parts * part_len stays below 2^31
constexpr int kNtfMaxParts = 65535;         // the parts are grid.z

// a half-step's view of the tensor: owner rows, the two contraction dimensions, the walk and its strides
struct NtfMode {
  int rows, nA, nB, outer;
  int64_t sO, sA;
};

inline NtfMode ntf_mode(int I, int J, int K, int mode) {
  const int64_t JK = (int64_t)J * K;
  if (mode == 0) return NtfMode{I, J, K, 0, JK, K};
  if (mode == 1) return NtfMode{J, I, K, 0, K, JK};
  return NtfMode{K, I, J, 1, 1, K};
}

// NMFMU_OK or the answer the entries give before any device work.  split(rows, contraction, r_pad, nsplit): the tile's parts
inline int ntf_check(const void* V, int I, int J, int K, int mode, const void* owner, const void* pa, const void* pb, int rank,
                     int r_pad, bool has_r_pad, int nsplit, int (*split)(int, int, int, int)) {
  if (const int rc = wmu_check(pb && I > 0 && J > 0 && K > 0 && mode >= 0 && mode <= 2, V, owner, pa, rank, r_pad, has_r_pad))
    return rc;
  const NtfMode md = ntf_mode(I, J, K, mode);
  if ((int64_t)md.nA * md.nB > kNtfMaxContraction) return NMFMU_ERR_UNSUPPORTED;
  if (has_r_pad && split(md.rows, md.nA * md.nB, r_pad, nsplit) > kNtfMaxParts) return NMFMU_ERR_UNSUPPORTED;   // a forced split
  return NMFMU_OK;
}

// ntf_finish_kernel (nmfmu_ntf.hip) on the slab of `parts` parts: the terms to num / den, or the update in place on the owner
void ntf_finish_launch(int fblocks, const float* ws, int parts, int rows, int rank, int r_pad, float* owner, float* num,
                       float* den, int step, MaskedApply ap, hipStream_t st);

}  // namespace nmfmu
