// The per-entry arithmetic of the exact-fp32 multiplicative updates that work on the fp32 masters directly: the two seeds of
// nmf.py:61-74 at one entry, the update of nmf.py:78-92 on one element, and the s-dependent term of metrics.beta_div.
// Shared by the missing-data kernels (nmfmu_sparse_masked.hip: one stored entry) and the weighted dense kernels
// (nmfmu_wmu.hip: one entry of the target tile).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/nmfmu.h"
#include "nmfmu_fused.h"

namespace nmfmu {

// (g_neg, g_pos) of one entry; s is the plain dot product
template <int KIND>
__device__ __forceinline__ void masked_g(float v, float s, float beta, float& gn, float& gp) {
  if constexpr (KIND == NMFMU_BETA_EUC) {
    gn = v, gp = s;                                   // nmf.py:62-63
  } else if constexpr (KIND == NMFMU_BETA_KL) {
    gn = v / (s + kEps), gp = 1.f;                    // nmf.py:65; the ones seed
  } else if constexpr (KIND == NMFMU_BETA_IS) {
    const float r = 1.f / (s + kEps);                 // nmf.py:68-70
    gp = r, gn = r * r * v;
  } else {
    const float se = s + kEps;                        // nmf.py:72-74
    const float p2 = exp2f((beta - 2.f) * log2f(se));
    gn = p2 * v, gp = p2 * se;
  }
}

struct MaskedApply {
  float l1, l2, gamma;
};

// nmf.py:78-92 on one element
__device__ __forceinline__ float masked_apply(float f, float num, float den, const MaskedApply& ap) {
  const float neg = fmaxf(num, 0.f) + kEps;
  float pos = fmaxf(den, 0.f) + kEps;
  if (ap.l1 > 0.f) pos += ap.l1;
  if (ap.l2 > 0.f) pos += ap.l2 * f;
  float mult = neg / pos;
  if (ap.gamma != 1.f) mult = powf(mult, ap.gamma);
  return f * mult;
}

// the s-dependent term of metrics.beta_div at one entry, in double (see nmfmu_sp_masked_loss in include/nmfmu.h)
template <int KIND>
__device__ __forceinline__ double masked_loss_term(float v, float s, float beta) {
  if constexpr (KIND == NMFMU_BETA_EUC) {
    const float d = s - v;                            // metrics.py:39
    return (double)d * (double)d;
  } else if constexpr (KIND == NMFMU_BETA_KL) {
    return (double)s - (double)(v * logf(s + kEps));  // metrics.py:22
  } else if constexpr (KIND == NMFMU_BETA_IS) {
    const float se = s + kEps;                        // metrics.py:56-57
    return (double)((v + kEps) / se) + (double)logf(se);
  } else {
    const float se = s + kEps;                        // metrics.py:85-95
    const float vt = beta < 0.f ? v + kEps : v;
    const float pb1 = exp2f((beta - 1.f) * log2f(se));
    return (double)pb1 * ((double)(beta - 1.f) * (double)se - (double)beta * (double)vt);
  }
}

}  // namespace nmfmu
