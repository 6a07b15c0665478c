// Host launcher for kernels that use dynamic LDS: shared by the fused MU kernels (nmfmu_fused.h, nmfmu_pp.h, nmfmu_sp.h,
// nmfmu_sp2.h) and the GEMM engine (nmfmu_gemm.h).  Self-contained host code.
#pragma once
#include <hip/hip_runtime.h>

namespace nmfmu {

// Per-device "attribute set" memo (one host thread may drive several devices)
inline bool* attr_flag(bool (&flags)[64]) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  return &flags[dev];
}

// Launches KERN with LDS_BYTES of dynamic LDS.  The dynamic-LDS attribute is per device: a single-process multi-device
// host sets it once on each.  KERN is a template argument, so the memo is one static per kernel instantiation.
template <auto KERN, int THREADS, int LDS_BYTES, class Args>
int launch_with_dynamic_lds(dim3 grid, hipStream_t s, const Args& a) {
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
  static bool done[64] = {};
  bool* flag = attr_flag(done);
  if (!*flag) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    if (e != hipSuccess) return (int)e;
    *flag = true;
  }
  hipLaunchKernelGGL(KERN, grid, dim3(THREADS), LDS_BYTES, s, a);
  return (int)hipGetLastError();
}

}  // namespace nmfmu
