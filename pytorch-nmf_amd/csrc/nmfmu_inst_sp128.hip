// Instantiation of the software-pipelined one-wave-per-SIMD fused MU kernel with 64 owner rows per wave (padded rank 128,
// beta = 1, fp16), nmfmu_sp128.h: the shipped placement of the ratio stage.  NMFMU_SP128_RB = reciprocals of tile t+1 that
// run in phase B(t) (0, 16, 32, 48 or 64; sweep builds: make VARIANT=_rb32 EXTRA=-DNMFMU_SP128_RB=32 VUNITS=nmfmu_inst_sp128).
// The RB = 0 arm of the A/B lives in nmfmu_inst_sp128_rb0.hip: exactly ONE kernel instance per unit.
#include "nmfmu_sp128.h"

#ifndef NMFMU_SP128_RB
#define NMFMU_SP128_RB 48
#endif

namespace nmfmu {

bool sp128_available(int r_pad, int opt, int mode) { return r_pad == 128 && opt == kOpF16 && mode == kModeMU; }

int launch_sp128(int r_pad, int opt, const FusedArgs& a, int grid, hipStream_t s) {
  if (r_pad == 128 && opt == kOpF16) return launch_sp128_one<kOpF16, NMFMU_SP128_RB>(a, grid, s);
  return -2;
}

}  // namespace nmfmu
