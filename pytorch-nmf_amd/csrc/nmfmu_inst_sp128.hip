// Instantiation of the software-pipelined one-wave-per-SIMD fused MU kernel with 64 owner rows per wave (padded rank 128,
// beta = 1, fp16), nmfmu_sp128.h.
#include "nmfmu_sp128.h"

namespace nmfmu {

bool sp128_available(int r_pad, int opt, int mode) { return r_pad == 128 && opt == kOpF16 && mode == kModeMU; }

int launch_sp128(int r_pad, int opt, const FusedArgs& a, int grid, hipStream_t s) {
  if (r_pad == 128 && opt == kOpF16) return launch_sp128_one<kOpF16>(a, grid, s);
  return -2;
}

}  // namespace nmfmu
