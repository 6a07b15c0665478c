// The RB = 0 schedule of nmfmu_sp128.h (the whole ratio stage of tile t in phase A(t), five instructions per MFMA gap) as a
// second instance: NMFMU_STAGE_DMA_SP128_RB0, the other arm of an A/B against the shipped placement in one library.
#include "nmfmu_sp128.h"

namespace nmfmu {

int launch_sp128_rb0(int r_pad, int opt, const FusedArgs& a, int grid, hipStream_t s) {
  if (r_pad == 128 && opt == kOpF16) return launch_sp128_one<kOpF16, 0>(a, grid, s);
  return -2;
}

}  // namespace nmfmu
