// f16 instantiations of the four-phase 2x2 form of the nearest-2x upsample + 3x3 convolution (GEMM_MODE_UP_PHASES; host entry: conv_up_phases.hip).
#include "gemm_kernel.h"
namespace fycg {
int run_f16_up_phases(const GemmP& p, int cfg, int ns, hipStream_t st) {
  return dispatch_cfg<f16_t, GEMM_MODE_UP_PHASES, FYC_EPI_LINEAR, true>(cfg, ns, p, 1, st);      // the packed 16-byte LINEAR epilogue only
}
}  // namespace fycg
