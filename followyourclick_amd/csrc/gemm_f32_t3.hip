// f32 parity-mode instantiations of the 3-tap convolution along the frame axis (FYC_GEMM_CONV_T3), two tile shapes like gemm_f32.hip.
#include "gemm_kernel.h"
namespace fycg {
int run_f32_t3(const GemmP& p, int batch, int cfg, hipStream_t st) {
  if (cfg & CFG_F32X3) return run_f32x3_t3(p, batch, cfg & ~CFG_F32X3, st);      // split-bf16 products: gemm_f32x3_t3.hip
  return dispatch_cfg<float, FYC_GEMM_CONV_T3, FYC_EPI_LINEAR, false>(cfg, 2, p, batch, st);
}
}  // namespace fycg
