// f32 storage with split-bf16 products: the 3-tap convolution along the frame axis (FYC_GEMM_CONV_T3), gemm_f32_t3.hip with the f32x3 product rule.
#include "gemm_kernel.h"
namespace fycg {
int run_f32x3_t3(const GemmP& p, int batch, int cfg, hipStream_t st) {
  return dispatch_cfg<float, FYC_GEMM_CONV_T3, FYC_EPI_LINEAR, false, f32x3_t>(cfg, 2, p, batch, st);
}
}  // namespace fycg
