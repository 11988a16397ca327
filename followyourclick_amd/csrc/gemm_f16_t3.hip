// f16 instantiations of the 3-tap convolution along the frame axis (FYC_GEMM_CONV_T3: TemporalConvBlock's Conv3d (3,1,1)).
#include "gemm_kernel.h"
namespace fycg {
int run_f16_t3(const GemmP& p, int batch, int cfg, int ns, hipStream_t st) {
  return dispatch_ns<f16_t, FYC_GEMM_CONV_T3, FYC_EPI_LINEAR>(ns, cfg, p, batch, st);
}
}  // namespace fycg
