// bf16 plain GEMM with a pointwise activation in the epilogue (conditioning encoders: CLIP MLPs, Resampler feed-forward).
// Off the denoising hot path, so only three tile shapes are built.
#include "gemm_kernel.h"
namespace fycg {
int run_bf16_act(const GemmP& p, int batch, int cfg, hipStream_t st) {
  if (!p.wide) return dispatch_cfg<bf16_t, FYC_GEMM_PLAIN, EPI_LINEAR_ACT, false>(cfg, 2, p, batch, st);
  switch (gemm_executed_cfg(GEMM_FAM_ACT, true, cfg, p.N)) {      // the planned tile folded onto the three (written out: the kernels keep their order in the object)
    case 6: return launch<bf16_t, 6, FYC_GEMM_PLAIN, EPI_LINEAR_ACT, 2, true>(p, batch, st);
    case 1: return launch<bf16_t, 1, FYC_GEMM_PLAIN, EPI_LINEAR_ACT, 2, true>(p, batch, st);
    case 2: return launch<bf16_t, 2, FYC_GEMM_PLAIN, EPI_LINEAR_ACT, 2, true>(p, batch, st);
  }
  FYC_FAIL(-2, "fyc_gemm: tile config %d not built for an activation", cfg);
}
}  // namespace fycg
