// f32 storage with split-bf16 products (fyc_gemm_args::f32_products = FYC_PRODUCTS_SPLIT_BF16): the instantiations of gemm_f32.hip with the
// f32x3 product rule (gemm_kernel.h::Mma<f32x3_t>, three v_mfma_f32_16x16x32_bf16 per block and K tile).  Same tiles, ring and epilogues.
#include "gemm_kernel.h"
namespace fycg {
template <int MODE, int EPI>
static int run_tile(const GemmP& p, int batch, int cfg, hipStream_t st) {
  return dispatch_cfg<float, MODE, EPI, false, f32x3_t>(cfg, 2, p, batch, st);
}
int run_f32x3(const GemmP& p, int batch, int cfg, hipStream_t st) {
  if (p.mode == FYC_GEMM_CONV3X3) return run_tile<FYC_GEMM_CONV3X3, FYC_EPI_LINEAR>(p, batch, cfg, st);
  if (p.mode == FYC_GEMM_CONV3X3_UP2) return run_tile<FYC_GEMM_CONV3X3_UP2, FYC_EPI_LINEAR>(p, batch, cfg, st);
  if (p.epilogue == FYC_EPI_LINEAR && p.act != FYC_ACT_NONE) return run_tile<FYC_GEMM_PLAIN, EPI_LINEAR_ACT>(p, batch, cfg, st);
  switch (p.epilogue) {
    case FYC_EPI_LINEAR: return run_tile<FYC_GEMM_PLAIN, FYC_EPI_LINEAR>(p, batch, cfg, st);
    case FYC_EPI_GEGLU: return run_tile<FYC_GEMM_PLAIN, FYC_EPI_GEGLU>(p, batch, cfg, st);
    case FYC_EPI_HEADS: return run_tile<FYC_GEMM_PLAIN, FYC_EPI_HEADS>(p, batch, cfg, st);
  }
  FYC_FAIL(-2, "fyc_gemm: bad epilogue %d", p.epilogue);
}
}  // namespace fycg
