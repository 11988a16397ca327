// What the fused attention kernels share - the 16-bit template of attention_kernel.h and the f32 split-products kernel of attention_f32x3.hip: the
// parameter block fyc_attention fills once for every dtype, the 16-byte LDS-DMA, the counted wait, and the threshold of the lagging running maximum.
#pragma once
#include "fyc_common.h"

namespace fyca {

struct AttnP {
  const bf16_t* q; const bf16_t* k; const bf16_t* vt; bf16_t* o;   // elements of the kernel's type (bf16, f16: same pointer arithmetic; f32: cast where the kernel starts)
  int batch, heads, n_q, n_k, d, ldo, ldvt, kv_batch_div, o_accumulate;
  int q_batch_mod;       // > 0: the q of batch element b is read from b % q_batch_mod (K / V / O stay per b)
  float sl2e, o_scale;   // f32(scale * log2(e))
  int nqb;               // query blocks per (b,h)
  const char* zero;
};

__device__ __forceinline__ void glds16(const void* gsrc, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

constexpr float RESCALE_THR = 6.0f;   // log2 units: probabilities stay <= 64 between moves of the running max

// attention_f32x3.hip: FYC_F32 tensors (f32_products = FYC_PRODUCTS_SPLIT_BF16); fyc_attention has checked the arguments.  The launchers of the 16-bit
// instantiations, run_small / run_medium / run_large, are declared beside their template (attention_kernel.h).
int run_f32x3(const AttnP& p, hipStream_t st);

}  // namespace fyca
