// Host entry of the fused attention: argument validation and dispatch (kernel template: attention_kernel.h;
// instantiations: attention_small.hip, attention_medium.hip, attention_large.hip; f32 tensors: attention_f32x3.hip; causal mask and head dims above 160, every
// dtype: attention_wide.h and its three instantiation files).
#include "attention_kernel.h"
#include "attention_wide.h"
#include "split_bf16.h"      // FYC_REQUIRE_F32_PRODUCTS

// both entries: fyc_attention is causal = 0; fyc_attention_masked has checked its own pointer
static int attention(const fyc_attn_args* a, int causal, void* stream) {
  FYC_REQUIRE(a && a->q && a->k && a->vt && a->o, "fyc_attention: null pointer");
  FYC_REQUIRE_F32_PRODUCTS("fyc_attention", a);
  FYC_REQUIRE(a->dtype != FYC_F32 || a->f32_products == FYC_PRODUCTS_SPLIT_BF16,
              "fyc_attention: dtype FYC_F32 needs f32_products = FYC_PRODUCTS_SPLIT_BF16 (there is no exact fused f32 kernel: the exact f32 mode uses materialised attention)");
  FYC_REQUIRE(a->dtype == FYC_F32 || a->dtype == FYC_BF16 || a->dtype == FYC_F16, "fyc_attention: bad dtype %d", a->dtype);
  FYC_REQUIRE(causal == 0 || causal == 1, "fyc_attention_masked: causal=%d (0 = off, 1 = key j counts for query i iff j <= i)", causal);
  FYC_REQUIRE(causal == 0 || (a->n_q == a->n_k && a->q_batch_mod == 0), "fyc_attention_masked: causal=1 needs n_q == n_k (%d, %d) and q_batch_mod == 0 (%d)", a->n_q, a->n_k, a->q_batch_mod);
  FYC_REQUIRE(a->d <= 160 || (a->d % 32 == 0 && a->d <= 512), "fyc_attention: head dim d=%d (above 160: a multiple of 32, <= 512)", a->d);
  FYC_REQUIRE(g_fyc_zero_page != nullptr, "fyc_attention: fyc_init() not called");
  FYC_REQUIRE(a->batch > 0 && a->heads > 0 && a->n_q > 0 && a->n_k > 0, "fyc_attention: bad sizes");
  FYC_REQUIRE(a->d % 8 == 0 && a->d >= 8 && a->d <= 512, "fyc_attention: head dim %d (multiple of 8 up to 160, multiple of 32 up to 512)", a->d);
  FYC_REQUIRE(a->ldvt % 8 == 0 && a->ldvt >= a->n_k, "fyc_attention: ldvt=%d must be a multiple of 8 and >= n_k", a->ldvt);
  FYC_REQUIRE(a->ldo % 4 == 0, "fyc_attention: ldo must be a multiple of 4");
  FYC_REQUIRE(a->kv_batch_div >= 1, "fyc_attention: kv_batch_div");
  FYC_REQUIRE(a->q_batch_mod >= 0 && a->q_batch_mod <= a->batch, "fyc_attention: q_batch_mod %d (0 .. batch)", a->q_batch_mod);
  fyca::AttnP p;      // one fill for every dtype: the kernels cast the element pointers to their type
  p.q = (const bf16_t*)a->q; p.k = (const bf16_t*)a->k; p.vt = (const bf16_t*)a->vt; p.o = (bf16_t*)a->o;
  p.batch = a->batch; p.heads = a->heads; p.n_q = a->n_q; p.n_k = a->n_k; p.d = a->d; p.ldo = a->ldo; p.ldvt = a->ldvt;
  p.kv_batch_div = a->kv_batch_div; p.o_accumulate = a->o_accumulate; p.q_batch_mod = a->q_batch_mod;
  p.sl2e = a->scale * 1.44269504088896340736f; p.o_scale = a->o_scale;
  p.nqb = 0; p.zero = (const char*)g_fyc_zero_page;
  hipStream_t st = (hipStream_t)stream;
  if (causal || a->d > 160) {      // attention_wide.h; causal = 0 with d <= 160 takes the launches below, unchanged
    if (a->dtype == FYC_F32) return fyca::run_wide_f32x3(p, causal != 0, st);
    return a->dtype == FYC_F16 ? fyca::run_wide_f16(p, causal != 0, st) : fyca::run_wide_bf16(p, causal != 0, st);
  }
  if (a->dtype == FYC_F32) return fyca::run_f32x3(p, st);      // attention_f32x3.hip (its QT rule is written there, beside the kernel's budgets)
  // Queries per wave = 16 * QT.  More queries amortise the K / V^T fragment reads over more MFMAs but cost registers: at d = 40
  // QT = 4 needs 170 VGPRs (2 waves / SIMD), QT = 3 needs 140 (3 waves / SIMD).  Large problems take QT = 3 (measured,
  // profiles/r02_attention_variants.txt); small ones QT = 2 so that the grid still fills the chip.  tuning key 3 forces QT.
  const long long wg3 = (long long)a->batch * a->heads * ((a->n_q + 191) / 192);
  // d = 64 (the SD-2.1 head layout) was measured on its own: QT = 3 takes 0.81 - 0.85 of QT = 2's time at n_q >= 2304 and is level with it at 1024
  // (profiles/sd21_forward.txt); the other head dims above 48 keep QT = 2 (3 tiles no longer fit 2 waves / SIMD, and nothing says otherwise)
  int qt = (a->n_q >= 1024 && wg3 >= 512 && (a->d <= 48 || a->d == 64)) ? 3 : 2;
  if (g_fyc_tuning[FYC_TUNE_ATTN_VARIANT] >= 2 && g_fyc_tuning[FYC_TUNE_ATTN_VARIANT] <= 4 && (a->d <= 80 || g_fyc_tuning[FYC_TUNE_ATTN_VARIANT] == 2)) qt = g_fyc_tuning[FYC_TUNE_ATTN_VARIANT];
  if (a->dtype == FYC_F16) {
    if (a->d <= 48) return fyca::run_small<f16_t>(p, qt, st);
    if (a->d <= 96) return fyca::run_medium<f16_t>(p, qt, st);
    return fyca::run_large<f16_t>(p, st);
  }
  if (a->d <= 48) return fyca::run_small<bf16_t>(p, qt, st);
  if (a->d <= 96) return fyca::run_medium<bf16_t>(p, qt, st);
  return fyca::run_large<bf16_t>(p, st);
}

extern "C" int fyc_attention(const fyc_attn_args* a, void* stream) { return attention(a, 0, stream); }

// (version 308) the same launch with the causal mask: fyc_attn_args stays as ABI 307 left it, the flag travels in a struct of its own around it
extern "C" int fyc_attention_masked(const fyc_attn_mask_args* a, void* stream) {
  FYC_REQUIRE(a, "fyc_attention_masked: null pointer");
  return attention(&a->attn, a->causal, stream);
}
