// The f32x3 tier's operand split (f32 storage, every product from three bf16 matrix instructions; f32_products = FYC_PRODUCTS_SPLIT_BF16, include/fyc.h)
// and the host-side refusals of that field.  The rule has this one home for the kernels outside the GEMM family (attention_f32x3.hip,
// temporal_attn_f32x3.hip):
//   hi = RNE_bf16(x), lo = RNE_bf16(x - hi) - round to nearest even both times, and x - hi is exact in f32;
//   c += lo(w) hi(a) + hi(w) lo(a) + hi(w) hi(a) - the two small terms meet the running sum first, lo(w) lo(a) is dropped.
// The per-product bound that follows from it (2^-17 per remainder, 2^-16 for the dropped product) is derived in tests/f32x3_spec.py.
// The one other statement of the rule is gemm_kernel.h::Mma<f32x3_t> (split, mma), kept on purpose: the GEMM family's sources and the headers they
// include are the identity of the HBM-traffic profile (_build.py::family_digest, profiles/r09_hbm_traffic.json), so that family includes nothing from
// here until the profile is taken again.  A change of the rule is an edit here, one there and one in tests/f32x3_spec.py.
#pragma once
#include "row_panel.h"

namespace sb {

struct Split { bf16x8 hi, lo; };
// 8 f32 -> hi and lo bf16x8 (x - hi is exact in f32)
__device__ __forceinline__ Split split8(f32x4 x0, f32x4 x1) {
  u32x4 h, l;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float a = e < 2 ? x0[2 * e] : x1[2 * e - 4], b = e < 2 ? x0[2 * e + 1] : x1[2 * e - 3];
    h[e] = pack_bf16x2(a, b);
    l[e] = pack_bf16x2(a - __uint_as_float(h[e] << 16), b - __uint_as_float(h[e] & 0xffff0000u));
  }
  return {__builtin_bit_cast(bf16x8, h), __builtin_bit_cast(bf16x8, l)};
}
// the same, and sum += hi(x) + lo(x) over the 8 values (each sum is an f32 number: lo is a rounding of the f32 number x - hi)
__device__ __forceinline__ Split split8_sum(f32x4 x0, f32x4 x1, float& sum) {
  const Split s = split8(x0, x1);
  const u32x4 h = __builtin_bit_cast(u32x4, s.hi), l = __builtin_bit_cast(u32x4, s.lo);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    sum += __uint_as_float(h[e] << 16) + __uint_as_float(l[e] << 16);
    sum += __uint_as_float(h[e] & 0xffff0000u) + __uint_as_float(l[e] & 0xffff0000u);
  }
  return s;
}
// c += hi(w) hi(a) + hi(w) lo(a) + lo(w) hi(a), the small terms first
__device__ __forceinline__ f32x4 mma3(const Split& w, const Split& a, f32x4 c) {
  c = rp::mfma(w.lo, a.hi, c);
  c = rp::mfma(w.hi, a.lo, c);
  return rp::mfma(w.hi, a.hi, c);
}

}  // namespace sb

// What fyc_attention and fyc_temporal_attention refuse about their f32_products field: a value other than the two rules, and the split rule on 16-bit
// tensors.  (fyc_gemm states the same pair itself, gemm.hip: see above.)
#define FYC_REQUIRE_F32_PRODUCTS(name, a)                                                                                                        \
  do {                                                                                                                                           \
    FYC_REQUIRE((a)->f32_products == FYC_PRODUCTS_EXACT || (a)->f32_products == FYC_PRODUCTS_SPLIT_BF16,                                         \
                name ": f32_products=%d (0 = exact, 1 = split bf16)", (a)->f32_products);                                                        \
    FYC_REQUIRE((a)->f32_products == FYC_PRODUCTS_EXACT || (a)->dtype == FYC_F32, name ": f32_products=%d needs dtype FYC_F32", (a)->f32_products); \
  } while (0)
