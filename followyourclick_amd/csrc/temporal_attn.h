// What temporal_attn.hip (entry points; 16-bit and exact f32 kernels), temporal_attn_long.hip (16-bit, clips of more than 64 frames) and
// temporal_attn_f32x3.hip (f32 tensors, split-bf16 products) share: the parameter block the entry points fill once, the other files' launchers and
// the rotation of a q / k fragment.
#pragma once
#include "fyc_common.h"

struct TAttnP {
  const void* qkv; void* o;      // elements of the kernel's type: cast where the kernel starts
  int clips, frames, pixels, heads, d;
  float scale;
  const char* zero;
  const float* rope_cos; const float* rope_sin;
};

// FYC_F32 tensors with f32_products = FYC_PRODUCTS_SPLIT_BF16; fyc_temporal_attention has checked sizes, head dim, frames <= 64, the tables and the zero page
int fyc_tattn_f32x3_launch(const TAttnP& p, hipStream_t st);
// FYC_BF16 / FYC_F16 tensors, 16 < frames <= 256 (temporal_attn_long.hip); the entry points have checked sizes, head dim, the tables and the zero page
int fyc_tattn_long_launch(const TAttnP& p, int dtype, hipStream_t st);

// rotate_half on the 8 head channels dd .. dd+7 of one frame's q or k row (`row` = the head's first channel of that row).  h = d/2 is
// a multiple of 4, so each 4-channel run of the fragment lies wholly below or above h and its partner run starts h channels away: at
// d = 8 inside this fragment, at d = 40 across two others.  The partners come from a second, 8-byte load of the same row (same cache
// lines, no HBM traffic).  Lanes outside the problem read the zero page for values, partners and tables alike and keep their zeros.
template <typename T>
__device__ __forceinline__ typename Pair16<T>::Vec8 rope8(typename Pair16<T>::Vec8 x, const T* row, int dd, int hh, const float* ct,
                                                          const float* st, bool ok, const T* zero) {
  const u32x4 xb = __builtin_bit_cast(u32x4, x);
  u32x4 xo;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int c0 = dd + 4 * r;
    const bool low = c0 < hh;
    const int cp = low ? c0 + hh : c0 - hh, cm = low ? c0 : c0 - hh;
    float xp[4];
    ElemIO<T>::ld4(ok ? row + cp : zero, xp);
    const f32x4 cs = *reinterpret_cast<const f32x4*>(ok ? ct + cm : reinterpret_cast<const float*>(zero));
    const f32x4 sn = *reinterpret_cast<const f32x4*>(ok ? st + cm : reinterpret_cast<const float*>(zero));
    const float xv[4] = {Pair16<T>::lo(xb[2 * r]), Pair16<T>::hi(xb[2 * r]), Pair16<T>::lo(xb[2 * r + 1]), Pair16<T>::hi(xb[2 * r + 1])};
    float y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = xv[i] * cs[i] + (low ? -xp[i] : xp[i]) * sn[i];
    xo[2 * r] = Pair16<T>::pack(y[0], y[1]);
    xo[2 * r + 1] = Pair16<T>::pack(y[2], y[3]);
  }
  return __builtin_bit_cast(typename Pair16<T>::Vec8, xo);
}
