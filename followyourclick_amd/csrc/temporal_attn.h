// What temporal_attn.hip (entry point; 16-bit and exact f32 kernels) and temporal_attn_f32x3.hip (f32 tensors, split-bf16 products) share: the
// parameter block fyc_temporal_attention fills once, and the second file's launcher.
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
