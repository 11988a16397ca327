// f32 tensors with split-bf16 products (the ABI-307 rule): instantiations of the chunk-walking attention kernel (attention_wide.h), head dims above 160 and the causal mask.
#include "attention_wide.h"
int fyca::run_wide_f32x3(const AttnP& p, bool causal, hipStream_t st) { return run_wide_impl<float>(p, causal, st); }
