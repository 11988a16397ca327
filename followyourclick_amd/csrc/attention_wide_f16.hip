// f16 instantiations of the chunk-walking attention kernel (attention_wide.h): head dims above 160 and the causal mask.
#include "attention_wide.h"
int fyca::run_wide_f16(const AttnP& p, bool causal, hipStream_t st) { return run_wide_impl<f16_t>(p, causal, st); }
