// Host entry of the GEMM family: argument validation, plan (gemm_plan.h), dispatch.
// Kernel template: gemm_kernel.h; instantiations: gemm_{bf16,f16}_{plain,conv,act,t3}.hip, gemm_f32.hip, gemm_f32_t3.hip, gemm_f32x3.hip, gemm_f32x3_t3.hip.
#include "gemm_plan.h"

using namespace fycg;

namespace {
// ---- split-K finish (when a problem splits, and why: gemm_plan.h).  The main kernel leaves one raw f32 partial per K slice in the
// caller's workspace; this kernel adds the `S` slices and applies the LINEAR epilogue.
template <typename T>
__global__ void __launch_bounds__(256) splitk_finish_kernel(const float* __restrict__ ws, int S, const float* __restrict__ bias,
                                                            const float* __restrict__ rowbias, int rows_per_batch, int ldrb,
                                                            const T* __restrict__ residual, int ldr, T* __restrict__ out, int ldo,
                                                            int M, int N, float out_scale) {
  const int n8 = N >> 3;
  for (long long idx = blockIdx.x * 256ll + threadIdx.x; idx < (long long)M * n8; idx += gridDim.x * 256ll) {
    const int m = (int)(idx / n8), n = (int)(idx - (long long)m * n8) * 8;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    for (int s = 0; s < S; ++s) {
      const float* src = ws + ((long long)s * M + m) * N + n;
      const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[e] += a[e]; v[4 + e] += b[e]; }
    }
    if (bias) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += bias[n + e];
    }
    if (rowbias) {
      const float* rb = rowbias + (long long)(m / rows_per_batch) * ldrb + n;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += rb[e];
    }
    if (residual) {
      float r[8];
      load8<T>(residual + (long long)m * ldr + n, r);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += r[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= out_scale;
    store8<T>(out + (long long)m * ldo + n, v);
  }
}

// The same finish with the OUTPUT STATISTICS of the LINEAR epilogue (fyc_gemm chan_parts; round 6: the split-K convolutions of the
// 8x8 level used to send their consumers to the separate fyc_gn_stats pass - 40 launches per forward).  One block = 128 rows (the
// row tile both split tile configs use: fyc_gemm_stat_layout) x 64 columns: the values go out as above, their rounded copies are
// parked in LDS and thread (slot, column) adds the rows of its sample slot IN ROW ORDER - no atomics, bitwise repeatable - and writes
// chan_parts[tile][slot][n] = {sum, sum of squares} of the values as stored.
template <typename T>
__global__ void __launch_bounds__(256) splitk_finish_stats_kernel(const float* __restrict__ ws, int S, const float* __restrict__ bias,
                                                                  const float* __restrict__ rowbias, int rows_per_batch, int ldrb,
                                                                  const T* __restrict__ residual, int ldr, T* __restrict__ out, int ldo,
                                                                  int M, int N, float out_scale, float* __restrict__ chan_parts, int cs_rows, int cs_slots) {
  __shared__ float tile[128][64];
  const int tile_m = blockIdx.x, n0 = blockIdx.y * 64;
  const int cch = threadIdx.x & 7, rsub = threadIdx.x >> 3;
  const int n = n0 + cch * 8;
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {      // (unrolled: the partial-sum loads of the four passes are independent)
    const int lr = pass * 32 + rsub, m = tile_m * 128 + lr;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    if (m < M && n < N) {
      for (int s = 0; s < S; ++s) {
        const float* src = ws + ((long long)s * M + m) * N + n;
        const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] += a[e]; v[4 + e] += b[e]; }
      }
      if (bias) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += bias[n + e];
      }
      if (rowbias) {
        const float* rb = rowbias + (long long)(m / rows_per_batch) * ldrb + n;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += rb[e];
      }
      if (residual) {
        float r[8];
        load8<T>(residual + (long long)m * ldr + n, r);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += r[e];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = round_through<T>(v[e] * out_scale);     // the value as stored
      store8<T>(out + (long long)m * ldo + n, v);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) tile[lr][cch * 8 + e] = v[e];                     // rows / columns outside the problem: 0
  }
  __syncthreads();
  const int col = threadIdx.x & 63, slot = threadIdx.x >> 6;                       // one wave per sample slot (cs_slots <= 4)
  if (slot < cs_slots && n0 + col < N) {
    const int first = (tile_m * 128) / cs_rows;
    const long long lo = (long long)(first + slot) * cs_rows - (long long)tile_m * 128, hi = lo + cs_rows;
    const int r0 = lo < 0 ? 0 : (int)lo, r1 = hi > 128 ? 128 : (int)hi;
    float sx = 0.f, sq = 0.f;
    for (int r = r0; r < r1; ++r) { const float x = tile[r][col]; sx += x; sq = __builtin_fmaf(x, x, sq); }
    *reinterpret_cast<float2*>(chan_parts + (((long long)tile_m * cs_slots + slot) * N + n0 + col) * 2) = make_float2(sx, sq);
  }
}

// the kernel entry of a plan's family; `products`: fyc_gemm_args::f32_products - the plan is the same for both rules, only the instantiation differs
int run(const GemmPlan& pl, const GemmP& p, int products, int batch, hipStream_t st) {
  if (pl.dtype == FYC_F32) {
    const int cfg = pl.cfg | (products == FYC_PRODUCTS_SPLIT_BF16 ? CFG_F32X3 : 0);
    return pl.family == GEMM_FAM_T3 ? run_f32_t3(p, batch, cfg, st) : run_f32(p, batch, cfg, st);
  }
  const bool f16 = pl.dtype == FYC_F16;
  switch (pl.family) {
    case GEMM_FAM_T3: return f16 ? run_f16_t3(p, batch, pl.cfg, pl.ns, st) : run_bf16_t3(p, batch, pl.cfg, pl.ns, st);
    case GEMM_FAM_ACT: return f16 ? run_f16_act(p, batch, pl.cfg, st) : run_bf16_act(p, batch, pl.cfg, st);
    case GEMM_FAM_PLAIN: return f16 ? run_f16_plain(p, batch, pl.cfg, pl.ns, st) : run_bf16_plain(p, batch, pl.cfg, pl.ns, st);
    default: return f16 ? run_f16_conv(p, batch, pl.cfg, pl.ns, st) : run_bf16_conv(p, batch, pl.cfg, pl.ns, st);
  }
}

// adds the K slices of a split problem and applies the LINEAR epilogue (with chan_parts: and writes the statistics)
template <typename T>
int finish(const GemmP& p, hipStream_t st) {
  if (p.chan_parts != nullptr) {
    hipLaunchKernelGGL(splitk_finish_stats_kernel<T>, dim3((p.M + 127) / 128, (p.N + 63) / 64), dim3(256), 0, st, (const float*)p.ws, p.splitk, p.bias, p.rowbias, p.rows_per_batch, p.ldrb,
                       (const T*)p.residual, p.ldr, (T*)p.out, p.ldo, p.M, p.N, p.out_scale, p.chan_parts, p.cs_rows, p.cs_slots);
    FYC_CHECK_LAUNCH("fyc_gemm split-K finish + statistics");
    return 0;
  }
  const long long items = (long long)p.M * (p.N / 8);
  const int blocks = (int)((items + 255) / 256 < 4096 ? (items + 255) / 256 : 4096);
  hipLaunchKernelGGL(splitk_finish_kernel<T>, dim3(blocks), dim3(256), 0, st, (const float*)p.ws, p.splitk, p.bias, p.rowbias, p.rows_per_batch, p.ldrb,
                     (const T*)p.residual, p.ldr, (T*)p.out, p.ldo, p.M, p.N, p.out_scale);
  FYC_CHECK_LAUNCH("fyc_gemm split-K finish");
  return 0;
}

// the plan of a host query: no checks, no workspace needed
bool query_plan(const fyc_gemm_args* a, int stats, GemmPlan& pl) {
  char unused[512];
  return a != nullptr && a->M > 0 && a->N > 0 && plan_gemm(a, stats, true, pl, unused);
}
int stats_of(const fyc_gemm_args* a) { return (a->chan_parts != nullptr ? GEMM_STATS_CHAN : 0) | (a->row_parts != nullptr ? GEMM_STATS_ROW : 0); }
}  // namespace

extern "C" int64_t fyc_gemm_workspace_bytes(const fyc_gemm_args* a) {
  GemmPlan pl;
  return query_plan(a, a != nullptr ? stats_of(a) : 0, pl) ? pl.ws_bytes : 0;
}
extern "C" int fyc_gemm_row_parts(const fyc_gemm_args* a) {
  GemmPlan pl;
  return query_plan(a, GEMM_STATS_ROW, pl) ? pl.col_tiles : 0;
}
extern "C" int fyc_gemm_stat_layout(const fyc_gemm_args* a, int32_t* tile_rows, int32_t* slots) {
  GemmPlan pl;
  if (a == nullptr || a->cs_rows <= 0 || !query_plan(a, GEMM_STATS_CHAN, pl)) return 0;
  if (tile_rows) *tile_rows = pl.bm;
  if (slots) *slots = pl.cs_slots;
  return pl.row_tiles;
}

extern "C" int fyc_gemm(const fyc_gemm_args* a, void* stream) {
  FYC_REQUIRE(a != nullptr, "fyc_gemm: null args");
  FYC_REQUIRE(a->f32_products == FYC_PRODUCTS_EXACT || (a->f32_products == FYC_PRODUCTS_SPLIT_BF16 && a->dtype == FYC_F32),
              "fyc_gemm: f32_products=%d must be 0 (exact) or, with dtype FYC_F32 only, 1 (split bf16) - dtype %d", a->f32_products, a->dtype);
  FYC_REQUIRE(g_fyc_zero_page != nullptr, "fyc_gemm: fyc_init() not called");
  FYC_REQUIRE(a->dtype == FYC_F32 || gemm_is16(a->dtype), "fyc_gemm: bad dtype %d", a->dtype);
  const int es = gemm_is16(a->dtype) ? 2 : 4, ch = 16 / es;
  FYC_REQUIRE(a->M > 0 && a->N > 0 && a->K > 0, "fyc_gemm: empty problem M=%d N=%d K=%d", a->M, a->N, a->K);
  FYC_REQUIRE((a->ln_stats == nullptr) == (a->ln_colsum == nullptr) && (a->ln_stats == nullptr || (a->mode == FYC_GEMM_PLAIN && a->batch <= 1 && ((uintptr_t)a->ln_stats % 8) == 0 && ((uintptr_t)a->ln_colsum % 16) == 0)),
              "fyc_gemm: ln_stats / ln_colsum must come together (PLAIN mode, no batch, 8-/16-byte aligned)");
  FYC_REQUIRE(a->act >= FYC_ACT_NONE && a->act <= FYC_ACT_QUICK_GELU && (a->act == FYC_ACT_NONE || a->epilogue == FYC_EPI_LINEAR),
              "fyc_gemm: act=%d needs the LINEAR epilogue", a->act);
  FYC_REQUIRE(a->K % ch == 0, "fyc_gemm: K=%d must be a multiple of %d", a->K, ch);
  FYC_REQUIRE(a->ldw % ch == 0 && a->stride_w % ch == 0, "fyc_gemm: ldw/stride_w must keep 16-B alignment");
  FYC_REQUIRE(((uintptr_t)a->a % 16) == 0 && ((uintptr_t)a->w % 16) == 0, "fyc_gemm: operands must be 16-B aligned");
  GemmP p;
  memset(&p, 0, sizeof(p));
  p.a = (const char*)a->a; p.a2 = (const char*)a->a2; p.w = (const char*)a->w;
  p.k_split = a->k_split; p.lda2 = a->lda2; p.bias = a->bias; p.rowbias = a->rowbias;
  p.residual = (const char*)a->residual; p.out = (char*)a->out;
  p.M = a->M; p.N = a->N; p.K = a->K; p.lda = a->lda; p.ldw = a->ldw; p.ldo = a->ldo; p.ldr = a->ldr;
  p.stride_a = a->stride_a; p.stride_w = a->stride_w; p.stride_o = a->stride_o;
  p.mode = a->mode; p.epilogue = a->epilogue;
  p.Hout = a->Hout; p.Wout = a->Wout; p.Hin = a->Hin; p.Win = a->Win; p.Cin = a->Cin; p.conv_stride = a->conv_stride; p.conv_pad = a->conv_pad;
  p.rows_per_batch = a->rows_per_batch > 0 ? a->rows_per_batch : 1;
  p.ldrb = a->ldrb > 0 ? a->ldrb : a->N;
  p.out_scale = a->out_scale;
  p.act = a->act;
  p.ln_stats = a->ln_stats; p.ln_colsum = a->ln_colsum;
  p.ln_nparts = a->ln_nparts; p.ln_eps = a->ln_eps;
  FYC_REQUIRE(a->ln_nparts >= 0 && (a->ln_nparts == 0 || (a->ln_stats != nullptr && a->a2 == nullptr)), "fyc_gemm: ln_nparts=%d needs ln_stats (and no a2)", a->ln_nparts);
  p.chan_parts = a->chan_parts; p.cs_rows = a->cs_rows; p.row_parts = a->row_parts; p.row_nparts = a->row_nparts;
  FYC_REQUIRE((a->chan_parts == nullptr && a->row_parts == nullptr) || (a->epilogue == FYC_EPI_LINEAR && (a->batch <= 1) && (a->dtype == FYC_F32 || a->act == FYC_ACT_NONE)),
              "fyc_gemm: output statistics need the LINEAR epilogue without batch (bf16: without activation)");
  p.zero = (const char*)g_fyc_zero_page;
  const int batch = a->batch > 0 ? a->batch : 1;
  {   // the loaders keep 32-bit element offsets inside one batch element
    const long long lim = 0xffffffffll;
    const bool small = (long long)a->N * a->ldw < lim &&
                       (a->mode == FYC_GEMM_PLAIN ? ((long long)a->M * a->lda < lim && (a->a2 == nullptr || (long long)a->M * a->lda2 < lim))
                        : a->mode == FYC_GEMM_CONV_T3 ? (long long)a->M * a->Cin < lim
                                                  : (a->Hout > 0 && a->Wout > 0 && (long long)a->M / ((long long)a->Hout * a->Wout) * a->Hin * a->Win * a->Cin < lim));
    FYC_REQUIRE(small, "fyc_gemm: an operand has 2^32 elements or more (M=%d lda=%d N=%d ldw=%d): split the call", a->M, a->lda, a->N, a->ldw);
  }
  FYC_REQUIRE(a->mode == FYC_GEMM_CONV_T3 || (a->t3_frames == 0 && a->t3_rows == 0), "fyc_gemm: t3_frames / t3_rows belong to FYC_GEMM_CONV_T3 (mode %d)", a->mode);
  if (a->mode == FYC_GEMM_PLAIN) {
    FYC_REQUIRE(a->lda % ch == 0 && a->stride_a % ch == 0, "fyc_gemm: lda/stride_a must keep 16-B alignment");
    if (a->a2 != nullptr) {
      FYC_REQUIRE(a->k_split > 0 && a->k_split < a->K && a->k_split % (8 * ch) == 0, "fyc_gemm: k_split=%d must be a multiple of %d inside (0, K)", a->k_split, 8 * ch);
      FYC_REQUIRE(a->lda2 % ch == 0 && ((uintptr_t)a->a2 % 16) == 0 && batch == 1, "fyc_gemm: a2 alignment / batch");
    }
  } else if (a->mode == FYC_GEMM_CONV_T3) {
    // 3 taps along the frame axis: a = [clips * t3_frames * t3_rows][Cin] channels-last, K order (slab, tap, channel)
    FYC_REQUIRE(a->Cin > 0 && a->Cin % 64 == 0, "fyc_gemm conv_t3: Cin=%d must be a multiple of 64", a->Cin);
    FYC_REQUIRE(a->K == 3 * a->Cin, "fyc_gemm conv_t3: K=%d != 3*Cin (Cin=%d)", a->K, a->Cin);
    FYC_REQUIRE(a->t3_frames > 0 && a->t3_rows > 0, "fyc_gemm conv_t3: t3_frames=%d / t3_rows=%d must be positive", a->t3_frames, a->t3_rows);
    FYC_REQUIRE((long long)a->M % ((long long)a->t3_frames * a->t3_rows) == 0, "fyc_gemm conv_t3: M=%d is not a whole number of clips of %d x %d rows", a->M, a->t3_frames, a->t3_rows);
    FYC_REQUIRE(batch == 1, "fyc_gemm conv_t3: batch must be 1");
    FYC_REQUIRE(a->a2 == nullptr && a->epilogue == FYC_EPI_LINEAR && a->act == FYC_ACT_NONE && a->ln_stats == nullptr,
                "fyc_gemm conv_t3: the LINEAR epilogue without activation, a2 or a folded LayerNorm");
    p.t3_frames = a->t3_frames; p.t3_rows = a->t3_rows;
  } else {
    const int bk = 8 * ch;
    FYC_REQUIRE(a->mode == FYC_GEMM_CONV3X3 || a->mode == FYC_GEMM_CONV3X3_UP2, "fyc_gemm: bad mode %d", a->mode);
    FYC_REQUIRE(a->Cin > 0 && a->Cin % bk == 0, "fyc_gemm conv: Cin=%d must be a multiple of %d", a->Cin, bk);
    FYC_REQUIRE(a->K == 9 * a->Cin, "fyc_gemm conv: K=%d != 9*Cin", a->K);
    FYC_REQUIRE(a->Hout > 0 && a->Wout > 0 && a->Hin > 0 && a->Win > 0, "fyc_gemm conv: bad spatial dims");
    FYC_REQUIRE(a->M % (a->Hout * a->Wout) == 0, "fyc_gemm conv: M=%d not a multiple of Hout*Wout", a->M);
    FYC_REQUIRE(batch == 1, "fyc_gemm conv: batch must be 1");
    FYC_REQUIRE(a->a2 == nullptr, "fyc_gemm conv: a2 is a PLAIN-mode feature");
    if (a->mode == FYC_GEMM_CONV3X3) {
      FYC_REQUIRE(a->conv_stride == 1 || a->conv_stride == 2, "fyc_gemm conv: stride %d", a->conv_stride);
      FYC_REQUIRE(a->conv_pad == 0 || a->conv_pad == 1, "fyc_gemm conv: conv_pad must be 0 or 1");
      FYC_REQUIRE(a->Hout == (a->Hin + a->conv_pad + 1 - 3) / a->conv_stride + 1 && a->Wout == (a->Win + a->conv_pad + 1 - 3) / a->conv_stride + 1,
                  "fyc_gemm conv: output size mismatch");
    } else {
      p.conv_stride = 1;
      p.conv_pad = 1;
      FYC_REQUIRE(a->Hout >= a->Hin && a->Wout >= a->Win, "fyc_gemm upconv: output must not be smaller than the input");
      p.up_exact2 = (a->Hout == 2 * a->Hin && a->Wout == 2 * a->Win) ? 1 : 0;
      p.up_sh = (float)a->Hin / (float)a->Hout;
      p.up_sw = (float)a->Win / (float)a->Wout;
    }
  }
  if (a->epilogue == FYC_EPI_GEGLU) {
    FYC_REQUIRE(a->N % 32 == 0, "fyc_gemm GEGLU: N=%d must be a multiple of 32", a->N);
    FYC_REQUIRE(a->residual == nullptr && a->rowbias == nullptr, "fyc_gemm GEGLU: residual/rowbias unsupported");
  } else if (a->epilogue == FYC_EPI_HEADS) {
    FYC_REQUIRE(a->seg_cols > 0 && a->heads > 0 && a->tokens > 0, "fyc_gemm HEADS: bad seg_cols/heads/tokens");
    FYC_REQUIRE(a->N % a->seg_cols == 0 && a->N / a->seg_cols <= 3, "fyc_gemm HEADS: N=%d vs seg_cols=%d", a->N, a->seg_cols);
    FYC_REQUIRE(a->seg_cols % a->heads == 0 && (a->seg_cols / a->heads) % 4 == 0, "fyc_gemm HEADS: head_dim must be a multiple of 4");
    FYC_REQUIRE(a->M % a->tokens == 0, "fyc_gemm HEADS: M not a multiple of tokens");
    FYC_REQUIRE(a->residual == nullptr && batch == 1, "fyc_gemm HEADS: residual/batch unsupported");
    p.seg_cols = a->seg_cols; p.heads = a->heads; p.tokens = a->tokens; p.head_dim = a->seg_cols / a->heads;
    p.inv_seg_cols = 1.0f / (float)p.seg_cols; p.inv_head_dim = 1.0f / (float)p.head_dim;      // (fdiv_small: N < 2^16, divisors <= 2^12)
    FYC_REQUIRE(a->N < 65536 && p.seg_cols <= 4096, "fyc_gemm HEADS: N=%d / seg_cols=%d beyond the epilogue's index arithmetic", a->N, p.seg_cols);
    for (int s = 0; s < a->N / a->seg_cols; ++s) {
      FYC_REQUIRE(a->seg_out[s] != nullptr, "fyc_gemm HEADS: seg_out[%d] null", s);
      p.seg_out[s] = (char*)a->seg_out[s];
      p.seg_transposed[s] = a->seg_transposed[s];
      p.seg_ld[s] = a->seg_ld[s] > 0 ? a->seg_ld[s] : a->tokens;
      FYC_REQUIRE(p.seg_ld[s] >= a->tokens, "fyc_gemm HEADS: seg_ld[%d] < tokens", s);
    }
  } else {
    FYC_REQUIRE(a->epilogue == FYC_EPI_LINEAR, "fyc_gemm: bad epilogue %d", a->epilogue);
    FYC_REQUIRE(a->out != nullptr, "fyc_gemm: out is null");
  }
  GemmPlan pl;
  if (!plan_gemm(a, stats_of(a), false, pl, g_fyc_err)) return -2;
  p.wide = pl.wide; p.colc = pl.colc; p.cs_slots = pl.cs_slots;
  if (pl.splitk > 1) { p.splitk = pl.splitk; p.ws = (float*)a->workspace; }
  const int rc = run(pl, p, a->f32_products, batch, (hipStream_t)stream);
  if (rc != 0 || pl.splitk <= 1) return rc;
  return a->dtype == FYC_F16 ? finish<f16_t>(p, (hipStream_t)stream) : finish<bf16_t>(p, (hipStream_t)stream);
}
