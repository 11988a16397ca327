// Temporal self-attention core of the AnimateDiff motion module (attention over the FRAME axis at
// every pixel; motion_module.py:371-464).  HBM-bound: arithmetic intensity ~F/2 FLOP/B.
//
// Input is the token-major output of the fused to_q|to_k|to_v GEMM, qkv[(b f p)][3C]; output is
// token-major o[(b f p)][C].  The reference's two physical transposes '(b f) d c <-> (b d) f c' are
// pure index arithmetic here: one wave64 owns one (clip b, pixel p, head h) task and gathers the
// F rows of that pixel (row stride P*3C) straight into MFMA operand registers.
//
// 16-bit path (v_mfma_f32_16x16x32_bf16 / _f16: template parameter T), F <= 64 (longer clips: temporal_attn_long.hip, one workgroup per task):
//   S^T = K Q^T (rows = key frames, cols = query frames), full softmax in registers (all keys of a
//   query are in 4 lanes x 4..16 regs), O^T = V^T P^T with the keys as the 32 MFMA k-slots (two such
//   MFMAs per output tile for F > 32).
// f32 path: scalar reference-precision kernel (parity mode only; F <= 256, its score array sized 64 or 256 by the clip); with f32_products =
// FYC_PRODUCTS_SPLIT_BF16 and F <= 64 the matrix-instruction kernel of temporal_attn_f32x3.hip (f32 storage, every product from three bf16 matrix
// instructions).  There is no split-product kernel for longer clips: they run the exact kernel, which is more accurate than the tier asks.
//
// ROPE (template parameter; rope_cos / rope_sin of fyc_tattn_args, f32 [F][d/2]): q and k are rotated per
// frame before the score product - x'[c] = x[c] cos[f][c mod h] -/+ x[c +/- h] sin[f][c mod h], h = d/2, the
// rotate_half pairing of the reference's RoPE (rope.py:102-116) - in f32 on the loaded values and rounded
// once to the operand type.  V is untouched.  The ROPE = false instantiations are the kernels without it.
#include "split_bf16.h"      // rp::mfma (row_panel.h), FYC_REQUIRE_F32_PRODUCTS
#include "temporal_attn.h"   // TAttnP, fyc_tattn_f32x3_launch

namespace {

// V^T operand of output tile t for key-tile pair pp, gathered from the wave's LDS tile (layout: at the tile's declaration)
template <typename T, int DP, int NFT>
__device__ __forceinline__ typename Pair16<T>::Vec8 vfrag(const unsigned short (*vt)[DP + 8], int pp, int t, int g, int r16) {
  const int dv = t * 16 + r16;
  unsigned short e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int fr = 32 * pp + ((j < 4) ? 4 * g + j : 16 + 4 * g + (j - 4));
    const bool ok = dv < DP && (j < 4 || 2 * pp + 1 < NFT);     // rows >= F and channels >= d hold zeros
    e[j] = ok ? vt[fr][dv] : (unsigned short)0;
  }
  u32x4 pk;
#pragma unroll
  for (int i = 0; i < 4; ++i) pk[i] = (unsigned)e[2 * i] | ((unsigned)e[2 * i + 1] << 16);
  return __builtin_bit_cast(typename Pair16<T>::Vec8, pk);
}

template <typename T, int DP, int DVT, int NFT, bool ROPE>
__global__ void __launch_bounds__(256) tattn_bf16_kernel(const TAttnP p) {
  typedef typename Pair16<T>::Vec8 Frag;
  constexpr int KS = DP / 32;
  constexpr int NP = (NFT + 1) / 2;   // k = 32 MFMAs per output tile of P V: one per pair of 16-frame key tiles
  const int lane = threadIdx.x & 63, g = lane >> 4, r16 = lane & 15;
  const long long task = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long long ntask = (long long)p.clips * p.pixels * p.heads;
  if (task >= ntask) return;
  const int h = (int)(task % p.heads);
  const long long bp = task / p.heads;
  const int pix = (int)(bp % p.pixels), b = (int)(bp / p.pixels);
  const int F = p.frames, C = p.heads * p.d, ld = 3 * C;
  const T* base = reinterpret_cast<const T*>(p.qkv) + ((long long)b * F * p.pixels + pix) * ld + h * p.d;
  const long long fstride = (long long)p.pixels * ld;  // elements between consecutive frames of a pixel
  const T* zero = reinterpret_cast<const T*>(p.zero);

  // Q / K fragments: lane (frame = 16*tile + r16, quad g) holds 8 consecutive head channels.  LAZY (F > 32): the MFMA operands of all
  // tiles (K, Q and V^T: 240 registers at d = 160, F = 64) do not fit the 256 architectural registers beside anything else, so only K
  // stays resident; the Q tile of a pass is loaded at its top and the V^T fragments are gathered from the LDS tile where they are used.
  // The same at F > 16 under ROPE, whose rotations hold partners and tables beside the operands (d = 160, F = 32: 264 -> 252 registers).
  constexpr bool LAZY = NFT > 2 || (ROPE && NFT > 1);
  const int hh = p.d >> 1;
  Frag qf[LAZY ? 1 : NFT][KS], kf[NFT][KS];
#pragma unroll
  for (int ft = 0; ft < NFT; ++ft) {
    const int fr = ft * 16 + r16;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int dd = 32 * ks + 8 * g;
      const bool ok = fr < F && dd < p.d;
      if constexpr (!LAZY) qf[ft][ks] = *reinterpret_cast<const Frag*>(ok ? base + fr * fstride + dd : zero);
      kf[ft][ks] = *reinterpret_cast<const Frag*>(ok ? base + fr * fstride + C + dd : zero);
      if constexpr (ROPE) {
        if constexpr (!LAZY) qf[ft][ks] = rope8<T>(qf[ft][ks], base + fr * fstride, dd, hh, p.rope_cos + fr * hh, p.rope_sin + fr * hh, ok, zero);
        kf[ft][ks] = rope8<T>(kf[ft][ks], base + fr * fstride + C, dd, hh, p.rope_cos + fr * hh, p.rope_sin + fr * hh, ok, zero);
      }
    }
  }
  // V^T fragments: lane (dv = 16*t + r16, quad g) of key-tile pair pp: k-slot j<4 <-> frame 32pp+4g+j, j>=4 <-> frame 32pp+16+4g+(j-4).  The operand wants
  // the FRAMES of one channel in a lane while memory has the channels of one frame contiguous: V rows are fetched like Q / K
  // (16 B per lane) and transposed through a wave-private LDS tile (2-byte gathers straight from global memory were 12-24
  // narrow requests per lane and held the kernel at 3.0 TB/s).  Row pitch DP + 8 elements: the four frame groups of a read
  // land 16 banks apart.
  __shared__ __attribute__((aligned(16))) unsigned short vsh[4][NFT * 16][DP + 8];
  unsigned short (*vt)[DP + 8] = vsh[threadIdx.x >> 6];
#pragma unroll
  for (int ft = 0; ft < NFT; ++ft) {
    const int fr = ft * 16 + r16;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int dd = 32 * ks + 8 * g;
      const bool ok = fr < F && dd < p.d;
      *reinterpret_cast<Frag*>(&vt[fr][dd]) = *reinterpret_cast<const Frag*>(ok ? base + fr * fstride + 2 * C + dd : zero);
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // same wave wrote and reads: LDS ops of a wave complete in order
  Frag vf[LAZY ? 1 : NP][DVT];
  if constexpr (!LAZY) {
#pragma unroll
    for (int t = 0; t < DVT; ++t) {
      const int dv = t * 16 + r16;
      unsigned short e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int fr = (j < 4) ? 4 * g + j : 16 + 4 * g + (j - 4);
        const bool ok = dv < DP && (j < 4 || NFT > 1);     // rows >= F and channels >= d hold zeros
        e[j] = ok ? vt[fr][dv] : (unsigned short)0;
      }
      u32x4 pk;
#pragma unroll
      for (int i = 0; i < 4; ++i) pk[i] = (unsigned)e[2 * i] | ((unsigned)e[2 * i + 1] << 16);
      vf[0][t] = __builtin_bit_cast(Frag, pk);
    }
  }

  const float sl2e = p.scale * 1.44269504088896340736f;
  T* obase = reinterpret_cast<T*>(p.o) + ((long long)b * F * p.pixels + pix) * C + h * p.d;
  const long long ofstride = (long long)p.pixels * C;

#pragma unroll
  for (int qt = 0; qt < NFT; ++qt) {
    if constexpr (LAZY) {
      const int fr = qt * 16 + r16;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int dd = 32 * ks + 8 * g;
        const bool ok = fr < F && dd < p.d;
        qf[0][ks] = *reinterpret_cast<const Frag*>(ok ? base + fr * fstride + dd : zero);
        if constexpr (ROPE) qf[0][ks] = rope8<T>(qf[0][ks], base + fr * fstride, dd, hh, p.rope_cos + fr * hh, p.rope_sin + fr * hh, ok, zero);
      }
    }
    // scores of query frame (qt*16 + r16) against key frames kt*16 + 4g + r
    f32x4 s[NFT];
#pragma unroll
    for (int kt = 0; kt < NFT; ++kt) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) a = rp::mfma(kf[kt][ks], qf[LAZY ? 0 : qt][ks], a);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (kt * 16 + 4 * g + r >= F) a[r] = -INFINITY;
      s[kt] = a;
    }
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NFT; ++kt) mx = fmaxf(mx, fmaxf(fmaxf(s[kt][0], s[kt][1]), fmaxf(s[kt][2], s[kt][3])));
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float pv[8 * NP], sum = 0.f;
#pragma unroll
    for (int j = 0; j < 8 * NP; ++j) pv[j] = 0.f;
#pragma unroll
    for (int kt = 0; kt < NFT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __builtin_amdgcn_exp2f((s[kt][r] - mx) * sl2e);
        pv[4 * kt + r] = e;
        sum += e;
      }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    const float inv = 1.0f / sum;
    Frag pf[NP];
#pragma unroll
    for (int pp = 0; pp < NP; ++pp) {
      u32x4 pk;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        pk[i] = (unsigned)Pair16<T>::to_bits(pv[8 * pp + 2 * i] * inv) | ((unsigned)Pair16<T>::to_bits(pv[8 * pp + 2 * i + 1] * inv) << 16);
      pf[pp] = __builtin_bit_cast(Frag, pk);
    }
    const int fq = qt * 16 + r16;
#pragma unroll
    for (int t = 0; t < DVT; ++t) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int pp = 0; pp < NP; ++pp) {
        if constexpr (LAZY) acc = rp::mfma(vfrag<T, DP, NFT>(vt, pp, t, g, r16), pf[pp], acc);
        else acc = rp::mfma(vf[pp][t], pf[pp], acc);
      }
      const int dd = t * 16 + 4 * g;
      if (fq < F && dd < p.d) {
        float v[4] = {acc[0], acc[1], acc[2], acc[3]};
        ElemIO<T>::st4(obase + fq * ofstride + dd, v);
      }
    }
  }
}

// parity-mode kernel: one thread per (b, pixel, head, query frame); f32 throughout.  MAXF >= F: the scores of a query (64: the kernel as it
// was, in registers; 256: clips of 65 .. 256 frames, the array in scratch - speed is not a goal of this mode)
template <bool ROPE, int MAXF>
__global__ void __launch_bounds__(256) tattn_f32_kernel(const TAttnP p) {
  const long long total = (long long)p.clips * p.pixels * p.heads * p.frames;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int fq = (int)(i % p.frames);
  long long t = i / p.frames;
  const int h = (int)(t % p.heads);
  t /= p.heads;
  const int pix = (int)(t % p.pixels), b = (int)(t / p.pixels);
  const int F = p.frames, C = p.heads * p.d, ld = 3 * C;
  const float* base = reinterpret_cast<const float*>(p.qkv) + ((long long)b * F * p.pixels + pix) * ld + h * p.d;
  const long long fs = (long long)p.pixels * ld;
  const float* q = base + fq * fs;
  float sc[MAXF];
  float mx = -INFINITY;
  for (int fk = 0; fk < F; ++fk) {
    const float* k = base + fk * fs + C;
    float a = 0.f;
    if constexpr (ROPE) {
      const int hh = p.d >> 1;
      const float *cq = p.rope_cos + fq * hh, *sq = p.rope_sin + fq * hh, *ck = p.rope_cos + fk * hh, *sk = p.rope_sin + fk * hh;
      for (int c = 0; c < p.d; ++c) {
        const bool low = c < hh;
        const int cp = low ? c + hh : c - hh, cm = low ? c : c - hh;
        const float qr = q[c] * cq[cm] + (low ? -q[cp] : q[cp]) * sq[cm];
        const float kr = k[c] * ck[cm] + (low ? -k[cp] : k[cp]) * sk[cm];
        a = fmaf(qr, kr, a);
      }
    } else
      for (int c = 0; c < p.d; ++c) a = fmaf(q[c], k[c], a);
    sc[fk] = a * p.scale;
    mx = fmaxf(mx, sc[fk]);
  }
  float sum = 0.f;
  for (int fk = 0; fk < F; ++fk) { sc[fk] = expf(sc[fk] - mx); sum += sc[fk]; }
  const float inv = 1.0f / sum;
  float* o = reinterpret_cast<float*>(p.o) + (((long long)b * F + fq) * p.pixels + pix) * C + h * p.d;
  for (int c = 0; c < p.d; ++c) {
    float a = 0.f;
    for (int fk = 0; fk < F; ++fk) a = fmaf(sc[fk] * inv, base[fk * fs + 2 * C + c], a);
    o[c] = a;
  }
}

template <typename T, int DP, int DVT, bool ROPE>
int launch_t(const TAttnP& p, hipStream_t st) {
  const long long ntask = (long long)p.clips * p.pixels * p.heads;
  dim3 grid((unsigned)((ntask + 3) / 4));
  if (p.frames <= 16) hipLaunchKernelGGL((tattn_bf16_kernel<T, DP, DVT, 1, ROPE>), grid, dim3(256), 0, st, p);
  else if (p.frames <= 32) hipLaunchKernelGGL((tattn_bf16_kernel<T, DP, DVT, 2, ROPE>), grid, dim3(256), 0, st, p);
  else if (p.frames <= 48) hipLaunchKernelGGL((tattn_bf16_kernel<T, DP, DVT, 3, ROPE>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((tattn_bf16_kernel<T, DP, DVT, 4, ROPE>), grid, dim3(256), 0, st, p);
  FYC_CHECK_LAUNCH("fyc_temporal_attention");
  return 0;
}

template <typename T, bool ROPE>
int launch_d(const TAttnP& p, hipStream_t st) {
  if (p.d <= 32) return launch_t<T, 32, 2, ROPE>(p, st);
  if (p.d <= 48) return launch_t<T, 64, 3, ROPE>(p, st);
  if (p.d <= 64) return launch_t<T, 64, 4, ROPE>(p, st);
  if (p.d <= 80) return launch_t<T, 96, 5, ROPE>(p, st);
  if (p.d <= 96) return launch_t<T, 96, 6, ROPE>(p, st);
  if (p.d <= 128) return launch_t<T, 128, 8, ROPE>(p, st);
  return launch_t<T, 160, 10, ROPE>(p, st);
}

}  // namespace

// the checks both entry points share (behind the null and f32_products checks) and the parameter block they fill; `fn` names the entry point in the messages
static int tattn_params(const fyc_tattn_args* a, const char* fn, TAttnP& p) {
  FYC_REQUIRE(g_fyc_zero_page != nullptr, "%s: fyc_init() not called", fn);
  FYC_REQUIRE(a->clips > 0 && a->frames > 0 && a->pixels > 0 && a->heads > 0, "%s: bad sizes", fn);
  FYC_REQUIRE(a->frames <= 256, "%s: frames=%d > 256 unsupported", fn, a->frames);
  FYC_REQUIRE((a->rope_cos == nullptr) == (a->rope_sin == nullptr), "%s: rope_cos and rope_sin must both be set or both be NULL", fn);
  FYC_REQUIRE((((uintptr_t)a->rope_cos | (uintptr_t)a->rope_sin) & 15) == 0, "%s: rope tables must be 16-byte aligned", fn);
  FYC_REQUIRE(a->d % 8 == 0 && a->d >= 8 && a->d <= 160, "%s: head dim %d", fn, a->d);
  p.qkv = a->qkv; p.o = a->o; p.clips = a->clips; p.frames = a->frames; p.pixels = a->pixels; p.heads = a->heads; p.d = a->d;
  p.scale = a->scale; p.zero = (const char*)g_fyc_zero_page;
  p.rope_cos = a->rope_cos; p.rope_sin = a->rope_sin;
  return 0;
}

extern "C" int fyc_temporal_attention(const fyc_tattn_args* a, void* stream) {
  FYC_REQUIRE(a && a->qkv && a->o, "fyc_temporal_attention: null pointer");
  FYC_REQUIRE_F32_PRODUCTS("fyc_temporal_attention", a);
  TAttnP p;
  if (const int rc = tattn_params(a, "fyc_temporal_attention", p)) return rc;
  const bool rope = a->rope_cos != nullptr;
  hipStream_t st = (hipStream_t)stream;
  if (a->dtype == FYC_F32) {
    if (a->f32_products == FYC_PRODUCTS_SPLIT_BF16 && p.frames <= 64) return fyc_tattn_f32x3_launch(p, st);      // temporal_attn_f32x3.hip
    const long long total = (long long)p.clips * p.pixels * p.heads * p.frames;
    FYC_REQUIRE(total + 255 < (256ll << 31), "fyc_temporal_attention(f32): %lld queries exceed the grid", total);
    const dim3 grid((unsigned)((total + 255) / 256));
    if (p.frames > 64) {      // (the split-product tier too: no split-product kernel covers these clips)
      if (rope) hipLaunchKernelGGL((tattn_f32_kernel<true, 256>), grid, dim3(256), 0, st, p);
      else hipLaunchKernelGGL((tattn_f32_kernel<false, 256>), grid, dim3(256), 0, st, p);
    } else if (rope) hipLaunchKernelGGL((tattn_f32_kernel<true, 64>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((tattn_f32_kernel<false, 64>), grid, dim3(256), 0, st, p);
    FYC_CHECK_LAUNCH("fyc_temporal_attention(f32)");
    return 0;
  }
  FYC_REQUIRE(a->dtype == FYC_BF16 || a->dtype == FYC_F16, "fyc_temporal_attention: bad dtype");
  if (p.frames > 64) return fyc_tattn_long_launch(p, a->dtype, st);      // temporal_attn_long.hip
  if (rope) return a->dtype == FYC_F16 ? launch_d<f16_t, true>(p, st) : launch_d<bf16_t, true>(p, st);
  return a->dtype == FYC_F16 ? launch_d<f16_t, false>(p, st) : launch_d<bf16_t, false>(p, st);
}

extern "C" int fyc_temporal_attention_long(const fyc_tattn_args* a, void* stream) {
  FYC_REQUIRE(a && a->qkv && a->o, "fyc_temporal_attention_long: null pointer");
  FYC_REQUIRE_F32_PRODUCTS("fyc_temporal_attention_long", a);
  TAttnP p;
  if (const int rc = tattn_params(a, "fyc_temporal_attention_long", p)) return rc;
  FYC_REQUIRE(a->dtype == FYC_BF16 || a->dtype == FYC_F16, "fyc_temporal_attention_long: FYC_BF16 / FYC_F16 tensors only (dtype %d)", a->dtype);
  FYC_REQUIRE(a->frames > 16, "fyc_temporal_attention_long: frames=%d: the long-clip kernel starts at 17 frames", a->frames);
  return fyc_tattn_long_launch(p, a->dtype, (hipStream_t)stream);
}
