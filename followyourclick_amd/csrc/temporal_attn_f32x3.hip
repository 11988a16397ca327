// Temporal self-attention on f32 tensors with split-bf16 products (fyc_tattn_args::f32_products = FYC_PRODUCTS_SPLIT_BF16, include/fyc.h): the
// work split of temporal_attn.hip's 16-bit kernel - one wave64 per (clip, pixel, head) task, S^T = K Q^T and O^T = V^T P^T on
// v_mfma_f32_16x16x32_bf16, the softmax in registers, -inf for the key frames outside the problem, the zero page for the lanes outside it - with
// f32 storage: a lane's eight head channels are two 16-byte loads, every operand fragment is split in registers into hi = RNE_bf16(x) and
// lo = RNE_bf16(x - hi), and every matrix instruction of the 16-bit kernel becomes three, lo hi, hi lo, hi hi (split_bf16.h: the rule, shared
// with attention_f32x3.hip; the two small terms meet the running sum first).  RoPE rotates q and k in f32 before the split.
//
// What the budgets decided (resource report: profiles/f32x3_tattn.txt):
//   K stays resident as hi + lo for all key tiles (160 registers at F = 64, d = 160); the Q fragment of a k-step is loaded, rotated and split
//   where it is used and serves all key tiles of that step (8 registers instead of a resident tile's 40); V^T fragments are always gathered
//   from LDS where they are used.  __launch_bounds__(256): the unified 512-entry file at one wave per SIMD takes what the largest shapes need.
//   LDS: V is transposed ONCE on its way in - the wave-private tile is [channel][frame] f32, so a V^T fragment is two 16-byte reads of the
//   frames 4g .. 4g+3 of a channel instead of eight 4-byte gathers, and re-reading it for every query tile (NFT times) is cheap.  Row pitch
//   16 NFT + 4 floats: the 16 channels of a 16-byte read phase land on 16 distinct bank quads.  4 tasks x DP x (16 NFT + 4) x 4 bytes is at
//   most 136 KB for every family but (DP 160, NFT 4) = 170 KB: that one runs two tasks per 128-thread block (85 KB).
#include "split_bf16.h"      // sb::Split, split8, mma3: the rule
#include "temporal_attn.h"   // TAttnP (filled by fyc_temporal_attention, temporal_attn.hip)

namespace {

using namespace sb;

// the 8 head channels dd .. dd+7 of one frame's q or k row (`row` = the head's first channel of that row), rotated (rotate_half, include/fyc.h:
// two rounded products and a rounded sum in f32 - the library is built with -ffp-contract=off) and split.  h = d/2 is a multiple of 4: each
// 4-channel run lies wholly below or above h and its partner run starts h channels away.  Lanes outside the problem read the zero page for
// values, partners and tables alike and keep their zeros.
template <bool ROPE>
__device__ __forceinline__ Split load_qk(const float* row, int dd, int hh, const float* ct, const float* st, bool ok, const float* zero) {
  f32x4 x[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int c0 = dd + 4 * r;
    x[r] = *reinterpret_cast<const f32x4*>(ok ? row + c0 : zero);
    if constexpr (ROPE) {
      const bool low = c0 < hh;
      const int cp = low ? c0 + hh : c0 - hh, cm = low ? c0 : c0 - hh;
      const f32x4 xp = *reinterpret_cast<const f32x4*>(ok ? row + cp : zero);
      const f32x4 cs = *reinterpret_cast<const f32x4*>(ok ? ct + cm : zero);
      const f32x4 sn = *reinterpret_cast<const f32x4*>(ok ? st + cm : zero);
#pragma unroll
      for (int i = 0; i < 4; ++i) x[r][i] = x[r][i] * cs[i] + (low ? -xp[i] : xp[i]) * sn[i];
    }
  }
  return split8(x[0], x[1]);
}

template <int DP, int DVT, int NFT, int TPB, bool ROPE>
__global__ void __launch_bounds__(64 * TPB) tattn_f32x3_kernel(const TAttnP p) {
  constexpr int KS = DP / 32;
  constexpr int NP = (NFT + 1) / 2;      // k = 32 MFMAs per output tile of P V: one per pair of 16-frame key tiles
  constexpr int PITCH = NFT * 16 + 4;    // floats per channel row of the V^T tile
  static_assert(DVT * 16 <= DP, "every output tile's channels lie inside the V^T tile");
  extern __shared__ __attribute__((aligned(16))) float vsh[];      // [TPB][DP][PITCH]
  const int lane = threadIdx.x & 63, g = lane >> 4, r16 = lane & 15, wave = threadIdx.x >> 6;
  const long long task = (long long)blockIdx.x * TPB + wave;
  const long long ntask = (long long)p.clips * p.pixels * p.heads;
  if (task >= ntask) return;
  const int h = (int)(task % p.heads);
  const long long bp = task / p.heads;
  const int pix = (int)(bp % p.pixels), b = (int)(bp / p.pixels);
  const int F = p.frames, C = p.heads * p.d, ld = 3 * C;
  const float* base = reinterpret_cast<const float*>(p.qkv) + ((long long)b * F * p.pixels + pix) * ld + h * p.d;
  const long long fstride = (long long)p.pixels * ld;  // elements between consecutive frames of a pixel
  const float* zero = reinterpret_cast<const float*>(p.zero);
  const int hh = p.d >> 1;

  // K fragments, resident: lane (frame = 16*tile + r16, quad g) holds 8 consecutive head channels as hi and lo
  Split kf[NFT][KS];
#pragma unroll
  for (int ft = 0; ft < NFT; ++ft) {
    const int fr = ft * 16 + r16;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int dd = 32 * ks + 8 * g;
      kf[ft][ks] = load_qk<ROPE>(base + fr * fstride + C, dd, hh, p.rope_cos + fr * hh, p.rope_sin + fr * hh, fr < F && dd < p.d, zero);
    }
  }
  // V: rows are fetched like K (32 B per lane) and written transposed, vt[channel][frame]; frames >= F and channels >= d hold zeros
  float* vt = vsh + wave * (DP * PITCH);
#pragma unroll
  for (int ft = 0; ft < NFT; ++ft) {
    const int fr = ft * 16 + r16;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int dd = 32 * ks + 8 * g;
      const bool ok = fr < F && dd < p.d;
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(ok ? base + fr * fstride + 2 * C + dd : zero);
      const f32x4 v1 = *reinterpret_cast<const f32x4*>(ok ? base + fr * fstride + 2 * C + dd + 4 : zero);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        vt[(dd + e) * PITCH + fr] = v0[e];
        vt[(dd + 4 + e) * PITCH + fr] = v1[e];
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // same wave wrote and reads: LDS ops of a wave complete in order

  const float sl2e = p.scale * 1.44269504088896340736f;
  float* obase = reinterpret_cast<float*>(p.o) + ((long long)b * F * p.pixels + pix) * C + h * p.d;
  const long long ofstride = (long long)p.pixels * C;

#pragma unroll
  for (int qt = 0; qt < NFT; ++qt) {
    const int fq = qt * 16 + r16;
    // scores of query frame fq against key frames kt*16 + 4g + r
    f32x4 s[NFT];
#pragma unroll
    for (int kt = 0; kt < NFT; ++kt) s[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int dd = 32 * ks + 8 * g;
      const Split qs = load_qk<ROPE>(base + fq * fstride, dd, hh, p.rope_cos + fq * hh, p.rope_sin + fq * hh, fq < F && dd < p.d, zero);
#pragma unroll
      for (int kt = 0; kt < NFT; ++kt) s[kt] = mma3(kf[kt][ks], qs, s[kt]);
    }
#pragma unroll
    for (int kt = 0; kt < NFT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (kt * 16 + 4 * g + r >= F) s[kt][r] = -INFINITY;
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
    // P^T operand: k-slot j<4 <-> key frame 32pp+4g+j, j>=4 <-> 32pp+16+4g+(j-4); normalised in f32, then split
    Split pf[NP];
#pragma unroll
    for (int pp = 0; pp < NP; ++pp) {
      const f32x4 p0 = {pv[8 * pp] * inv, pv[8 * pp + 1] * inv, pv[8 * pp + 2] * inv, pv[8 * pp + 3] * inv};
      const f32x4 p1 = {pv[8 * pp + 4] * inv, pv[8 * pp + 5] * inv, pv[8 * pp + 6] * inv, pv[8 * pp + 7] * inv};
      pf[pp] = split8(p0, p1);
    }
#pragma unroll
    for (int t = 0; t < DVT; ++t) {
      const float* vrow = vt + (t * 16 + r16) * PITCH + 4 * g;      // lane (channel 16t + r16, quad g)
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int pp = 0; pp < NP; ++pp) {
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(vrow + 32 * pp);
        f32x4 v1 = {0.f, 0.f, 0.f, 0.f};      // (an odd NFT has no second tile in its last pair)
        if (2 * pp + 1 < NFT) v1 = *reinterpret_cast<const f32x4*>(vrow + 32 * pp + 16);
        acc = mma3(split8(v0, v1), pf[pp], acc);
      }
      const int dd = t * 16 + 4 * g;
      if (fq < F && dd < p.d) *reinterpret_cast<f32x4*>(obase + fq * ofstride + dd) = acc;
    }
  }
}

template <int DP, int DVT, int NFT, bool ROPE>
int launch_k(const TAttnP& p, hipStream_t st) {
  constexpr int PITCH = NFT * 16 + 4;
  constexpr int TPB = 4 * DP * PITCH * 4 <= 160 * 1024 ? 4 : 2;      // tasks per block: what the 160 KiB of a CU hold
  constexpr int LDS_BYTES = TPB * DP * PITCH * 4;
  static_assert(LDS_BYTES <= 160 * 1024, "the V^T tiles of a block fit one CU");
  FYC_REQUIRE(rp::lds_fits(LDS_BYTES), "fyc_temporal_attention(f32, split products): %d bytes of LDS do not fit this device", LDS_BYTES);
  if constexpr (LDS_BYTES > 64 * 1024) {
    static rp::LdsAttr attr;                          // one per instantiation
    if (int rc = attr.set("fyc_temporal_attention(f32, split products)", LDS_BYTES, tattn_f32x3_kernel<DP, DVT, NFT, TPB, ROPE>)) return rc;
  }
  const long long ntask = (long long)p.clips * p.pixels * p.heads;
  hipLaunchKernelGGL((tattn_f32x3_kernel<DP, DVT, NFT, TPB, ROPE>), dim3((unsigned)((ntask + TPB - 1) / TPB)), dim3(64 * TPB), LDS_BYTES, st, p);
  FYC_CHECK_LAUNCH("fyc_temporal_attention(f32, split products)");
  return 0;
}

template <int DP, int DVT, bool ROPE>
int launch_t(const TAttnP& p, hipStream_t st) {
  if (p.frames <= 16) return launch_k<DP, DVT, 1, ROPE>(p, st);
  if (p.frames <= 32) return launch_k<DP, DVT, 2, ROPE>(p, st);
  if (p.frames <= 48) return launch_k<DP, DVT, 3, ROPE>(p, st);
  return launch_k<DP, DVT, 4, ROPE>(p, st);
}

template <bool ROPE>
int launch_d(const TAttnP& p, hipStream_t st) {      // the head-dim families of temporal_attn.hip
  if (p.d <= 32) return launch_t<32, 2, ROPE>(p, st);
  if (p.d <= 48) return launch_t<64, 3, ROPE>(p, st);
  if (p.d <= 64) return launch_t<64, 4, ROPE>(p, st);
  if (p.d <= 80) return launch_t<96, 5, ROPE>(p, st);
  if (p.d <= 96) return launch_t<96, 6, ROPE>(p, st);
  if (p.d <= 128) return launch_t<128, 8, ROPE>(p, st);
  return launch_t<160, 10, ROPE>(p, st);
}

}  // namespace

// fyc_temporal_attention has checked sizes, head dim, frames <= 64, the tables and the zero page, and has filled p
int fyc_tattn_f32x3_launch(const TAttnP& p, hipStream_t st) {
  FYC_REQUIRE(rp::aligned16(p.qkv, p.o), "fyc_temporal_attention: f32_products = FYC_PRODUCTS_SPLIT_BF16 needs 16-byte aligned qkv and o");
  return p.rope_cos != nullptr ? launch_d<true>(p, st) : launch_d<false>(p, st);
}
