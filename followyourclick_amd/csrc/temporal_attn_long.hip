// Temporal self-attention over clips of more than 64 frames (64 < F <= 256; fyc_temporal_attention_long runs it from 17 frames on), 16-bit types.
// Contract and numerical rules are temporal_attn.hip's: qkv[(b f p)][3C] in, o[(b f p)][C] out, the frames of a pixel gathered by index arithmetic,
// both products on v_mfma_f32_16x16x32_{bf16,f16} with f32 accumulation, the softmax in f32, P rounded to the storage type as the operand of P V,
// RoPE in f32 on the loaded q and k and rounded once, key frames >= F at -inf, the zero page for everything outside the problem.
//
// What differs is the work split.  The short kernel gives one wave a whole (clip, pixel, head) task with every K fragment and every score of a
// query in registers; at 256 frames and d = 160 the K fragments alone are 320 registers.  Here one WORKGROUP owns a task:
//   - one wave per 16-frame query tile (ceil(F / 16) waves, 2 .. 16): its Q fragments (rotated once) and its O^T accumulators stay in registers
//     for the whole task - 20 + 40 registers at d = 160;
//   - the keys go by in blocks of 64 frames: all waves together stage K (rotated once, row-major [frame][channel]) and V^T ([channel][frame],
//     transposed on the way in) of a block into LDS - 44.5 KB at d = 160, so q, k and v are read from HBM once per task - and every wave forms its
//     16 x 64 scores and its P V from LDS fragments;
//   - the softmax keeps a running maximum and rescales the accumulators between key blocks (the whole-row alternative holds 64 score
//     registers per query tile beside Q and O^T, past the 128 registers a wave of a 16-wave workgroup has, or needs a second sweep over K).
//     exp2((s - m) scale log2 e) of a block is rounded to the storage type for P V while the row sum adds the f32 values; the output is divided by
//     the row sum at the end.  Each p carries one rounding of the storage type, as in the short kernel, taken before instead of after the division.
//
// LDS: K rows at a pitch of DP + 8 elements (16-byte fragment reads of 16 consecutive rows land 4 .. 20 dwords apart); V^T rows at 72 elements =
// 36 dwords: the 8-byte reads of a fragment (16 channels x 4 frame groups) cover all 64 banks once.  V is written as frame PAIRS, one dword per
// channel, consecutive lanes on consecutive frame pairs: consecutive banks.
#include "split_bf16.h"      // rp::mfma (row_panel.h)
#include "temporal_attn.h"   // TAttnP, rope8

namespace {

constexpr int KB = 64;             // key frames per staged block
constexpr int VPITCH = KB + 8;     // elements per channel row of the V^T tile

template <typename T, int DP, int DVT, bool ROPE>
__global__ void __launch_bounds__(1024) tattn_long_kernel(const TAttnP p) {
  typedef typename Pair16<T>::Vec8 Frag;
  constexpr int KS = DP / 32, CG = DP / 8, KPITCH = DP + 8;
  static_assert(DP % 32 == 0 && DVT * 16 <= DP, "every output tile's channels lie inside the V^T tile");
  __shared__ __attribute__((aligned(16))) unsigned short ksh[KB][KPITCH];
  __shared__ __attribute__((aligned(16))) unsigned short vsh[DP][VPITCH];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int lane = tid & 63, g = lane >> 4, r16 = lane & 15, qt = tid >> 6;      // 64 * ceil(F / 16) threads: every wave has a query tile
  const long long task = blockIdx.x;
  const int h = (int)(task % p.heads);
  const long long bp = task / p.heads;
  const int pix = (int)(bp % p.pixels), b = (int)(bp / p.pixels);
  const int F = p.frames, C = p.heads * p.d, ld = 3 * C, hh = p.d >> 1;
  const T* base = reinterpret_cast<const T*>(p.qkv) + ((long long)b * F * p.pixels + pix) * ld + h * p.d;
  const long long fstride = (long long)p.pixels * ld;  // elements between consecutive frames of a pixel
  const T* zero = reinterpret_cast<const T*>(p.zero);

  // Q fragments of this wave's tile: lane (frame = 16 qt + r16, quad g) holds 8 consecutive head channels per k-step
  const int fq = qt * 16 + r16;
  Frag qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int dd = 32 * ks + 8 * g;
    const bool ok = fq < F && dd < p.d;
    const T* row = base + fq * fstride;
    qf[ks] = *reinterpret_cast<const Frag*>(ok ? row + dd : zero);
    if constexpr (ROPE) qf[ks] = rope8<T>(qf[ks], row, dd, hh, p.rope_cos + fq * hh, p.rope_sin + fq * hh, ok, zero);
  }

  const float sl2e = p.scale * 1.44269504088896340736f;
  f32x4 acc[DVT];
#pragma unroll
  for (int t = 0; t < DVT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float mx = -INFINITY, sum = 0.f;      // running maximum of query fq (all four quads agree); this lane's share of its row sum

  for (int k0 = 0; k0 < F; k0 += KB) {
    __syncthreads();      // the previous block's fragments have been read
    // K rows k0 .. k0+63, 16 bytes per thread and step; rows >= F and channels >= d hold zeros
    for (int c = tid; c < KB * CG; c += nthr) {
      const int fl = c / CG, dd = 8 * (c - fl * CG), fr = k0 + fl;
      const bool ok = fr < F && dd < p.d;
      const T* row = base + fr * fstride + C;
      Frag x = *reinterpret_cast<const Frag*>(ok ? row + dd : zero);
      if constexpr (ROPE) x = rope8<T>(x, row, dd, hh, p.rope_cos + fr * hh, p.rope_sin + fr * hh, ok, zero);
      *reinterpret_cast<Frag*>(&ksh[fl][dd]) = x;
    }
    // V^T: the 8 channels dd .. dd+7 of the frame pair (k0 + 2 fp, k0 + 2 fp + 1) become one dword in each of 8 channel rows
    for (int c = tid; c < (KB / 2) * CG; c += nthr) {
      const int fp = c & (KB / 2 - 1), dd = 8 * (c / (KB / 2)), f0 = k0 + 2 * fp;
      const bool in = dd < p.d;
      const T* row = base + f0 * fstride + 2 * C + dd;
      const u32x4 v0 = *reinterpret_cast<const u32x4*>(in && f0 < F ? row : zero);
      const u32x4 v1 = *reinterpret_cast<const u32x4*>(in && f0 + 1 < F ? row + fstride : zero);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        *reinterpret_cast<unsigned*>(&vsh[dd + 2 * i][2 * fp]) = (v0[i] & 0xffffu) | (v1[i] << 16);
        *reinterpret_cast<unsigned*>(&vsh[dd + 2 * i + 1][2 * fp]) = (v0[i] >> 16) | (v1[i] & 0xffff0000u);
      }
    }
    __syncthreads();

    // scores of query frame fq against key frames k0 + 16 kt + 4 g + r; tiles wholly behind F are skipped (uniform)
    f32x4 s[KB / 16];
    float bm = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < KB / 16; ++kt) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      if (k0 + kt * 16 < F) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) a = rp::mfma(*reinterpret_cast<const Frag*>(&ksh[kt * 16 + r16][32 * ks + 8 * g]), qf[ks], a);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (k0 + kt * 16 + 4 * g + r >= F) a[r] = -INFINITY;
        bm = fmaxf(bm, a[r]);
      }
      s[kt] = a;
    }
    bm = fmaxf(bm, __shfl_xor(bm, 16));
    bm = fmaxf(bm, __shfl_xor(bm, 32));
    const float mn = fmaxf(mx, bm);      // finite from the first block on: key frame 0 exists
    const float alpha = __builtin_amdgcn_exp2f((mx - mn) * sl2e);
    mx = mn;
    sum *= alpha;
#pragma unroll
    for (int t = 0; t < DVT; ++t) acc[t] *= alpha;
    Frag pf[KB / 32];
#pragma unroll
    for (int pp = 0; pp < KB / 32; ++pp) {
      float e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {      // k-slot j < 4 <-> key tile 2 pp, frame 4 g + j; j >= 4 <-> key tile 2 pp + 1, frame 4 g + j - 4
        e[j] = __builtin_amdgcn_exp2f((s[2 * pp + (j >> 2)][j & 3] - mn) * sl2e);
        sum += e[j];
      }
      u32x4 pk;
#pragma unroll
      for (int i = 0; i < 4; ++i) pk[i] = (unsigned)Pair16<T>::to_bits(e[2 * i]) | ((unsigned)Pair16<T>::to_bits(e[2 * i + 1]) << 16);
      pf[pp] = __builtin_bit_cast(Frag, pk);
    }
    // O^T += V^T P^T: lane (channel = 16 t + r16, quad g) reads the frames of its k-slots from the channel's row
#pragma unroll
    for (int pp = 0; pp < KB / 32; ++pp) {
      if (k0 + pp * 32 < F) {
#pragma unroll
        for (int t = 0; t < DVT; ++t) {
          const unsigned short* vr = &vsh[t * 16 + r16][32 * pp + 4 * g];
          const u32x2 lo = *reinterpret_cast<const u32x2*>(vr), hi = *reinterpret_cast<const u32x2*>(vr + 16);
          const u32x4 vv = {lo[0], lo[1], hi[0], hi[1]};
          acc[t] = rp::mfma(__builtin_bit_cast(Frag, vv), pf[pp], acc[t]);
        }
      }
    }
  }

  sum += __shfl_xor(sum, 16);
  sum += __shfl_xor(sum, 32);
  const float inv = 1.0f / sum;
  T* obase = reinterpret_cast<T*>(p.o) + ((long long)b * F * p.pixels + pix) * C + h * p.d;
  const long long ofstride = (long long)p.pixels * C;
#pragma unroll
  for (int t = 0; t < DVT; ++t) {
    const int dd = t * 16 + 4 * g;
    if (fq < F && dd < p.d) {
      const float v[4] = {acc[t][0] * inv, acc[t][1] * inv, acc[t][2] * inv, acc[t][3] * inv};
      ElemIO<T>::st4(obase + fq * ofstride + dd, v);
    }
  }
}

template <typename T, int DP, int DVT, bool ROPE>
int launch_t(const TAttnP& p, hipStream_t st) {
  const long long ntask = (long long)p.clips * p.pixels * p.heads;
  FYC_REQUIRE(ntask < (1ll << 31), "fyc_temporal_attention: %lld (clip, pixel, head) tasks exceed the grid", ntask);
  hipLaunchKernelGGL((tattn_long_kernel<T, DP, DVT, ROPE>), dim3((unsigned)ntask), dim3(64 * ((p.frames + 15) / 16)), 0, st, p);
  FYC_CHECK_LAUNCH("fyc_temporal_attention(long)");
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

int fyc_tattn_long_launch(const TAttnP& p, int dtype, hipStream_t st) {
  FYC_REQUIRE(p.frames > 16 && p.frames <= 256, "fyc_temporal_attention: the long-clip kernel covers 16 < frames <= 256 (frames=%d)", p.frames);
  FYC_REQUIRE(dtype == FYC_BF16 || dtype == FYC_F16, "fyc_temporal_attention: the long-clip kernel takes FYC_BF16 / FYC_F16 tensors");
  const bool rope = p.rope_cos != nullptr;
  if (rope) return dtype == FYC_F16 ? launch_d<f16_t, true>(p, st) : launch_d<bf16_t, true>(p, st);
  return dtype == FYC_F16 ? launch_d<f16_t, false>(p, st) : launch_d<bf16_t, false>(p, st);
}
