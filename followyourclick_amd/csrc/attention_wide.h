// Fused flash attention for what the kernels of attention_kernel.h / attention_f32x3.hip do not take (version 308: fyc_attention, fyc_attention_masked): head dims above 160 (multiples
// of 32 up to 512, the VAE mid block's single head of 512) and the causal mask (key j counts for query i iff j <= i: the CLIP text tower), for the three
// element families - T = bf16_t / f16_t (16-bit rule of include/fyc.h) and T = float (split-bf16 products, the ABI-307 rule word for word).
//
// The work split is the one of those kernels: a workgroup of 4 wave64 on 64 QT queries of one (batch, head), each wave 16 QT queries for the whole key loop,
// S^T = K Q'^T (v_mfma_f32_16x16x32) so that a lane's 8 exponentiated scores of a 32-key block are the B operand of O^T = V^T P^T, K and V^T by LDS-DMA
// (global_load_lds, 16 B / lane) through a ring with counted vmcnt waits behind raw s_barriers.  What differs:
//   * the head dim is walked in CHUNKS of 128 channels.  At d = 512 a 32-key tile of K plus V^T is 64 KB in 16 bits and 128 KB in f32: a ring of whole tiles does
//     not fit.  A ring stage here holds ONE unit - the K rows of one chunk (32 keys x 128 channels) or the V^T rows of one chunk (128 channels x 32 keys) - and a
//     key tile is the unit sequence K_0 .. K_NC-1, V_0 .. V_NC-1: S accumulates over the K units in the MFMA accumulators, the softmax runs once behind K_NC-1, and
//     every V unit produces its 128 rows of O^T from the same P fragments.  NS = 4 stages: three units in flight while one is consumed;
//   * the head dim is padded per 32-channel k-step / 16-row block with zero-page chunks and steps past d are branched over (wave-uniform), so only one MFMA shape is
//     issued and a head dim of 8 pays for one k-step, not for a chunk;
//   * Q' stays resident (16-bit fragments, or hi + lo), O^T is the full head: NC = 4 is 128 QT accumulator registers - the wide files are built with AGPR
//     accumulators (_build.AGPR_SOURCES) and one workgroup per CU;
//   * l is added up on the VALU per lane from the ROUNDED probabilities (16-bit: the values the PV product sees; tier: hi(p) + lo(p)) and folded over the four quads
//     of a query column in the epilogue, as in attention_f32x3.hip: no row of ones, no -m in a padding slot (m is never rounded to 16 bits here);
//   * every lane issues every DMA of a unit (lanes outside the data fetch 16 bytes of the zero page), so the counted wait is a compile-time number;
//   * CAUSAL: a masked score is -inf before the maximum, so it enters neither m nor l; key 0 is visible to every query, so the first block fixes a finite m
//     for every row; key tiles wholly above the query block's last query are not visited (workgroup-uniform, the barriers stay matched).
// Budgets (compiler resource report) and timings: profiles/wide_attention.txt.
#pragma once
#include "attention_common.h"      // fyca::AttnP, glds16, wait_vmcnt, RESCALE_THR
#include "split_bf16.h"            // sb::Split, split8, split8_sum, mma3; rp::mfma, rows_max, rows_sum, LdsAttr

namespace fyca {

// ---- what the kernel asks of an element family
template <typename T> struct Wide16 {
  typedef T Elem;
  typedef typename Pair16<T>::Vec8 Op;        // one MFMA operand: 8 consecutive k values
  static constexpr int EPC = 8;                // elements per 16-byte chunk
  static constexpr int KPC = 17;               // K unit: row pitch in chunks (16 of data + 1: odd pitch spreads a fragment read's 16 key rows over the banks)
  static constexpr int VCPR = 4;               // V^T unit: chunks per channel row (32 keys); rows are 64 B, a fragment read of 16 rows x 4 quads is lane-linear
  __device__ static __forceinline__ int v_chunk(int, int c) { return c; }
  __device__ static __forceinline__ Op load_q(const T* src, float sl2e) {       // 8 channels of q, times f32(scale * log2e), rounded to T
    float v[8];
    load8<T>(src, v);
    u32x4 pk;
#pragma unroll
    for (int i = 0; i < 4; ++i) pk[i] = Pair16<T>::pack(v[2 * i] * sl2e, v[2 * i + 1] * sl2e);
    return __builtin_bit_cast(Op, pk);
  }
  __device__ static __forceinline__ Op k_frag(const char* krow, int ks, int g) { return *reinterpret_cast<const Op*>(krow + (4 * ks + g) * 16); }
  __device__ static __forceinline__ Op v_frag(const char* sV, int vrow, int g) { return *reinterpret_cast<const Op*>(sV + vrow * 64 + g * 16); }
  __device__ static __forceinline__ f32x4 mma(const Op& a, const Op& b, f32x4 c) { return rp::mfma(a, b, c); }
  // P^T operand of 8 keys, rounded to T; l += the rounded values (what the PV product multiplies)
  __device__ static __forceinline__ Op make_p(f32x4 p0, f32x4 p1, float& l) {
    u32x4 pk = {Pair16<T>::pack(p0[0], p0[1]), Pair16<T>::pack(p0[2], p0[3]), Pair16<T>::pack(p1[0], p1[1]), Pair16<T>::pack(p1[2], p1[3])};
#pragma unroll
    for (int i = 0; i < 4; ++i) l += Pair16<T>::lo(pk[i]) + Pair16<T>::hi(pk[i]);
    return __builtin_bit_cast(Op, pk);
  }
};
template <typename T> struct WideFam;
template <> struct WideFam<bf16_t> : Wide16<bf16_t> {};
template <> struct WideFam<f16_t> : Wide16<f16_t> {};
template <> struct WideFam<float> {
  typedef float Elem;
  typedef sb::Split Op;
  static constexpr int EPC = 4;
  static constexpr int KPC = 33;               // 32 chunks of data + 1
  static constexpr int VCPR = 8;               // 128-byte rows, chunk XOR row & 7 (attention_f32x3.hip)
  __device__ static __forceinline__ int v_chunk(int row, int c) { return c ^ (row & 7); }
  __device__ static __forceinline__ Op load_q(const float* src, float sl2e) {   // one f32 rounding, then the split
    f32x4 x0 = *reinterpret_cast<const f32x4*>(src), x1 = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { x0[i] *= sl2e; x1[i] *= sl2e; }
    return sb::split8(x0, x1);
  }
  __device__ static __forceinline__ Op k_frag(const char* krow, int ks, int g) {
    return sb::split8(*reinterpret_cast<const f32x4*>(krow + (8 * ks + 2 * g) * 16), *reinterpret_cast<const f32x4*>(krow + (8 * ks + 2 * g + 1) * 16));
  }
  __device__ static __forceinline__ Op v_frag(const char* sV, int vrow, int g) {
    const char* vr = sV + vrow * 128;
    return sb::split8(*reinterpret_cast<const f32x4*>(vr + (((2 * g) ^ (vrow & 7)) * 16)), *reinterpret_cast<const f32x4*>(vr + (((2 * g + 1) ^ (vrow & 7)) * 16)));
  }
  __device__ static __forceinline__ f32x4 mma(const Op& a, const Op& b, f32x4 c) { return sb::mma3(a, b, c); }
  __device__ static __forceinline__ Op make_p(f32x4 p0, f32x4 p1, float& l) { return sb::split8_sum(p0, p1, l); }      // l += hi(p) + lo(p)
};

// LDS geometry of the ring, shared by the kernel and its launcher
template <typename T>
struct WideGeo {
  typedef WideFam<T> F;
  static constexpr int KB = 32, CW = 128, NS = 4;
  static constexpr int K_CHUNKS = KB * F::KPC, V_CHUNKS = CW * F::VCPR;
  static constexpr int LOADS = ((K_CHUNKS > V_CHUNKS ? K_CHUNKS : V_CHUNKS) + 255) / 256;      // DMA instructions per unit and wave
  static constexpr int STAGE = LOADS * 256 * 16;
  static constexpr int LDS_BYTES = NS * STAGE;
};

// NC: 128-channel chunks of the head dim = ceil(d / 128).  QT: 16-query tiles per wave.
template <typename T, int NC, bool CAUSAL, int QT>
__global__ void __launch_bounds__(256) fyc_attn_wide_kernel(const AttnP p) {
  typedef WideFam<T> F;
  typedef WideGeo<T> G;
  typedef typename F::Op Op;
  constexpr int KB = G::KB, CW = G::CW, NS = G::NS, LOADS = G::LOADS, STAGE = G::STAGE, K_CHUNKS = G::K_CHUNKS, V_CHUNKS = G::V_CHUNKS;
  constexpr int EPC = F::EPC, KPC = F::KPC, VCPR = F::VCPR;
  constexpr int UNITS = 2 * NC;                // per key tile
  static_assert((NS - 2) * LOADS <= 15, "the counted wait is an immediate");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, r16 = lane & 15;

  // block -> (bh, query block); all query blocks of one (b, h) on one XCD (attention_kernel.h)
  const int BH = p.batch * p.heads;
  int bh, qb;
  if ((BH & 7) == 0) {
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    bh = (j / p.nqb) * 8 + xcd;
    qb = j % p.nqb;
  } else {
    bh = blockIdx.x / p.nqb;
    qb = blockIdx.x % p.nqb;
  }
  const int b = bh / p.heads, h = bh - b * p.heads;
  const int kvb = (b / p.kv_batch_div) * p.heads + h;
  const int bh_q = p.q_batch_mod > 0 ? (b % p.q_batch_mod) * p.heads + h : bh;
  const T* Q = reinterpret_cast<const T*>(p.q) + (long long)bh_q * p.n_q * p.d;
  const T* K = reinterpret_cast<const T*>(p.k) + (long long)kvb * p.n_k * p.d;
  const T* VT = reinterpret_cast<const T*>(p.vt) + (long long)kvb * p.d * p.ldvt;
  const char* zero = p.zero;
  int ntiles = (p.n_k + KB - 1) / KB;
  if (CAUSAL) {                                // tiles whose first key lies behind the block's last query hold no visible key (n_q == n_k)
    const int q_last = min((qb + 1) * (64 * QT), p.n_q) - 1;
    ntiles = min(ntiles, q_last / KB + 1);
  }
  const int units = ntiles * UNITS;

  // ---- unit loader.  LDS chunk L = it * 256 + tid of a stage.  K unit c: L < K_CHUNKS is chunk L % KPC (EPC channels from 128 c + EPC (L % KPC)) of key row
  // L / KPC.  V^T unit c: L < V_CHUNKS is key chunk v_chunk(row, L % VCPR) of channel row L / VCPR (channel 128 c + row).  Everything else - pad chunks, channels
  // >= d, keys >= n_k of K, keys >= ldvt of V^T - is 16 bytes of the zero page.  V^T is read up to ldvt: finite pad keys, times p = 0.
  auto issue = [&](int tile, int j, int stage) {
    char* sS = smem + stage * STAGE;
    const int key0 = tile * KB;
    if (j < NC) {
      const int ch0 = j * CW;
#pragma unroll
      for (int it = 0; it < LOADS; ++it) {
        const int L = it * 256 + tid, row = L / KPC, cc = L - row * KPC;
        const int key = key0 + row, ch = ch0 + cc * EPC;
        const void* src = zero;
        if (L < K_CHUNKS && cc < KPC - 1 && key < p.n_k && ch < p.d) src = K + (long long)key * p.d + ch;
        glds16(src, sS + (it * 256 + wave * 64) * 16);
      }
    } else {
      const int ch0 = (j - NC) * CW;
#pragma unroll
      for (int it = 0; it < LOADS; ++it) {
        const int L = it * 256 + tid, row = L / VCPR, c = F::v_chunk(row, L & (VCPR - 1));
        const int key = key0 + c * EPC, ch = ch0 + row;
        const void* src = zero;
        if (L < V_CHUNKS && ch < p.d && key < p.ldvt) src = VT + (long long)ch * p.ldvt + key;
        glds16(src, sS + (it * 256 + wave * 64) * 16);
      }
    }
  };
#pragma unroll
  for (int u = 0; u < NS - 1; ++u)
    if (u < units) issue(u / UNITS, u % UNITS, u);

  // ---- Q' fragments (B operand), resident: lane (query = r16, quad g) holds Q'[query][32 kk + 8 g .. +8]
  const int qbase = qb * (64 * QT) + wave * (16 * QT);
  Op qf[QT][4 * NC];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int query = qbase + qt * 16 + r16;
#pragma unroll
    for (int kk = 0; kk < 4 * NC; ++kk) {
      const int dd = 32 * kk + 8 * g;
      const bool ok = query < p.n_q && dd < p.d;
      qf[qt][kk] = F::load_q(ok ? Q + (long long)query * p.d + dd : reinterpret_cast<const T*>(zero), p.sl2e);
    }
  }

  f32x4 o[QT][8 * NC];
  float m_run[QT], l_run[QT];     // running max (log2 units), this LANE's share of the row sum (its 8 keys of every block)
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    m_run[qt] = 0.f;
    l_run[qt] = 0.f;
#pragma unroll
    for (int dv = 0; dv < 8 * NC; ++dv) o[qt][dv] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  bool started = false;           // the first key block always fixes the running max (scores may sit anywhere)

  int st_c = 0, st_i = NS - 1, u = 0;
  for (int tile = 0; tile < ntiles; ++tile) {
    f32x4 s[2][QT];
    Op pf[QT];
#pragma unroll
    for (int j = 0; j < UNITS; ++j, ++u) {
      // unit u landed; up to NS - 2 later ones may stay in flight (every lane issues all LOADS DMAs of a unit)
      const int after = min(NS - 2, units - 1 - u);
      if (after >= 2) wait_vmcnt<2 * LOADS>();
      else if (after == 1) wait_vmcnt<LOADS>();
      else wait_vmcnt<0>();
      __builtin_amdgcn_s_barrier();
      if (u + NS - 1 < units) {    // the stage freed by unit u - 1 takes unit u + NS - 1
        issue(tile + (j + NS - 1) / UNITS, (j + NS - 1) % UNITS, st_i);
        st_i = (st_i + 1 == NS) ? 0 : st_i + 1;
      }
      const char* sU = smem + st_c * STAGE;
      st_c = (st_c + 1 == NS) ? 0 : st_c + 1;

      if (j < NC) {
        // ---- S^T += K_j Q'_j^T: score tile t row i <-> key 8 (i >> 2) + 4 t + (i & 3), so that the lane holds keys 8 g .. 8 g + 7 of query r16 in s[0], s[1]
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const char* kr = sU + (8 * (r16 >> 2) + 4 * t + (r16 & 3)) * (KPC * 16);
#pragma unroll
          for (int qt = 0; qt < QT; ++qt)
            if (j == 0) s[t][qt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            if (j * CW + 32 * ks >= p.d) continue;      // wave-uniform: k-steps past the head dim
            const Op kf = F::k_frag(kr, ks, g);        // read (and split) once, used by all QT query tiles
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) s[t][qt] = F::mma(kf, qf[qt][4 * (j < NC ? j : 0) + ks], s[t][qt]);
          }
        }
        if (j == NC - 1) {
          // ---- online softmax in f32; lane holds keys tile * 32 + 8 g + 4 t + r of query r16
          float mx[QT];        // this LANE's maximum over its 8 keys (the other three quads of the query column hold the other 24)
          const bool tail = tile * KB + KB > p.n_k;
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) {
            if (CAUSAL || tail) {
              const int query = qbase + qt * 16 + r16;
#pragma unroll
              for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  const int key = tile * KB + 8 * g + 4 * t + r;
                  if (key >= p.n_k || (CAUSAL && key > query)) s[t][qt][r] = -INFINITY;
                }
            }
            const float m0 = fmaxf(fmaxf(s[0][qt][0], s[0][qt][1]), fmaxf(s[0][qt][2], s[0][qt][3]));
            const float m1 = fmaxf(fmaxf(s[1][qt][0], s[1][qt][1]), fmaxf(s[1][qt][2], s[1][qt][3]));
            mx[qt] = fmaxf(m0, m1);
          }
          // does ANY lane of the wave see a score above its running max + THR?  (wave-uniform: the rescale runs in the first tiles only)
          bool move = !started;
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) move = move || (mx[qt] > m_run[qt] + RESCALE_THR);
          if (__builtin_amdgcn_ballot_w64(move) != 0) {
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
              const float mq = rp::rows_max(mx[qt]);      // the four quads of a query column agree (fyc_common.h: never fmaxf over the builtin's two results)
              const bool mv = !started || (mq > m_run[qt] + RESCALE_THR);
              const float m_new = mv ? mq : m_run[qt];
              const float alpha = started ? __builtin_amdgcn_exp2f(m_run[qt] - m_new) : 1.0f;      // first block: O^T and l are 0
              m_run[qt] = m_new;
              l_run[qt] *= alpha;
#pragma unroll
              for (int dv = 0; dv < 8 * NC; ++dv) { o[qt][dv][0] *= alpha; o[qt][dv][1] *= alpha; o[qt][dv][2] *= alpha; o[qt][dv][3] *= alpha; }
            }
            started = true;
          }
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) {      // P^T operand: k-slot i <-> key 8 g + i; unnormalised
            f32x4 p0, p1;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              p0[r] = __builtin_amdgcn_exp2f(s[0][qt][r] - m_run[qt]);
              p1[r] = __builtin_amdgcn_exp2f(s[1][qt][r] - m_run[qt]);
            }
            pf[qt] = F::make_p(p0, p1, l_run[qt]);
          }
        }
      } else {
        // ---- O^T rows of chunk j - NC += V^T P^T: lane (channel 16 dv + r16 of the chunk, quad g) reads V^T[channel][keys 8 g .. 8 g + 7]
        const int c = j >= NC ? j - NC : 0;             // (the other branch is compiled for every j of the unrolled loop)
#pragma unroll
        for (int dv = 0; dv < 8; ++dv) {
          if (c * CW + 16 * dv >= p.d) continue;        // wave-uniform: row blocks past the head dim
          const Op vf = F::v_frag(sU, dv * 16 + r16, g);
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) o[qt][8 * c + dv] = F::mma(vf, pf[qt], o[qt][8 * c + dv]);
        }
      }
    }
  }

  // ---- epilogue: lane holds O[query r16][16 dv + 4 g + r]; l is folded over the four quads of the query column
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const float l = rp::rows_sum(l_run[qt]);
    const float inv = 1.0f / l;
    const int query = qbase + qt * 16 + r16;
    if (query >= p.n_q) continue;
    T* orow = reinterpret_cast<T*>(p.o) + ((long long)b * p.n_q + query) * p.ldo + h * p.d;
#pragma unroll
    for (int dv = 0; dv < 8 * NC; ++dv) {
      const int dd = dv * 16 + 4 * g;
      if (dd >= p.d) continue;
      float v[4] = {o[qt][dv][0] * inv, o[qt][dv][1] * inv, o[qt][dv][2] * inv, o[qt][dv][3] * inv};
      if (p.o_accumulate) {
        float prev[4];
        ElemIO<T>::ld4(orow + dd, prev);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = prev[r] + p.o_scale * v[r];
      }
      ElemIO<T>::st4(orow + dd, v);
    }
  }
}

template <typename T, int NC, bool CAUSAL, int QT>
int launch_wide(const AttnP& p0, hipStream_t st) {
  constexpr int LDS_BYTES = WideGeo<T>::LDS_BYTES;
  static_assert(LDS_BYTES <= 160 * 1024, "the ring fits one CU");
  FYC_REQUIRE(rp::lds_fits(LDS_BYTES), "fyc_attention (wide / causal): %d bytes of LDS do not fit this device", LDS_BYTES);
  if constexpr (LDS_BYTES > 64 * 1024) {
    static rp::LdsAttr attr;                          // one per instantiation
    if (int rc = attr.set("fyc_attention (wide / causal)", LDS_BYTES, fyc_attn_wide_kernel<T, NC, CAUSAL, QT>)) return rc;
  }
  AttnP p = p0;
  p.nqb = (p.n_q + 64 * QT - 1) / (64 * QT);
  hipLaunchKernelGGL((fyc_attn_wide_kernel<T, NC, CAUSAL, QT>), dim3((unsigned)(p.batch * p.heads * p.nqb)), dim3(256), LDS_BYTES, st, p);
  FYC_CHECK_LAUNCH("fyc_attention (wide / causal)");
  return 0;
}

// Queries per wave = 16 QT: two tiles share every K / V^T fragment read (and, in the tier, its split).  From three chunks on there is one tile: with two, Q' and O^T
// (16-bit: 2 x 64 + 2 x 128 registers at d = 512, the tier twice the Q') spill - 208 to 904 bytes of scratch per lane in the 16-bit build, which the budget of zero
// scratch refuses (profiles/wide_attention.txt section 1).
template <typename T, int NC> constexpr int wide_qt() { return NC >= 3 ? 1 : 2; }

// fyc_attention (attention.hip) has checked pointers, sizes, head dim, pitches, kv_batch_div, q_batch_mod, causal and the zero page, and has filled p.
// One translation unit per element family instantiates this: attention_wide.hip, attention_wide_f16.hip, attention_wide_f32x3.hip.
template <typename T>
int run_wide_impl(const AttnP& p, bool causal, hipStream_t st) {
  FYC_REQUIRE(rp::aligned16(p.q, p.k, p.vt, p.o), "fyc_attention: causal / d > 160 needs 16-byte aligned q, k, vt and o");
  switch ((p.d + 127) / 128) {
    case 1: if (causal) return launch_wide<T, 1, true, wide_qt<T, 1>()>(p, st); break;      // without the mask d <= 160 is attention_kernel.h's / attention_f32x3.hip's
    case 2: return causal ? launch_wide<T, 2, true, wide_qt<T, 2>()>(p, st) : launch_wide<T, 2, false, wide_qt<T, 2>()>(p, st);
    case 3: return causal ? launch_wide<T, 3, true, wide_qt<T, 3>()>(p, st) : launch_wide<T, 3, false, wide_qt<T, 3>()>(p, st);
    case 4: return causal ? launch_wide<T, 4, true, wide_qt<T, 4>()>(p, st) : launch_wide<T, 4, false, wide_qt<T, 4>()>(p, st);
  }
  FYC_FAIL(-2, "fyc_attention: head dim %d not built", p.d);
}

int run_wide_bf16(const AttnP& p, bool causal, hipStream_t st);      // attention_wide.hip
int run_wide_f16(const AttnP& p, bool causal, hipStream_t st);       // attention_wide_f16.hip
int run_wide_f32x3(const AttnP& p, bool causal, hipStream_t st);     // attention_wide_f32x3.hip

}  // namespace fyca
