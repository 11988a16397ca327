// Fused flash attention on f32 tensors with split-bf16 products (fyc_attn_args::f32_products = FYC_PRODUCTS_SPLIT_BF16, include/fyc.h): the work split and
// the MFMA orientation of attention_kernel.h - a workgroup of 4 wave64 on 64 QT queries of one (batch, head), K and V^T key tiles global -> LDS by
// global_load_lds into a 3-deep ring with counted vmcnt waits, S^T = K Q^T so that a lane's 8 exponentiated scores of a 32-key block are the B operand of
// O^T = V^T P^T - with f32 storage: every operand fragment is split in registers behind its LDS read into hi = RNE_bf16(x) and lo = RNE_bf16(x - hi)
// (split_bf16.h: the rule, shared with temporal_attn_f32x3.hip) and every matrix instruction of the 16-bit kernel becomes three, lo hi, hi lo, hi hi.
//
// What does not carry over from the 16-bit kernel, and what the budgets decided (resource report and timings: profiles/f32x3_attention.txt):
//   * no -m in a padding slot of the head dim (that trick rounds m to bf16): t - m is an f32 subtraction;
//   * l = sum_j hi(p) + lo(p) is added up on the VALU per lane (a lane owns 8 keys of a block) and folded over the four quads of a query column once, in
//     the epilogue: no row of ones in the V^T tile, the tile holds the head's channels only;
//   * the head dim is padded to a multiple of 32 (zero-page chunks in the K tile): only v_mfma_f32_16x16x32_bf16 is issued, there is no 16-wide tail
//     step and therefore no mixed-width accumulation chain (DESIGN.md "Spatial attention": the missing wait state of hipcc 7.2);
//   * key tiles are 32 keys high for every head dim: an f32 tile is twice the bytes of a 16-bit one, and at 32 keys three ring stages are 48 KB at d = 40,
//     60 KB at d = 64, 72 KB at d = 80 and 132 KB at d = 160 - two or three workgroups per CU up to d = 80, one above (rp::LdsAttr above 64 KB);
//   * Q is split once per wave and stays resident as hi + lo; a K or V^T fragment is split once per key block and serves all QT query tiles: QT = 4 is built
//     up to d = 80 and pays 3 - 4 % at 4096 queries (the dispatch rule and its measurement: fyca::run_f32x3 below);
//   * every lane issues every DMA of a tile (lanes outside the data fetch 16 bytes of the zero page), so the counted wait is a compile-time number.
#include "attention_common.h"      // fyca::AttnP (filled by fyc_attention, attention.hip), glds16, wait_vmcnt, RESCALE_THR
#include "split_bf16.h"            // sb::Split, split8, split8_sum, mma3: the rule

namespace {

using namespace sb;
using fyca::AttnP, fyca::glds16, fyca::wait_vmcnt, fyca::RESCALE_THR;

// LDS geometry of one ring stage, shared by the kernel and its launcher.  K tile: KB keys x (DP / 4 + 1) 16-byte chunks (4 channels each; the odd pitch
// spreads the 16 key rows of a fragment read over the banks), directly behind it the V^T tile: DVT * 16 channel rows x 8 chunks (4 keys each), chunk XOR row & 7.
// The two tiles share one chunk index space, so that the 256-lane DMA rounds are rounded up once per stage, not once per tile.
template <int DP32, int DVT>
struct Geo {
  static constexpr int KB = 32;
  static constexpr int PC = DP32 * 8 + 1;
  static constexpr int K_CHUNKS = KB * PC, V_CHUNKS = DVT * 16 * 8;
  static constexpr int LOADS = (K_CHUNKS + V_CHUNKS + 255) / 256;      // DMA instructions per tile and wave
  static constexpr int STAGE = LOADS * 256 * 16, NS = 3;
  static constexpr int LDS_BYTES = NS * STAGE;
};

// DP32: head dim padded to 32-channel k-steps.  DVT: 16-row blocks of O^T = ceil(d / 16).  QT: 16-query tiles per wave.
template <int DP32, int DVT, int QT>
__global__ void __launch_bounds__(256) fyc_attn_f32x3_kernel(const AttnP p) {
  typedef Geo<DP32, DVT> G;
  constexpr int KS = DP32, KB = G::KB, PC = G::PC, K_CHUNKS = G::K_CHUNKS, STAGE = G::STAGE, LOADS = G::LOADS, NS = G::NS;
  static_assert(LOADS <= 15, "the counted wait is an immediate");
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
  const float* Q = reinterpret_cast<const float*>(p.q) + (long long)bh_q * p.n_q * p.d;
  const float* K = reinterpret_cast<const float*>(p.k) + (long long)kvb * p.n_k * p.d;
  const float* VT = reinterpret_cast<const float*>(p.vt) + (long long)kvb * p.d * p.ldvt;
  const char* zero = p.zero;
  const int ntiles = (p.n_k + KB - 1) / KB;
  const int nfull = p.n_k / KB;            // tiles 0 .. nfull-1 hold KB keys
  const int dchunks = p.d >> 2;            // 16-byte chunks of a K row that hold data

  // ---- K / V^T tile loader.  LDS chunk L = it * 256 + tid of a stage: L < K_CHUNKS is chunk L % PC of key row L / PC, the others are V^T chunks.  What a
  // lane fetches in a FULL tile is a fixed byte offset from the tile's K or V^T base (NODATA: a pad chunk, a channel >= d, a chunk beyond the tiles - 16
  // bytes of the zero page, the longest read of a masked lane)
  constexpr unsigned NODATA = 0xffffffffu;
  unsigned off[LOADS];
#pragma unroll
  for (int it = 0; it < LOADS; ++it) {
    const int L = it * 256 + tid;
    if (L < K_CHUNKS) {
      const int row = L / PC, cc = L - row * PC;
      off[it] = cc < dchunks ? (unsigned)(row * p.d + cc * 4) * 4u : NODATA;
    } else {
      const int Lv = L - K_CHUNKS, row = Lv >> 3, c = (Lv & 7) ^ (row & 7);
      off[it] = row < p.d ? (unsigned)(row * p.ldvt + c * 4) * 4u : NODATA;
    }
  }
  auto issue = [&](int tile, int stage) {
    char* sS = smem + stage * STAGE;
    if (tile < nfull) {
      const char* kb = reinterpret_cast<const char*>(K) + (long long)tile * (KB * 4) * p.d;
      const char* vb = reinterpret_cast<const char*>(VT) + (long long)tile * (KB * 4);
#pragma unroll
      for (int it = 0; it < LOADS; ++it) {
        const char* base = (it * 256 + tid < K_CHUNKS) ? kb : vb;
        glds16(off[it] != NODATA ? base + off[it] : zero, sS + (it * 256 + wave * 64) * 16);
      }
      return;
    }
    // the ragged last tile: keys >= n_k of K come from the zero page (their scores are masked), V^T is read up to ldvt (finite pad keys, times p = 0)
    const int key0 = tile * KB;
#pragma unroll
    for (int it = 0; it < LOADS; ++it) {
      const int L = it * 256 + tid;
      const void* src = zero;
      if (L < K_CHUNKS) {
        const int row = L / PC, cc = L - row * PC;
        const int key = key0 + row;
        if (key < p.n_k && cc < dchunks) src = K + (long long)key * p.d + cc * 4;
      } else {
        const int Lv = L - K_CHUNKS, row = Lv >> 3, c = (Lv & 7) ^ (row & 7);
        const int key = key0 + c * 4;
        if (row < p.d && key < p.ldvt) src = VT + (long long)row * p.ldvt + key;
      }
      glds16(src, sS + (it * 256 + wave * 64) * 16);
    }
  };
  issue(0, 0);
  if (ntiles > 1) issue(1, 1);

  // ---- Q fragments (B operand), pre-scaled by f32(scale * log2(e)) with one f32 rounding, split once: lane (query = r16, quad g) holds
  //      Q'[query][32 ks + 8 g .. +8] as hi and lo
  const int qbase = qb * (64 * QT) + wave * (16 * QT);
  Split qf[QT][KS];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int query = qbase + qt * 16 + r16;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int dd = 32 * ks + 8 * g;
      const bool ok = query < p.n_q && dd < p.d;
      const float* src = Q + (long long)query * p.d + dd;
      f32x4 x0 = *reinterpret_cast<const f32x4*>(ok ? src : reinterpret_cast<const float*>(zero));
      f32x4 x1 = *reinterpret_cast<const f32x4*>(ok ? src + 4 : reinterpret_cast<const float*>(zero));
#pragma unroll
      for (int i = 0; i < 4; ++i) { x0[i] *= p.sl2e; x1[i] *= p.sl2e; }
      qf[qt][ks] = split8(x0, x1);
    }
  }

  f32x4 o[QT][DVT];
  float m_run[QT], l_run[QT];     // running max (log2 units), this LANE's share of the row sum (its 8 keys of every block)
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    m_run[qt] = 0.f;
    l_run[qt] = 0.f;
#pragma unroll
    for (int dv = 0; dv < DVT; ++dv) o[qt][dv] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  bool started = false;           // the first key block always fixes the running max (scores may sit anywhere)

  int st_c = 0, st_i = (ntiles > 1) ? 2 : 1;
  for (int tile = 0; tile < ntiles; ++tile) {
    // tile landed; the next one may stay in flight (every lane issues all LOADS DMAs of a tile)
    if (tile + 1 < ntiles) wait_vmcnt<LOADS>();
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (tile + 2 < ntiles) { issue(tile + 2, st_i); st_i = (st_i + 1 == NS) ? 0 : st_i + 1; }
    const char* sK = smem + st_c * STAGE;
    const char* sV = sK + K_CHUNKS * 16;
    st_c = (st_c + 1 == NS) ? 0 : st_c + 1;

    // ---- S^T = K Q'^T: score tile t row i <-> key 8 (i >> 2) + 4 t + (i & 3), so that the lane holds keys 8 g .. 8 g + 7 of query r16 in s[0], s[1]
    f32x4 s[2][QT];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const char* kr = sK + (8 * (r16 >> 2) + 4 * t + (r16 & 3)) * (PC * 16);
      Split kf[KS];             // one key tile's fragments at a time, split once, used by all QT query tiles
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(kr + (8 * ks + 2 * g) * 16);
        const f32x4 x1 = *reinterpret_cast<const f32x4*>(kr + (8 * ks + 2 * g + 1) * 16);
        kf[ks] = split8(x0, x1);
      }
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        s[t][qt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) s[t][qt] = mma3(kf[ks], qf[qt][ks], s[t][qt]);
      }
    }

    // ---- online softmax in f32; lane holds keys tile * 32 + 8 g + 4 t + r of query r16
    float mx[QT];        // this LANE's maximum over its 8 keys (the other three quads of the query column hold the other 24)
    const bool tail = tile * KB + KB > p.n_k;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      if (tail) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (tile * KB + 8 * g + 4 * t + r >= p.n_k) s[t][qt][r] = -INFINITY;
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
        const float mq = rp::rows_max(mx[qt]);      // the four quads of a query column agree (v_permlane swaps, fyc_common.h: never fmaxf over the builtin's two results)
        const bool mv = !started || (mq > m_run[qt] + RESCALE_THR);
        const float m_new = mv ? mq : m_run[qt];
        const float alpha = started ? __builtin_amdgcn_exp2f(m_run[qt] - m_new) : 1.0f;      // first block: O^T and l are 0
        m_run[qt] = m_new;
        l_run[qt] *= alpha;
#pragma unroll
        for (int dv = 0; dv < DVT; ++dv) { o[qt][dv][0] *= alpha; o[qt][dv][1] *= alpha; o[qt][dv][2] *= alpha; o[qt][dv][3] *= alpha; }
      }
      started = true;
    }
    Split pf[QT];        // P^T operand: k-slot j <-> key 8 g + j; unnormalised, split
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      f32x4 p0, p1;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p0[r] = __builtin_amdgcn_exp2f(s[0][qt][r] - m_run[qt]);
        p1[r] = __builtin_amdgcn_exp2f(s[1][qt][r] - m_run[qt]);
      }
      pf[qt] = split8_sum(p0, p1, l_run[qt]);
    }

    // ---- O^T += V^T P^T: lane (channel 16 dv + r16, quad g) reads V^T[channel][keys 8 g .. 8 g + 7]
#pragma unroll
    for (int dv = 0; dv < DVT; ++dv) {
      const int vrow = dv * 16 + r16;
      const char* vr = sV + vrow * 128;
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(vr + (((2 * g) ^ (vrow & 7)) * 16));
      const f32x4 x1 = *reinterpret_cast<const f32x4*>(vr + (((2 * g + 1) ^ (vrow & 7)) * 16));
      const Split vf = split8(x0, x1);
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) o[qt][dv] = mma3(vf, pf[qt], o[qt][dv]);
    }
  }

  // ---- epilogue: lane holds O[query r16][16 dv + 4 g + r]; l is folded over the four quads of the query column
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const float l = rp::rows_sum(l_run[qt]);
    const float inv = 1.0f / l;
    const int query = qbase + qt * 16 + r16;
    if (query >= p.n_q) continue;
    float* orow = reinterpret_cast<float*>(p.o) + ((long long)b * p.n_q + query) * p.ldo + h * p.d;
#pragma unroll
    for (int dv = 0; dv < DVT; ++dv) {
      const int dd = dv * 16 + 4 * g;
      if (dd >= p.d) continue;
      f32x4 v = {o[qt][dv][0] * inv, o[qt][dv][1] * inv, o[qt][dv][2] * inv, o[qt][dv][3] * inv};
      if (p.o_accumulate) {
        const f32x4 prev = *reinterpret_cast<const f32x4*>(orow + dd);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = prev[r] + p.o_scale * v[r];
      }
      *reinterpret_cast<f32x4*>(orow + dd) = v;
    }
  }
}

template <int DP32, int DVT, int QT>
int launch_k(const AttnP& p0, hipStream_t st) {
  constexpr int LDS_BYTES = Geo<DP32, DVT>::LDS_BYTES;
  static_assert(LDS_BYTES <= 160 * 1024, "the ring fits one CU");
  FYC_REQUIRE(rp::lds_fits(LDS_BYTES), "fyc_attention(f32, split products): %d bytes of LDS do not fit this device", LDS_BYTES);
  if constexpr (LDS_BYTES > 64 * 1024) {
    static rp::LdsAttr attr;                          // one per instantiation
    if (int rc = attr.set("fyc_attention(f32, split products)", LDS_BYTES, fyc_attn_f32x3_kernel<DP32, DVT, QT>)) return rc;
  }
  AttnP p = p0;
  p.nqb = (p.n_q + 64 * QT - 1) / (64 * QT);
  hipLaunchKernelGGL((fyc_attn_f32x3_kernel<DP32, DVT, QT>), dim3((unsigned)(p.batch * p.heads * p.nqb)), dim3(256), LDS_BYTES, st, p);
  FYC_CHECK_LAUNCH("fyc_attention(f32, split products)");
  return 0;
}

template <int DP32, int DVT>
int launch_q(const AttnP& p, int qt, hipStream_t st) {
  if constexpr (DVT <= 5) {      // d <= 80
    if (qt == 4) return launch_k<DP32, DVT, 4>(p, st);
  }
  return launch_k<DP32, DVT, 2>(p, st);
}

}  // namespace

// fyc_attention has checked pointers, sizes, head dim, pitches, kv_batch_div, q_batch_mod and the zero page, and has filled p
int fyca::run_f32x3(const AttnP& p, hipStream_t st) {
  FYC_REQUIRE(rp::aligned16(p.q, p.k, p.vt, p.o), "fyc_attention: f32_products = FYC_PRODUCTS_SPLIT_BF16 needs 16-byte aligned q, k, vt and o");
  FYC_REQUIRE((long long)p.d * p.ldvt * 4 < (1ll << 32), "fyc_attention: f32_products = FYC_PRODUCTS_SPLIT_BF16: one head of vt (%d x %d f32) must stay below 4 GiB", p.d, p.ldvt);
  // Queries per wave = 16 QT.  A K / V^T fragment is read and split once per key block and serves QT query tiles: QT = 4 halves the LDS reads and the split's
  // VALU work per matrix instruction, at 230 - 310 registers against 150 - 224 (d = 40 .. 80).  Measured (profiles/f32x3_attention.txt section 2, the two forced
  // with tuning key 3): at 4096 queries QT = 4 takes 0.96 - 0.97 of QT = 2's time (d = 40 and 64, also where 256-query blocks leave CUs without a workgroup);
  // at 1024 it is between 0.98 (d = 80) and 1.08 (d = 64), at 256 level, at 64 queries 1.39 (three waves of four idle).  Hence QT = 4 from 2048 queries on, up to
  // d = 80 (above, Q and O^T of four tiles do not fit the register file beside the fragments: not built).  Tuning key 3 forces 2 or 4.
  int qt = (p.d <= 80 && p.n_q >= 2048) ? 4 : 2;
  if (g_fyc_tuning[FYC_TUNE_ATTN_VARIANT] == 2 || (g_fyc_tuning[FYC_TUNE_ATTN_VARIANT] == 4 && p.d <= 80)) qt = g_fyc_tuning[FYC_TUNE_ATTN_VARIANT];
  switch ((p.d + 15) / 16) {      // 16-row blocks of O^T -> (k-steps of 32 channels, blocks)
    case 1: return launch_q<1, 1>(p, qt, st);
    case 2: return launch_q<1, 2>(p, qt, st);
    case 3: return launch_q<2, 3>(p, qt, st);
    case 4: return launch_q<2, 4>(p, qt, st);
    case 5: return launch_q<3, 5>(p, qt, st);
    case 6: return launch_q<3, 6>(p, qt, st);
    case 7: return launch_q<4, 7>(p, qt, st);
    case 8: return launch_q<4, 8>(p, qt, st);
    case 9: return launch_q<5, 9>(p, qt, st);
    default: return launch_q<5, 10>(p, qt, st);
  }
}
