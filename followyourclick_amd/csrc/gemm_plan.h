// The host side of fyc_gemm, in one place: the kernel-argument struct, the tile table, the launch plan of a problem and the launch decisions of a kernel.
//   GEMM_TILES        every tile config id: geometry, the ring depths and epilogues it is built for.  The kernels are instantiated FROM it (gemm_kernel.h::dispatch_cfg)
//   gemm_executed_cfg the tile a planned config runs as (narrow epilogue, activation family)
//   plan_gemm()       kernel family, tile, ring depth, split-K, epilogue width, statistics layout, workspace of one problem - fyc_gemm executes the plan,
//                     fyc_gemm_workspace_bytes / fyc_gemm_row_parts / fyc_gemm_stat_layout read a field of it
//   gemm_launch_plan() what one launch of one instantiation decides beyond the plan: epilogue forms, tile order, LDS bytes, the persistent grid
// Host only, on fyc_common.h alone (gemm_kernel.h includes this file, not the other way round): pure functions of the scalar fields of their arguments, of
// which pointers are null and how they are aligned, and of g_fyc_tuning; no HIP call, no static state.
//
// A problem that writes output statistics (chan_parts / row_parts) is planned from its shape alone - M, N, K, mode, dtype, batch, tile,
// cs_rows and the tuning table, which is all the layout queries see (the engine sizes its buffers before the call exists).  The actual
// arguments are then checked against that plan, and a call that cannot run it (a folded LayerNorm on a problem that splits, operands
// that rule out the 16-byte epilogue, ...) is REFUSED with the conflict named: never another tile, never a layout nobody announced.
#pragma once
#include "fyc_common.h"

namespace fycg {

// Internal kernel mode beside the public FYC_GEMM_* values (never a value of fyc_gemm_args::mode; host: conv_up_phases.hip): nearest-2x upsampling + 3x3
// convolution as four 2x2 convolutions of the LOW-resolution input, one per output phase (py, px) = parity of the output pixel.  On the upsampled image every
// input pixel appears 2x2 times, so the three filter rows an output pixel (2y + py, 2x + px) touches collapse onto two input rows (py = 0: row y - 1 with
// W[ky=0], row y with W[1] + W[2]; py = 1: row y with W[0] + W[1], row y + 1 with W[2]), columns alike: K = 4 * Cin with weights pre-summed at pack time
// instead of 9 * Cin.  Rows of the problem are VIRTUAL, ordered [group][phase = 2 py + px][row in group]; a group is up_rows consecutive input pixels (whole
// frames: one statistics sample of the consuming GroupNorm), up_rows % BM == 0, so a row tile has one phase and lies in one group.  The A gather is the CONV3X3
// one with 4 taps whose top-left is (y - 1 + py, x - 1 + px) on the Hin x Win image (zero padding maps onto itself); the weights are [4 phases][N][ldw], and the
// epilogue stores virtual row m at the output pixel's row ((frame * 2 Hin + 2 y + py) * 2 Win + 2 x + px).
constexpr int GEMM_MODE_UP_PHASES = 16;

// internal epilogue id: LINEAR with the pointwise activation p.act compiled in.  A separate instantiation so that the
// hot-path LINEAR kernels do not carry the GELU code (it costs the 256x320 tile 80 B/lane of scratch).
constexpr int EPI_LINEAR_ACT = 3;

struct GemmP {
  const char* a; const char* a2; const char* w; const float* bias; const float* rowbias; const char* residual; char* out;
  char* seg_out[3]; int seg_transposed[3]; int seg_ld[3];
  int M, N, K, lda, ldw, ldo, ldr, ldrb, k_split, lda2;
  long long stride_a, stride_w, stride_o;
  int mode, epilogue;
  int Hout, Wout, Hin, Win, Cin, conv_stride, conv_pad;
  int rows_per_batch, seg_cols, heads, tokens, head_dim;
  float out_scale;
  int act;    // FYC_ACT_* (LINEAR epilogue)
  const float* ln_stats; const float* ln_colsum;   // folded LayerNorm (see fyc.h): acc := rstd*(acc - mean*colsum[n])
  int ln_nparts; float ln_eps;                     // ln_nparts > 0: ln_stats holds [M][ln_nparts] partial {sum, sum sq} (row_parts of the producer)
  // statistics of the OUTPUT for the GroupNorm / LayerNorm that consumes it (LINEAR epilogue), see fyc.h
  float* chan_parts; int cs_rows, cs_slots;        // [tiles_m][cs_slots][N][2] = {sum, sum sq} of the stored values per (row tile, sample slot, channel)
  float* row_parts; int row_nparts;                // [M][row_nparts][2] = per row, per column tile {sum, sum sq}
  int tiles_m, tiles_n;
  int strip;  // > 0: tiles are walked in column strips of this many tiles (row-major inside a strip), see tile_coords
  int up_exact2; float up_sh, up_sw;   // nearest-upsample source mapping
  int colc;   // bias / colsum / tile-uniform rowbias may be fetched 16 B at a time and staged through LDS once per tile
  int rb_tile; // rowbias row is the same for every row of a tile (rows_per_batch % BM == 0): folded into the staged bias
  int rb_slots; // bf16 LINEAR wide epilogue: a tile touches up to this many rowbias rows (rows_per_batch % 16 == 0), staged through LDS next to the bias
  int splitk; int t3_frames; float* ws;   // t3_frames: CONV_T3, frames per clip.  split-K (small M, long K): `splitk` work items per output tile, raw f32 partials to ws[splitk][M][N]
  int stagger; // 8-wave tiles: the upper half of the waves issues its DMAs between its two MFMA k-steps (fyc_set_tuning key 5 = 1: off)
  int wide;   // bf16 linear epilogue may use 16-B row accesses (N, ldo, ldr multiples of 8; bias/rowbias 16-B aligned)
  const char* zero;
  int res_acc;   // bf16 LINEAR wide epilogue: the residual tile is loaded INTO the accumulators before the K loop (see epilogue_linear_packed)
  float inv_seg_cols, inv_head_dim;   // HEADS epilogue: reciprocals for fdiv_small (host: fyc_gemm)
  int fast1;   // packed LINEAR epilogue: specialised pass 1 (fyc_set_tuning key 13 = 1: the generic one, A/B)
  int heads_pk; // head-split epilogue: the pack-first form (epilogue_heads_packed) - M <= 8192 only, see gemm_launch_plan()
  int pre;     // round 6: the epilogue's per-row / per-column inputs are already in LDS (issue_consts in fyc_gemm_kernel), see pre_bytes()
  int phase_delay; int t3_rows;   // t3_rows: CONV_T3, rows per frame (H*W).  phase_delay: round 6 (A/B, fyc_set_tuning key 11): every other block of an XCD starts this many x 1024 cycles late, see fyc_gemm_kernel
  unsigned long long* trace;   // timing builds (-DFYC_TRACE, tools/gemm_phase_probe.py): per-block s_memtime stamps; nullptr otherwise
};
// (t3_frames / t3_rows sit in the two alignment holes the struct had: its size and every kernel-argument offset of the older modes stay put)
// (GEMM_MODE_UP_PHASES adds no field either: t3_rows holds its rows per group, up_sw the reciprocal 1 / Win of its output row map)
static_assert(sizeof(GemmP) == 392, "GemmP grew: the kernel-argument offsets of every instantiation move");

// one translation unit per (dtype, family) keeps the build parallel.  `cfg` / `ns` are the PLANNED tile config and ring depth (GemmPlan::cfg / ns): the
// entries resolve what runs through gemm_executed_cfg themselves
int run_bf16_plain(const GemmP& p, int batch, int cfg, int ns, hipStream_t st);
int run_bf16_conv(const GemmP& p, int batch, int cfg, int ns, hipStream_t st);
int run_bf16_act(const GemmP& p, int batch, int cfg, hipStream_t st);   // LINEAR + activation: tile configs 1, 2, 6
int run_f32(const GemmP& p, int batch, int cfg, hipStream_t st);
// f32 storage, split-bf16 products (f32x3_t): gemm_f32x3.hip, gemm_f32x3_t3.hip.  fyc_gemm reaches them through run_f32 / run_f32_t3 with CFG_F32X3 OR-ed into
// `cfg` (like the ring depth in fyc_gemm_args::tile): the product rule is no part of the plan, and the entry points of a (dtype, family) stay one per family
constexpr int CFG_F32X3 = 0x100;
int run_f32x3(const GemmP& p, int batch, int cfg, hipStream_t st);
int run_f32x3_t3(const GemmP& p, int batch, int cfg, hipStream_t st);
// f16 storage (FYC_F16): the same kernels on v_mfma_f32_16x16x32_f16
int run_f16_plain(const GemmP& p, int batch, int cfg, int ns, hipStream_t st);
int run_f16_conv(const GemmP& p, int batch, int cfg, int ns, hipStream_t st);
int run_f16_act(const GemmP& p, int batch, int cfg, hipStream_t st);
// 3-tap convolution along the frame axis (FYC_GEMM_CONV_T3): gemm_{bf16,f16,f32}_t3.hip
int run_bf16_t3(const GemmP& p, int batch, int cfg, int ns, hipStream_t st);
int run_f16_t3(const GemmP& p, int batch, int cfg, int ns, hipStream_t st);
int run_f32_t3(const GemmP& p, int batch, int cfg, hipStream_t st);
// nearest-2x upsample + 3x3 as four 2x2 phase convolutions (GEMM_MODE_UP_PHASES; entry: conv_up_phases.hip): gemm_{bf16,f16}_up.hip
int run_bf16_up_phases(const GemmP& p, int cfg, int ns, hipStream_t st);
int run_f16_up_phases(const GemmP& p, int cfg, int ns, hipStream_t st);

// ---- the tile table -------------------------------------------------------------------------------------------------------------------
// One row per tile config id.  All tiles use the 2-deep ring (deeper rings measured no gain, profiles/r01_gemm_tile_sweep*.txt); config 1 is also built
// 3-deep so that the counted-wait ring logic stays exercised (tests), config 2 3- and 4-deep for the latency-bound small-M linears (8x8 latent level).
// The narrow epilogue (f32 parity mode and 16-bit problems whose shapes / alignment rule out 16-byte accesses) only exists for configs 1 and 2.
//   5: N = 320*k (every layer width of SD-1.5): 320-wide tiles read the A panel once per 320 columns
//   8 / 10: 64-byte K tiles: half the LDS per stage -> two independent 4-wave blocks per CU with 64x160 wave tiles (8)
//   11: round 6: 128x160 over 2x2 waves (64x80 per wave, the wave tile of config 6) with 72 KB of ring: TWO independent workgroups per CU, so one's
//       epilogue / first fill runs under the other's K loop - for the short-K problems whose 128x320 tiles spend as long in the epilogue as in the K loop
//       (profiles/r06_gemm_two_workgroups_ab.txt)
// GEGLU pairs 16-column value / gate blocks inside a wave: configs 6 and 11 give a wave 5 column blocks (128x320 over 2x4 waves) and used to leave the
// output unwritten (found by tools/gemm_diag.py at M = 4096 / 8192, N = 2560 - shapes the UNet never issued): they are not built for it, `geglu` runs.
// RETIRED ids, never built (no wave grid): 12 / 13 / 14, the 32x32x16 main-loop twins of 5 / 7 / 3 (8-12 % slower on every shape,
// profiles/r06_gemm_mi32_ab.txt), and 21 / 22 / 23 / 31, the round-4 main-loop experiments on the tiles of 5 / 6 / 7 / 6
// (profiles/r04_gemm_pingpong_and_prefetch_sweep.txt): a request for one of the latter runs its one-phase `twin` (same tile, same wave grid), as it did in
// every build without them.  Their rows stay so that the layout queries answer as they always did.
enum { GEMM_FAM_PLAIN, GEMM_FAM_CONV, GEMM_FAM_ACT, GEMM_FAM_T3 };   // one translation unit per (dtype, family): run_* above

struct GemmTile {
  int id, bm, bn;            // rows x columns
  int wgm, wgn;              // wave grid (0 x 0: retired, layout only)
  int rb;                    // bytes of K per LDS row (one K tile)
  unsigned rings_plain, rings;   // bit ns: built with an ns-deep ring, in PLAIN mode / in the convolution modes (wide epilogue; narrow: 2 only)
  unsigned epi;              // bit e: built for epilogue e (FYC_EPI_*, EPI_LINEAR_ACT), wide
  bool narrow;               // built with the narrow per-lane epilogue as well (every epilogue, 2-deep)
  int geglu;                 // > 0: a wave owns an odd number of column blocks, GEGLU runs this config instead
  int twin;                  // > 0: retired, a request runs this config
};
constexpr unsigned RING2 = 1u << 2, RING3 = 1u << 3, RING4 = 1u << 4;
constexpr unsigned E_LIN = 1u << FYC_EPI_LINEAR, E_GEGLU = 1u << FYC_EPI_GEGLU, E_HEADS = 1u << FYC_EPI_HEADS, E_ACT = 1u << EPI_LINEAR_ACT;
constexpr GemmTile GEMM_TILES[] = {
    // id bm   bn  waves rb   rings: PLAIN           other modes    epilogues                          narrow geglu twin
    {1,  128, 128, 2, 2, 128, RING2 | RING3,         RING2 | RING3, E_LIN | E_GEGLU | E_HEADS | E_ACT, true,  0,  0},
    {2,  128, 64,  2, 2, 128, RING2 | RING3 | RING4, RING2,         E_LIN | E_GEGLU | E_HEADS | E_ACT, true,  0,  0},
    {3,  256, 128, 4, 2, 128, RING2,                 RING2,         E_LIN | E_GEGLU | E_HEADS,         false, 0,  0},
    {4,  256, 64,  4, 1, 128, RING2,                 RING2,         E_LIN | E_GEGLU | E_HEADS,         false, 0,  0},
    {5,  256, 320, 4, 2, 128, RING2,                 RING2,         E_LIN | E_GEGLU | E_HEADS,         false, 0,  0},
    {6,  128, 320, 2, 4, 128, RING2,                 RING2,         E_LIN | E_HEADS | E_ACT,           false, 5,  0},
    {7,  256, 256, 2, 4, 128, RING2,                 RING2,         E_LIN | E_GEGLU | E_HEADS,         false, 0,  0},
    {8,  128, 320, 2, 2, 64,  RING2,                 RING2,         E_LIN | E_GEGLU | E_HEADS,         false, 0,  0},
    {10, 128, 128, 2, 2, 64,  RING2,                 RING2,         E_LIN | E_GEGLU | E_HEADS,         false, 0,  0},
    {11, 128, 160, 2, 2, 128, RING2,                 RING2,         E_LIN | E_HEADS,                   false, 5,  0},
    {12, 256, 320, 0, 0, 128, 0,                     0,             0,                                 false, 0,  0},
    {13, 256, 256, 0, 0, 128, 0,                     0,             0,                                 false, 0,  0},
    {14, 256, 128, 0, 0, 128, 0,                     0,             0,                                 false, 0,  0},
    {21, 256, 320, 0, 0, 128, 0,                     0,             0,                                 false, 0,  5},
    {22, 128, 320, 0, 0, 128, 0,                     0,             0,                                 false, 21, 6},
    {23, 256, 256, 0, 0, 128, 0,                     0,             0,                                 false, 0,  7},
    {31, 128, 320, 0, 0, 128, 0,                     0,             0,                                 false, 0,  6},
};
constexpr int GEMM_N_TILES = (int)(sizeof(GEMM_TILES) / sizeof(GEMM_TILES[0]));
constexpr GemmTile GEMM_NO_TILE = {0, 128, 128, 0, 0, 128, 0, 0, 0, false, 0, 0};   // an id the table does not know: the layout queries have always answered 128 x 128

constexpr GemmTile gemm_tile(int cfg) {
  for (int i = 0; i < GEMM_N_TILES; ++i)
    if (GEMM_TILES[i].id == cfg) return GEMM_TILES[i];
  return GEMM_NO_TILE;
}
inline int gemm_tile_bm(int cfg) { return gemm_tile(cfg).bm; }
inline int gemm_tile_bn(int cfg) { return gemm_tile(cfg).bn; }
// the table's own consistency: a built tile is refused GEGLU exactly where a wave owns an odd number of 16-column blocks, and has a replacement there
constexpr bool gemm_tiles_consistent() {
  for (int i = 0; i < GEMM_N_TILES; ++i) {
    const GemmTile& t = GEMM_TILES[i];
    if (t.wgm > 0 && ((t.bn / t.wgn / 16) % 2 == 1) != ((t.epi & E_GEGLU) == 0)) return false;
    if (t.wgm > 0 && ((t.epi & E_GEGLU) == 0) != (t.geglu > 0)) return false;
  }
  return true;
}
static_assert(gemm_tiles_consistent(), "GEMM_TILES: GEGLU column and wave grid disagree");

constexpr bool gemm_ring_built(const GemmTile& t, int mode, int ns) { return ns >= 2 && ns <= 4 && (((mode == FYC_GEMM_PLAIN ? t.rings_plain : t.rings) >> ns) & 1u); }

// One instantiation of fyc_gemm_kernel: a tile of the table, ring depth, epilogue width and id, kernel mode, bytes per element.
struct GemmGeom { GemmTile t; int ns; bool wide; int epi, mode, esize; };
// Is it one the library builds?  (dispatch_cfg instantiates exactly these)
constexpr bool gemm_built(const GemmGeom& g) {
  if (g.t.wgm == 0) return false;
  if (!g.wide) return g.t.narrow && g.ns == 2;
  if (g.esize != 2 || !((g.t.epi >> g.epi) & 1u)) return false;
  if (g.epi == EPI_LINEAR_ACT) return g.ns == 2;      // (the activation family takes no ring depth)
  return gemm_ring_built(g.t, g.mode, g.ns);
}
constexpr int RB_SLOTS = 4;     // rowbias rows a tile may touch in the packed LINEAR epilogue (GemmP::rb_slots)
// bytes of the epilogue inputs pre-staged behind the ring (gemm_kernel.h: "epilogue inputs pre-staged by DMA"): [BM] {mean, rstd} | [BN] bias | [BN] column sums | [RB_SLOTS][BN] row-bias rows
constexpr int pre_bytes(int bm, int bn) { return bm * 8 + (2 + RB_SLOTS) * bn * 4; }
constexpr bool gemm_pre_built(const GemmGeom& g) { return g.wide && g.ns == 2; }
constexpr int gemm_lds_bytes(const GemmGeom& g) { return g.ns * (g.t.bm + g.t.bn) * g.t.rb + (gemm_pre_built(g) ? pre_bytes(g.t.bm, g.t.bn) : 0); }

// rowbias rows (batch elements) a row tile of bm rows can touch; 0 = more than the packed LINEAR epilogue stages (fyc_gemm() then takes the narrow epilogue)
inline int rowbias_slots(int bm, int rpb) {
  if (rpb <= 0 || rpb % 16 != 0) return 0;
  const int n = (bm % rpb == 0) ? bm / rpb : (bm - 1) / rpb + 2;
  return n <= RB_SLOTS ? n : 0;
}

// ---- what a planned tile runs as --------------------------------------------------------------------------------------------------------
// The tile config / ring depth the kernels of `family` execute for a PLANNED config (GemmPlan::cfg / ns; a retired id counts as its twin): the narrow
// epilogue only exists for configs 1 and 2, and the activation family (off the denoising hot path: CLIP MLPs, Resampler feed-forward) builds 1, 2 and 6 and
// folds every planned tile onto one of them.  Neither takes a ring depth.  A config that is not built stays itself: the entry refuses it by its number.
inline int gemm_executed_cfg(int family, bool wide, int cfg, int N) {
  if (gemm_tile(cfg).twin > 0) cfg = gemm_tile(cfg).twin;
  if (!wide) return gemm_tile(cfg).narrow ? cfg : (N % 128 == 0 || N > 512) ? 1 : 2;
  if (family == GEMM_FAM_ACT) return (cfg == 6 || cfg == 5) ? 6 : (cfg == 1 || cfg == 3 || cfg == 7) ? 1 : 2;
  return cfg;
}
inline int gemm_executed_ns(int family, bool wide, int ns) { return (wide && family != GEMM_FAM_ACT) ? ns : 2; }

// ---- the plan of a problem ----------------------------------------------------------------------------------------------------------------
enum { GEMM_STATS_CHAN = 1, GEMM_STATS_ROW = 2 };

struct GemmPlan {
  int dtype, family;
  int cfg, bm, bn, ns;     // PLANNED tile config (of the split launch when splitk > 1), its rows x columns, ring depth: what the layout queries answer from
  int run_cfg, run_bm, run_bn, run_ns;   // ... and what the family's kernels execute for it (gemm_executed_cfg / _ns)
  int splitk;              // K slices per output tile; 1 = no split, > 1: a splitk_finish kernel adds the slices after the main launch
  int wide, colc;          // GemmP::wide / colc
  int cs_slots;            // chan_parts: sample slots per row tile
  int row_tiles, col_tiles;   // chan_parts holds [row_tiles][cs_slots][N][2]; row_nparts must equal col_tiles
  int64_t ws_bytes;        // split-K scratch the problem wants (0: it does not split)
};

inline bool gemm_is16(int dtype) { return dtype == FYC_BF16 || dtype == FYC_F16; }   // the 16-bit storage formats share every tile / epilogue decision

// Fills `pl` for the problem `a`, or returns false with the refusal in err[512].  `stats`: GEMM_STATS_* the problem writes (fyc_gemm: from
// its pointers; a layout query: the statistic it asks about).  `query`: plan as if the workspace the plan asks for were passed, and
// check nothing - the answer of a query must not depend on what only the call can know.
inline bool plan_gemm(const fyc_gemm_args* a, int stats, bool query, GemmPlan& pl, char* err) {
#define PLAN_REFUSE_IF(cond, ...) do { if (!query && (cond)) { snprintf(err, 512, __VA_ARGS__); return false; } } while (0)
  const int* tune = g_fyc_tuning;
  const bool h16 = gemm_is16(a->dtype), linear = a->epilogue == FYC_EPI_LINEAR, chan = (stats & GEMM_STATS_CHAN) != 0;
  const int rpb = a->rows_per_batch > 0 ? a->rows_per_batch : 1, ldrb = a->ldrb > 0 ? a->ldrb : a->N;
  memset(&pl, 0, sizeof(pl));
  pl.dtype = a->dtype;
  pl.family = a->mode == FYC_GEMM_CONV_T3 ? GEMM_FAM_T3 : (h16 && a->act != FYC_ACT_NONE) ? GEMM_FAM_ACT : a->mode == FYC_GEMM_PLAIN ? GEMM_FAM_PLAIN : GEMM_FAM_CONV;
  // ---- epilogue width: 16-byte row accesses need the shapes and alignments for them ----------------------------------------------
  const bool rb16 = a->rowbias == nullptr || (ldrb % 4 == 0 && ((uintptr_t)a->rowbias % 16) == 0);
  bool wide = h16 && a->epilogue != FYC_EPI_HEADS && a->N % (a->epilogue == FYC_EPI_GEGLU ? 32 : 8) == 0 && a->ldo % 8 == 0 && a->stride_o % 8 == 0 &&
              ((uintptr_t)a->out % 16) == 0 && (a->residual == nullptr || (a->ldr % 8 == 0 && ((uintptr_t)a->residual % 16) == 0)) &&
              (a->bias == nullptr || ((uintptr_t)a->bias % 16) == 0) && rb16 && tune[FYC_TUNE_NO_WIDE_EPILOGUE] == 0;
  // bias / colsum / rowbias rows may be fetched as 16-byte vectors and staged through LDS (always true for the engine's buffers)
  const bool colc = wide || (h16 && a->epilogue != FYC_EPI_GEGLU && a->N % 4 == 0 && ((uintptr_t)a->bias % 16) == 0 && ((uintptr_t)a->ln_colsum % 16) == 0 && rb16);
  if (h16 && a->epilogue == FYC_EPI_HEADS && colc && tune[FYC_TUNE_NO_WIDE_EPILOGUE] == 0 && tune[FYC_TUNE_NO_WIDE_HEADS] == 0 && a->heads > 0 && a->seg_cols > 0 &&
      (a->seg_cols / a->heads) % 8 == 0 && a->tokens % 16 == 0 && a->N % 8 == 0) {
    wide = true;                                      // wide head-split epilogue: 16-byte runs into every segment
    for (int s = 0; s < a->N / a->seg_cols && s < 3; ++s)
      wide = wide && ((uintptr_t)a->seg_out[s] % 16) == 0 && (!a->seg_transposed[s] || (a->seg_ld[s] > 0 ? a->seg_ld[s] : a->tokens) % 8 == 0);
  }
  // ---- tile config and ring depth.  FYC_TUNE_GEMM_TILE / _RING force a config / depth (bench sweeps, tests) --------------------------
  int cfg, ns = 2;
  if (!h16) {
    cfg = (a->N % 128 == 0) ? 1 : 2;                  // f32 parity mode: the narrow epilogue only exists for configs 1 and 2
  } else {
    // measured on MI355X (tools/gemm_bench.py, profiles/r01_gemm_tile_sweep.txt): the DMA fill rate of the
    // LDS ring, not the MFMA rate, bounds this kernel, so the widest tile that still fills the chip wins.
    if (a->N % 320 == 0) {
      // One or two column tiles per row and a short K loop (N = 320, K <= 320; N = 640, K <= 640): the epilogue is most of the
      // tile, and 128-row tiles give every CU twice as many epilogues to overlap with the next tile's fill.  Measured with the
      // operands coming from HBM and the epilogue features the UNet uses (tools/gemm_probe.py, profiles/r02_gemm_probe_cold_sweep.txt):
      // 95 (config 6) vs 111 (8) / 122 (5) us at M = 131072, N = K = 320 + residual, 67 vs 75 (5) at M = 32768, N = K = 640; the
      // Infinity-Cache-hot sweep had ranked 8 first.
      // Round 6 (profiles/r06_gemm_tile_sweep.txt, after the packed epilogue of round 4 and this round's epilogue work): with a residual the
      // two tiles are level (84 / 58 us either way), WITHOUT one the 256-row tile is 10-18 % faster (q2 head projection 131072x320x320: 72 vs
      // 88 us, 32768x640x640: 51 vs 61; proj_in 32768x640x640: 44 vs 49) - the short-K rule now only holds for problems with a residual.
      // (A problem with output statistics is planned from its shape: it keeps the residual-independent rule.)
      const bool short_k = a->mode == FYC_GEMM_PLAIN && (a->N == 320 || a->N == 640) && a->K <= a->N && (a->residual != nullptr || stats != 0);
      if (a->M >= 16384) cfg = short_k ? 6 : 5;
      else if (a->M >= 4096) cfg = (a->N >= 5120) ? 5 : 6;
      // M < 4096 (the 8x8 latent level): the widest tile that still gives the chip ~200+ work items.  Cold-operand probe at
      // M = 2048 (profiles/r04_gemm_small_m_ring_depth.txt): N = 10240 GEGLU 256x320 59 us vs 95 us on 128x64 tiles, N = 3840
      // 128x128 35 vs 47 us, N = 1280 stays on 128x64 (24 vs 27 / 34 us).  Deeper rings on the small tiles measured equal
      // (3-deep) or 1.6x slower (4-deep: one workgroup per CU) - more workgroups in flight, not a deeper ring, hide the latency.
      else cfg = (a->N >= 5120) ? 5 : (a->N >= 2560 ? 1 : 2);
    } else if (a->N % 256 == 0 && a->M >= 16384) {
      cfg = 7;
    } else if (a->N % 128 == 0 || a->N > 512) {
      cfg = (a->M >= 16384) ? 3 : 1;
    } else {
      cfg = 2;
    }
    if (a->tile > 0) { cfg = a->tile & 0xff; if (a->tile >> 8) ns = a->tile >> 8; }
    if (tune[FYC_TUNE_GEMM_TILE] > 0) cfg = tune[FYC_TUNE_GEMM_TILE];
    if (tune[FYC_TUNE_GEMM_RING] > 0) ns = tune[FYC_TUNE_GEMM_RING];
  }
  const auto geglu_tile = [&](int c) { return (a->epilogue == FYC_EPI_GEGLU && gemm_tile(c).geglu > 0) ? gemm_tile(c).geglu : c; };   // (the table: odd column blocks per wave)
  if (h16) {
    cfg = geglu_tile(cfg);
    if (!gemm_ring_built(gemm_tile(cfg), a->mode, ns)) ns = 2;   // deeper rings: config 1 (3) and, for linears, config 2 (3, 4) - the table
  }
  // The packed 16-bit LINEAR epilogue stages every per-column input through LDS.  The 64-byte K-tile configs (8 / 10) have a ring stage too
  // small for the accumulators of the statistics or for row-bias groups: their 128-byte twins run.  Two combinations stay with the narrow
  // per-lane epilogue (tile configs 1 / 2): a residual next to a LayerNorm fold, and row-bias groups it cannot stage (not multiples of 16
  // rows, more than 4 per row tile).
  const bool packed = wide && linear && a->act == FYC_ACT_NONE;
  const bool rb_multi = packed && a->rowbias != nullptr && rpb % gemm_tile_bm(cfg) != 0;
  if ((stats != 0 || rb_multi) && (cfg == 8 || cfg == 10)) cfg = (cfg == 8) ? 6 : 1;
  if (packed && ((a->residual != nullptr && a->ln_stats != nullptr) || (rb_multi && rowbias_slots(gemm_tile_bm(cfg), rpb) == 0))) {
    PLAN_REFUSE_IF(stats != 0, "fyc_gemm: output statistics need a row-bias layout / LayerNorm + residual combination the 16-byte epilogue covers");
    wide = false;
  }
  // ---- split-K: small M with a long K (the 8x8-latent level: M = 2048, K up to 23040) -------------------------------------------------
  // A 128x64 tile grid (320 tiles) re-fetches 3.4x the operand bytes per FLOP of the 320-wide tiles, and 128x320 tiles alone leave 3/4 of
  // the CUs idle (64 tiles): each output tile is cut into K slices (raw f32 partials to the workspace, added by a finish kernel that also
  // applies the LINEAR epilogue and, for chan_parts, writes the statistics in ITS 128-row tiles).
  int splitk = 1;
  const int split_cfg = (a->N % 320 == 0) ? 6 : 1;             // 128x320 or 128x128 tiles
  {
    // FYC_TUNE_SPLITK_MIN_KT = v > 0 (A/B): at least v K tiles per slice instead of 10, K >= 128 v instead of 2048 - the K = 1280 linears
    // of the 8x8 latent level (profiles/r06_gemm_small_m_split_k.txt) - and one 128-column tile is enough, so that a small test problem
    // can be made to split
    const int v = tune[FYC_TUNE_SPLITK_MIN_KT];
    const int min_kt = v > 0 ? v : 10;     // (16 until round 6: the K = 2560 shortcut of the 8x8 level now splits 4 ways, 39 -> 33 us)
    if (h16 && linear && a->act == FYC_ACT_NONE && a->batch <= 1 && a->tile == 0 && tune[FYC_TUNE_GEMM_TILE] <= 0 && tune[FYC_TUNE_NO_SPLITK] != 1 &&
        a->M > 0 && a->M <= 4096 && a->K >= (v > 0 ? 128 * v : 2048) && a->N % 8 == 0 && a->N >= (v > 0 ? 128 : 256)) {
      const int bn = gemm_tile_bn(split_cfg);
      const long long tiles = (long long)((a->M + 127) / 128) * ((a->N + bn - 1) / bn);
      const int kt = (a->K + 63) / 64;
      int s = (int)(256 / tiles);
      if (s > 8) s = 8;
      while (s > 1 && kt / s < min_kt) --s;                        // keep >= min_kt K tiles per slice
      if (s >= 2) splitk = s;
    }
    // the main kernel of a split problem writes raw partials: it can neither fold a LayerNorm nor sum its rows.  Without chan_parts such
    // a problem runs unsplit; WITH them the split is part of the announced layout
    const bool unsplittable = a->ln_stats != nullptr || (stats & GEMM_STATS_ROW) != 0;
    PLAN_REFUSE_IF(splitk > 1 && chan && unsplittable,
                   "fyc_gemm: chan_parts next to ln_stats / row_parts on a split-K shape (M=%d N=%d K=%d): the chan_parts layout fyc_gemm_stat_layout announces is the split-K finish kernel's, and a split problem can neither fold a LayerNorm nor sum its rows", a->M, a->N, a->K);
    if (!chan && unsplittable) splitk = 1;
    const int64_t want = (int64_t)splitk * a->M * a->N * 4;
    const bool ws_ok = query || (a->workspace != nullptr && a->workspace_bytes >= want && ((uintptr_t)a->workspace % 16) == 0);
    if (splitk > 1 && !(wide && ws_ok)) {
      PLAN_REFUSE_IF(chan, "fyc_gemm: chan_parts of a split-K problem (fyc_gemm_workspace_bytes() > 0) are laid out for its finish kernel: pass the workspace (and 16-byte aligned operands)");
      if (!chan) splitk = 1;
    }
    if (splitk > 1) { cfg = split_cfg; ns = 2; pl.ws_bytes = (chan && unsplittable) ? 0 : want; }      // (a call that will be refused wants nothing)
  }
  if (gemm_tile(cfg).twin > 0) cfg = gemm_tile(cfg).twin;      // a retired main-loop experiment: its one-phase twin (the table)
  cfg = geglu_tile(cfg);      // (the twin may be the one tile GEGLU is not built for)

  pl.cfg = cfg; pl.ns = ns; pl.splitk = splitk; pl.wide = wide ? 1 : 0; pl.colc = colc ? 1 : 0;
  pl.bm = gemm_tile_bm(cfg); pl.bn = gemm_tile_bn(cfg);
  pl.run_cfg = gemm_executed_cfg(pl.family, wide, cfg, a->N); pl.run_ns = gemm_executed_ns(pl.family, wide, ns);
  pl.run_bm = gemm_tile_bm(pl.run_cfg); pl.run_bn = gemm_tile_bn(pl.run_cfg);
  pl.row_tiles = (a->M + pl.bm - 1) / pl.bm; pl.col_tiles = (a->N + pl.bn - 1) / pl.bn;
  if (chan && a->cs_rows > 0)    // sample slots a row tile of bm rows can touch when a sample has cs_rows rows
    pl.cs_slots = a->cs_rows % pl.bm == 0 ? 1 : pl.bm % a->cs_rows == 0 ? pl.bm / a->cs_rows : (pl.bm - 1) / a->cs_rows + 2;
  // ---- the actual arguments against the plan ------------------------------------------------------------------------------------------
  PLAN_REFUSE_IF(chan && !(a->cs_rows > 0 && a->cs_rows % 16 == 0 && pl.cs_slots >= 1 && pl.cs_slots <= 4 && a->M % a->cs_rows == 0 && ((uintptr_t)a->chan_parts % 8) == 0),
                 "fyc_gemm: chan_parts needs cs_rows (=%d) a multiple of 16 dividing M=%d, and at most 4 samples per row tile (%d)", a->cs_rows, a->M, pl.cs_slots);
  PLAN_REFUSE_IF((stats & GEMM_STATS_ROW) && !(((uintptr_t)a->row_parts % 8) == 0 && a->row_nparts == pl.col_tiles),
                 "fyc_gemm: row_parts needs row_nparts == fyc_gemm_row_parts() = %d (got %d)", pl.col_tiles, a->row_nparts);
  // (the layouts above are the PLANNED tile's: statistics of a 16-bit problem therefore need the epilogue that executes it, or a plan on 1 / 2)
  PLAN_REFUSE_IF(chan && h16 && !wide && cfg != 1 && cfg != 2, "fyc_gemm: chan_parts in bf16 needs the 16-byte aligned layout or tile config 1 / 2");
  PLAN_REFUSE_IF((stats & GEMM_STATS_ROW) && h16 && !wide, "fyc_gemm: row_parts in bf16 needs the 16-byte aligned layout (N, ldo, ldr multiples of 8; aligned pointers)");
  PLAN_REFUSE_IF(pl.family == GEMM_FAM_ACT && a->mode != FYC_GEMM_PLAIN, "fyc_gemm: act needs the PLAIN mode");
  return true;
#undef PLAN_REFUSE_IF
}

// ---- the decisions of one launch ------------------------------------------------------------------------------------------------------------
// What launching the instantiation `g` on the problem `p` (as the entry points fill it: fyc_gemm, fyc_conv_up_phases) decides, on a device of n_cu compute
// units: the GemmP fields of the same names, the dynamic LDS bytes and the grid.  gemm_kernel.h::launch copies them and launches.
struct GemmLaunch {
  int tiles_m, tiles_n, rb_tile, rb_slots, pre, fast1, heads_pk, stagger, phase_delay, res_acc, strip;
  int smem;
  unsigned grid;      // blocks per batch element
};
inline GemmLaunch gemm_launch_plan(const GemmP& p, const GemmGeom& g, const int* tune, int n_cu, int batch) {
  const int BM = g.t.bm, BN = g.t.bn;
  const bool packed_linear = g.wide && g.epi == FYC_EPI_LINEAR;
  GemmLaunch q = {};
  q.smem = gemm_lds_bytes(g);
  q.tiles_m = (p.M + BM - 1) / BM;
  q.tiles_n = (p.N + BN - 1) / BN;
  q.rb_tile = (p.colc && p.rowbias != nullptr && p.rows_per_batch % BM == 0) ? 1 : 0;
  q.rb_slots = (packed_linear && p.rowbias != nullptr && !q.rb_tile) ? rowbias_slots(BM, p.rows_per_batch) : 0;
  // epilogue inputs by DMA under the K loop: 2-deep-ring wide epilogues with at least two K tiles per output tile; the row statistics as
  // stored {mean, rstd} pairs, two rows per 16-byte lane (M even, 16-byte aligned); row-bias rows only where the packed LINEAR epilogue
  // stages them (fyc_set_tuning key 12 = 1 restores the loads in the epilogue: A/B)
  {
    const int BK = (g.t.rb / 16) * (16 / g.esize);
    const int kt = (p.K + BK - 1) / BK;
    const bool rb_ok = p.rowbias == nullptr || (g.epi == FYC_EPI_LINEAR && (q.rb_tile || q.rb_slots > 0));
    q.pre = (gemm_pre_built(g) && tune[FYC_TUNE_NO_PRESTAGE] != 1 && kt >= 2 && !(p.splitk > 1) && p.ln_nparts == 0 && rb_ok && p.wide &&
             (p.ln_stats == nullptr || (p.M % 2 == 0 && ((uintptr_t)p.ln_stats % 16) == 0))) ? 1 : 0;
  }
  q.fast1 = tune[FYC_TUNE_GENERIC_PASS1] == 1 ? 0 : 1;
  // pack-first head-split epilogue: in the pipeline it wins at the 16x16 level only (8192x3840x1280 0.588 -> 0.562 ms per DDIM step, 8192x1280x1280
  // 0.235 -> 0.212) and LOSES at the 64x64 / 32x32 levels (131072x960x320 0.970 -> 1.051, 32768x1920x640 0.666 -> 0.756: profiles/r06_gemm_epilogue_ab.txt
  // part 4) - key 15 = 1 forces it on, 2 off
  q.heads_pk = tune[FYC_TUNE_HEADS_PACKED] == 1 ? 1 : tune[FYC_TUNE_HEADS_PACKED] == 2 ? 0 : (p.M <= 8192 ? 1 : 0);
  q.stagger = tune[FYC_TUNE_NO_STAGGER] == 1 ? 0 : 1;
  q.phase_delay = tune[FYC_TUNE_PHASE_DELAY] > 0 ? tune[FYC_TUNE_PHASE_DELAY] : 0;
  q.res_acc = (packed_linear && p.residual != nullptr && p.ln_stats == nullptr && !(p.splitk > 1)) ? 1 : 0;
  q.strip = (q.tiles_n > 4 && tune[FYC_TUNE_GEMM_STRIP] >= 0) ? (tune[FYC_TUNE_GEMM_STRIP] > 0 ? tune[FYC_TUNE_GEMM_STRIP] : (q.tiles_n >= 16 ? 8 : 4)) : 0;   // measured: profiles/r01_gemm_strip_order.txt
  // persistent grid: as many blocks as stay resident (LDS-limited), each walks a strided tile list
  int occ = (160 * 1024) / q.smem;
  const int wave_cap = 32 / (g.t.wgm * g.t.wgn);
  if (occ > wave_cap) occ = wave_cap;
  if (occ < 1) occ = 1;
  long long resident = (long long)n_cu * occ / (batch > 0 ? batch : 1);
  if (resident < n_cu) resident = n_cu;
  const long long ntiles = (long long)q.tiles_m * q.tiles_n * (p.splitk > 1 ? p.splitk : 1);
  q.grid = (unsigned)(ntiles < resident ? ntiles : resident);
  return q;
}

}  // namespace fycg
