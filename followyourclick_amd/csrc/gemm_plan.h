// The launch plan of one fyc_gemm problem: kernel family, tile, ring depth, split-K, epilogue width, statistics layout, workspace.
// plan_gemm() is the ONE place these are decided - fyc_gemm executes the plan, fyc_gemm_workspace_bytes / fyc_gemm_row_parts /
// fyc_gemm_stat_layout read a field of it.  Host only: a pure function of the scalar fields of fyc_gemm_args, of which pointers are null
// and how they are aligned, and of g_fyc_tuning; no HIP call, no static state.
//
// A problem that writes output statistics (chan_parts / row_parts) is planned from its shape alone - M, N, K, mode, dtype, batch, tile,
// cs_rows and the tuning table, which is all the layout queries see (the engine sizes its buffers before the call exists).  The actual
// arguments are then checked against that plan, and a call that cannot run it (a folded LayerNorm on a problem that splits, operands
// that rule out the 16-byte epilogue, ...) is REFUSED with the conflict named: never another tile, never a layout nobody announced.
#pragma once
#include "gemm_kernel.h"

namespace fycg {

enum { GEMM_FAM_PLAIN, GEMM_FAM_CONV, GEMM_FAM_ACT, GEMM_FAM_T3 };   // one translation unit per (dtype, family): gemm_kernel.h::run_*
enum { GEMM_STATS_CHAN = 1, GEMM_STATS_ROW = 2 };

struct GemmPlan {
  int dtype, family;
  int cfg, bm, bn, ns;     // tile config (gemm_kernel.h::dispatch_cfg; of the split launch when splitk > 1), its rows x columns, ring depth
  int splitk;              // K slices per output tile; 1 = no split, > 1: a splitk_finish kernel adds the slices after the main launch
  int wide, colc;          // GemmP::wide / colc
  int cs_slots;            // chan_parts: sample slots per row tile
  int row_tiles, col_tiles;   // chan_parts holds [row_tiles][cs_slots][N][2]; row_nparts must equal col_tiles
  int64_t ws_bytes;        // split-K scratch the problem wants (0: it does not split)
};

inline bool gemm_is16(int dtype) { return dtype == FYC_BF16 || dtype == FYC_F16; }   // the 16-bit storage formats share every tile / epilogue decision

// row-tile height / column-tile width of a tile config (gemm_kernel.h::dispatch_cfg).  12 / 13 / 14 (the 32x32x16 twins of 5 / 7 / 3) and 21 / 22 / 23 /
// 31 (main-loop experiments on the tiles of 5 / 6 / 7 / 6) are RETIRED ids, never built: their rows stay so that the layout queries answer as they always did
inline int gemm_tile_bm(int cfg) { return (cfg == 3 || cfg == 4 || cfg == 5 || cfg == 7 || (cfg >= 12 && cfg <= 14) || cfg == 21 || cfg == 23) ? 256 : 128; }
inline int gemm_tile_bn(int cfg) {
  switch (cfg) { case 2: case 4: return 64; case 5: case 6: case 8: case 12: case 21: case 22: case 31: return 320; case 7: case 13: case 23: return 256; case 11: return 160; default: return 128; }
}

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
  // GEGLU pairs 16-column value / gate blocks inside a wave: config 6 gives a wave 5 column blocks (128x320 over 2x4 waves) and
  // used to leave the output unwritten (found by tools/gemm_diag.py at M = 4096 / 8192, N = 2560 - shapes the UNet never issued)
  const auto geglu_tile = [&](int c) { return a->epilogue != FYC_EPI_GEGLU ? c : (c == 6 || c == 11) ? 5 : c == 22 ? 21 : c; };
  if (h16) {
    cfg = geglu_tile(cfg);
    if (!((cfg == 1 && ns == 3) || (cfg == 2 && (ns == 3 || ns == 4) && a->mode == FYC_GEMM_PLAIN))) ns = 2;   // deeper rings: config 1 (3) and, for linears, config 2 (3, 4)
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
  // tile configs 21 / 22 / 23 / 31 named the round-4 main-loop experiments (retired: profiles/r04_gemm_pingpong_and_prefetch_sweep.txt): a request for one runs its
  // one-phase twin (same tile, same wave grid), as it did in every build without them
  cfg = cfg == 21 ? 5 : cfg == 22 ? 6 : cfg == 23 ? 7 : cfg == 31 ? 6 : cfg;
  cfg = geglu_tile(cfg);      // (the twin may be the one tile GEGLU is not built for)

  pl.cfg = cfg; pl.ns = ns; pl.splitk = splitk; pl.wide = wide ? 1 : 0; pl.colc = colc ? 1 : 0;
  pl.bm = gemm_tile_bm(cfg); pl.bn = gemm_tile_bn(cfg);
  pl.row_tiles = (a->M + pl.bm - 1) / pl.bm; pl.col_tiles = (a->N + pl.bn - 1) / pl.bn;
  if (chan && a->cs_rows > 0)    // sample slots a row tile of bm rows can touch when a sample has cs_rows rows
    pl.cs_slots = a->cs_rows % pl.bm == 0 ? 1 : pl.bm % a->cs_rows == 0 ? pl.bm / a->cs_rows : (pl.bm - 1) / a->cs_rows + 2;
  // ---- the actual arguments against the plan ------------------------------------------------------------------------------------------
  PLAN_REFUSE_IF(chan && !(a->cs_rows > 0 && a->cs_rows % 16 == 0 && pl.cs_slots >= 1 && pl.cs_slots <= 4 && a->M % a->cs_rows == 0 && ((uintptr_t)a->chan_parts % 8) == 0),
                 "fyc_gemm: chan_parts needs cs_rows (=%d) a multiple of 16 dividing M=%d, and at most 4 samples per row tile (%d)", a->cs_rows, a->M, pl.cs_slots);
  PLAN_REFUSE_IF((stats & GEMM_STATS_ROW) && !(((uintptr_t)a->row_parts % 8) == 0 && a->row_nparts == pl.col_tiles),
                 "fyc_gemm: row_parts needs row_nparts == fyc_gemm_row_parts() = %d (got %d)", pl.col_tiles, a->row_nparts);
  PLAN_REFUSE_IF(chan && h16 && !wide && cfg != 1 && cfg != 2, "fyc_gemm: chan_parts in bf16 needs the 16-byte aligned layout or tile config 1 / 2");
  PLAN_REFUSE_IF((stats & GEMM_STATS_ROW) && h16 && !wide, "fyc_gemm: row_parts in bf16 needs the 16-byte aligned layout (N, ldo, ldr multiples of 8; aligned pointers)");
  PLAN_REFUSE_IF(pl.family == GEMM_FAM_ACT && a->mode != FYC_GEMM_PLAIN, "fyc_gemm: act needs the PLAIN mode");
  return true;
#undef PLAN_REFUSE_IF
}

}  // namespace fycg
