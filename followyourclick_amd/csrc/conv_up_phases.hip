// Host entry of the four-phase form of Upsample3D / Upsample2D's nearest-2x + 3x3 convolution (kernel mode GEMM_MODE_UP_PHASES, gemm_kernel.h;
// instantiations: gemm_{bf16,f16}_up.hip): argument validation, tile choice through the GEMM planner (gemm_plan.h, no rule of its own), launch.
// fyc_gemm and its plan table do not know the mode: FYC_GEMM_CONV3X3_UP2 stays what it was, this is a second way to compute the exact-2x case.
#include "gemm_plan.h"

using namespace fycg;

namespace {
struct UpPlan { int cfg, ns, bm, colc, wide, row_tiles; };

// The tile of the (M, N, K = 4 Cin) problem is the one plan_gemm gives a LINEAR-epilogue convolution of that shape with output statistics (asked for or
// not: the layout query and the call must agree without seeing each other's pointers).  A row tile must not straddle a phase or a group: where the planned
// tile does not divide the group (or the shape would split K, whose finish kernel knows no row map) the 128-row tile of that width runs instead.
bool up_plan(const fyc_conv_up_phases_args* u, UpPlan& up) {
  char unused[512];
  fyc_gemm_args g = u->gemm;
  g.mode = FYC_GEMM_CONV3X3; g.epilogue = FYC_EPI_LINEAR; g.act = FYC_ACT_NONE; g.batch = 1;
  g.cs_rows = u->group_rows;
  GemmPlan pl;
  if (g.M <= 0 || g.N <= 0 || u->group_rows <= 0 || !plan_gemm(&g, GEMM_STATS_CHAN, true, pl, unused)) return false;
  if ((pl.splitk > 1 || u->group_rows % pl.bm != 0) && g.tile == 0) {
    g.tile = (g.N % 320 == 0) ? 6 : (g.N % 128 == 0 || g.N > 512) ? 1 : 2;
    if (!plan_gemm(&g, GEMM_STATS_CHAN, true, pl, unused)) return false;
  }
  if (pl.splitk > 1 || u->group_rows % pl.bm != 0 || pl.cs_slots != 1 || pl.family != GEMM_FAM_CONV) return false;
  up.cfg = pl.cfg; up.ns = pl.ns; up.bm = pl.bm; up.colc = pl.colc; up.wide = pl.wide; up.row_tiles = pl.row_tiles;
  return true;
}

// what the shape itself must satisfy (no pointer is read); nullptr = fine, else the reason
const char* up_shape_refusal(const fyc_conv_up_phases_args* u) {
  const fyc_gemm_args* a = &u->gemm;
  if (!gemm_is16(a->dtype)) return "16-bit dtypes only (FYC_F32 keeps FYC_GEMM_CONV3X3_UP2)";
  if (a->Cin <= 0 || a->Cin % 64 != 0) return "Cin must be a positive multiple of 64";
  if (a->N <= 0 || a->N % 8 != 0) return "N (Cout) must be a positive multiple of 8";
  if (a->Hin <= 0 || a->Win <= 0 || a->Win > 4096) return "Hin / Win must be positive, Win <= 4096";
  if (a->Hout != 2 * a->Hin || a->Wout != 2 * a->Win) return "the output must be exactly twice the input (other sizes keep FYC_GEMM_CONV3X3_UP2)";
  const long long hw = (long long)a->Hin * a->Win;
  if (u->group_rows <= 0 || u->group_rows % hw != 0) return "group_rows must be a whole number of input frames (Hin * Win rows each)";
  if (a->M <= 0 || a->M % 4 != 0 || (a->M / 4) % u->group_rows != 0) return "M must be 4 * group_rows * (number of groups)";
  if ((long long)(a->M / 4) * a->Cin >= 0xffffffffll || 4ll * a->N * a->Cin * 4 >= 0xffffffffll) return "an operand has 2^32 elements or more: split the call";
  return nullptr;
}
}  // namespace

extern "C" int fyc_conv_up_phases_supported(int32_t dtype, int32_t Cin, int32_t Cout, int32_t Hin, int32_t Win, int32_t group_rows, int32_t exact2) {
  if (!exact2 || group_rows <= 0 || group_rows > (1 << 28)) return 0;
  fyc_conv_up_phases_args u;
  memset(&u, 0, sizeof(u));
  u.gemm.dtype = dtype; u.gemm.Cin = Cin; u.gemm.N = Cout; u.gemm.K = 4 * Cin; u.gemm.ldw = 4 * Cin; u.gemm.ldo = Cout;
  u.gemm.Hin = Hin; u.gemm.Win = Win; u.gemm.Hout = 2 * Hin; u.gemm.Wout = 2 * Win;
  u.gemm.M = 4 * group_rows;      // one group: whether a shape is covered does not depend on how many there are (up_plan falls back to the 128-row tile)
  u.group_rows = group_rows;
  UpPlan up;
  return up_shape_refusal(&u) == nullptr && up_plan(&u, up) && up.wide ? 1 : 0;
}

extern "C" int fyc_conv_up_phases_stat_layout(const fyc_conv_up_phases_args* u, int32_t* tile_rows, int32_t* slots) {
  UpPlan up;
  if (u == nullptr || up_shape_refusal(u) != nullptr || !up_plan(u, up)) return 0;
  if (tile_rows) *tile_rows = up.bm;
  if (slots) *slots = 1;      // by construction: a row tile lies inside one (group, phase) sample of group_rows rows
  return up.row_tiles;
}

extern "C" int fyc_conv_up_phases(const fyc_conv_up_phases_args* u, void* stream) {
  FYC_REQUIRE(u != nullptr, "fyc_conv_up_phases: null args");
  const fyc_gemm_args* a = &u->gemm;
  FYC_REQUIRE(g_fyc_zero_page != nullptr, "fyc_conv_up_phases: fyc_init() not called");
  FYC_REQUIRE(a->mode == FYC_GEMM_CONV3X3_UP2 && a->epilogue == FYC_EPI_LINEAR && a->act == FYC_ACT_NONE && a->batch <= 1 && a->tile >= 0,
              "fyc_conv_up_phases: the embedded arguments describe a FYC_GEMM_CONV3X3_UP2 problem with the LINEAR epilogue (mode %d, epilogue %d, act %d, batch %d)",
              a->mode, a->epilogue, a->act, a->batch);
  FYC_REQUIRE(a->residual == nullptr && a->rowbias == nullptr && a->a2 == nullptr && a->ln_stats == nullptr && a->ln_colsum == nullptr && a->row_parts == nullptr,
              "fyc_conv_up_phases: bias and chan_parts only - residual, rowbias, a2, a folded LayerNorm and row_parts are not built for the phase form");
  const char* why = up_shape_refusal(u);
  FYC_REQUIRE(why == nullptr, "fyc_conv_up_phases: %s (M=%d N=%d Cin=%d Hin=%d Win=%d Hout=%d Wout=%d group_rows=%d dtype=%d)", why, a->M, a->N, a->Cin, a->Hin,
              a->Win, a->Hout, a->Wout, u->group_rows, a->dtype);
  FYC_REQUIRE(a->K == 4 * a->Cin && a->ldw >= a->K && a->ldw % 8 == 0, "fyc_conv_up_phases: K=%d must be 4*Cin and ldw=%d a multiple of 8 >= K (weights [4 phases][N][ldw])", a->K, a->ldw);
  FYC_REQUIRE(4ll * a->N * a->ldw < 0xffffffffll, "fyc_conv_up_phases: the phase weights have 2^32 elements or more");
  FYC_REQUIRE(a->a != nullptr && a->w != nullptr && a->out != nullptr && ((uintptr_t)a->a % 16) == 0 && ((uintptr_t)a->w % 16) == 0, "fyc_conv_up_phases: a / w / out must be set, a and w 16-byte aligned");
  FYC_REQUIRE(a->chan_parts == nullptr || (a->cs_rows == u->group_rows && ((uintptr_t)a->chan_parts % 8) == 0),
              "fyc_conv_up_phases: chan_parts are per (group, phase): cs_rows=%d must equal group_rows=%d (8-byte aligned)", a->cs_rows, u->group_rows);
  UpPlan up;
  FYC_REQUIRE(up_plan(u, up), "fyc_conv_up_phases: no row tile divides group_rows=%d (a multiple of 128 is needed; N=%d): keep FYC_GEMM_CONV3X3_UP2", u->group_rows, a->N);
  FYC_REQUIRE(up.wide, "fyc_conv_up_phases: the 16-byte epilogue needs ldo=%d a multiple of 8 and 16-byte aligned out / bias", a->ldo);
  GemmP p;
  memset(&p, 0, sizeof(p));
  p.a = (const char*)a->a; p.w = (const char*)a->w; p.bias = a->bias; p.out = (char*)a->out;
  p.M = a->M; p.N = a->N; p.K = a->K; p.lda = a->Cin; p.ldw = a->ldw; p.ldo = a->ldo; p.ldr = a->ldo;
  p.mode = GEMM_MODE_UP_PHASES; p.epilogue = FYC_EPI_LINEAR;
  p.Hout = a->Hout; p.Wout = a->Wout; p.Hin = a->Hin; p.Win = a->Win; p.Cin = a->Cin; p.conv_stride = 1; p.conv_pad = 1;
  p.rows_per_batch = 1; p.ldrb = a->N;
  p.out_scale = a->out_scale;
  p.chan_parts = a->chan_parts; p.cs_rows = u->group_rows; p.cs_slots = 1;
  p.t3_rows = u->group_rows;            // GEMM_MODE_UP_PHASES: rows per group
  p.up_sw = 1.0f / (float)a->Win;       // ... and the reciprocal of its output row map (fdiv_small)
  p.wide = 1; p.colc = up.colc;
  p.zero = (const char*)g_fyc_zero_page;
  return a->dtype == FYC_F16 ? run_f16_up_phases(p, up.cfg, up.ns, (hipStream_t)stream) : run_bf16_up_phases(p, up.cfg, up.ns, (hipStream_t)stream);
}
