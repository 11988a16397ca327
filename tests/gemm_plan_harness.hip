// Host-decision table of fyc_gemm (tests/test_gemm_plan.py): linked with csrc/gemm.hip and csrc/api.hip in place of the kernel
// instantiations.  Every fycg::run_* below records what it was asked to launch and returns 0; main() walks a grid of fyc_gemm_args and
// prints, per case, the three host queries, the recorded launch and the return code.  No GPU is used: the program hides every device
// before its first HIP call and refuses to go on if one is still visible (the operand pointers are made-up addresses).  The only real
// launch a call can reach is the split-K finish kernel, which then fails with "no ROCm-capable device" AFTER the stub has recorded:
// that one message is masked (rc 0).
//   line:  <dtype> <mode> <M>x<N>x<K> <variation> | <workspace bytes> <row_parts tiles> <stat tiles>/<tile rows>/<slots> | <launch> | <rc> [message]
//   launch: <family> <cfg> <ns> <wide> <colc> <splitk> <cs_slots> <batch>   (ns -1: the entry takes none)
// Invariants asserted for every case that returns 0 (a violated one is appended to the line as !I1 / !I2 / !I3, exit status 1):
//   I1  chan_parts: the executed (row-tile height, cs_slots, split or not) is what fyc_gemm_stat_layout / fyc_gemm_workspace_bytes answer
//       for the pointer-free copy of the arguments
//   I2  row_parts: row_nparts == ceil(N / column-tile width) of the executed tile
//   I3  fyc_gemm_workspace_bytes > 0 exactly when the call, given that workspace, splits
//
// Second mode (tests/test_gemm_cases.py): `gemm_plan_harness <file>` (`-` = stdin) plans the cases of that file instead of the grid, one per
// line: a name without blanks, then key=value fields (tests/gemm_cases.py::harness_line writes them; an unknown key is an error, exit 4).
//   scalars:   dtype mode M N K lda ldw ldo ldr ldrb rpb tile batch stride_a stride_w stride_o cs_rows
//              Hout Wout Hin Win Cin stride pad t3_frames t3_rows epilogue act ln_nparts k_split lda2 seg_cols heads tokens
//   operands:  bias rowbias residual chan a2 = 1 (present) / 0; residual = 2: the residual IS the output (in-place add); ln = 1: ln_stats and ln_colsum
//   offsets:   out_off rb_off res_off = bytes added to the made-up 256-byte aligned address of that operand
//   segments:  seg_tr seg_ld seg_off = comma-separated seg_transposed / seg_ld / byte offset of seg_out, one entry per segment of the HEADS epilogue
//   tuning:    tune=<key>:<value>, may repeat; reset after the case
//   answer:    <name> | <launch, as above> | <executed cfg> <executed rows>x<columns> | <rc> [message] | <decisions>
//   executed:  GemmPlan::run_cfg / run_bm / run_bn of the plan the call executed (0 0x0: nothing was launched)
//   decisions: pre fast1 heads_pk res_acc rb_tile rb_slots strip lds grid, as key=value: what gemm_plan.h::gemm_launch_plan decides for the recorded launch
//              on a device of 256 compute units (no device answers here); `-` where nothing was launched or the executed tile is one the table does not build
// Without an argument the output is the table above, byte for byte.
#include <stdlib.h>

#include <functional>
#include <string>
#include <vector>

#include "../followyourclick_amd/csrc/gemm_plan.h"

using fycg::GemmP;

namespace {
struct Rec { const char* fam; int cfg, ns, wide, colc, splitk, cs_slots, batch, calls; };
Rec g_rec;
GemmP g_rec_p;      // the arguments of the recorded launch
int record(const char* fam, const GemmP& p, int batch, int cfg, int ns) {
  g_rec = Rec{fam, cfg, ns, p.wide, p.colc, p.splitk, p.cs_slots, batch, g_rec.calls + 1};
  g_rec_p = p;
  return 0;
}
}  // namespace

namespace fycg {
int run_bf16_plain(const GemmP& p, int batch, int cfg, int ns, hipStream_t) { return record("bf16_plain", p, batch, cfg, ns); }
int run_bf16_conv(const GemmP& p, int batch, int cfg, int ns, hipStream_t) { return record("bf16_conv", p, batch, cfg, ns); }
int run_bf16_act(const GemmP& p, int batch, int cfg, hipStream_t) { return record("bf16_act", p, batch, cfg, -1); }
int run_f32(const GemmP& p, int batch, int cfg, hipStream_t) { return record("f32", p, batch, cfg, -1); }
int run_f16_plain(const GemmP& p, int batch, int cfg, int ns, hipStream_t) { return record("f16_plain", p, batch, cfg, ns); }
int run_f16_conv(const GemmP& p, int batch, int cfg, int ns, hipStream_t) { return record("f16_conv", p, batch, cfg, ns); }
int run_f16_act(const GemmP& p, int batch, int cfg, hipStream_t) { return record("f16_act", p, batch, cfg, -1); }
int run_bf16_t3(const GemmP& p, int batch, int cfg, int ns, hipStream_t) { return record("bf16_t3", p, batch, cfg, ns); }
int run_f16_t3(const GemmP& p, int batch, int cfg, int ns, hipStream_t) { return record("f16_t3", p, batch, cfg, ns); }
int run_f32_t3(const GemmP& p, int batch, int cfg, hipStream_t) { return record("f32_t3", p, batch, cfg, -1); }
}  // namespace fycg

namespace {
// made-up, 256-byte aligned operand addresses: the host code only looks at null-ness and alignment
void* fake(int i) { return (void*)(uintptr_t)(0x10000000ull * (unsigned)(i + 1)); }
enum { P_A, P_W, P_OUT, P_BIAS, P_RES, P_RB, P_LNS, P_LNC, P_CP, P_RP, P_A2, P_WS, P_SEG };

const char* const DT_NAME[3] = {"f32", "bf16", "f16"};
const char* const MODE_NAME[5] = {"plain", "conv", "conv_s2", "up2", "t3"};   // (conv_s2: FYC_GEMM_CONV3X3 with stride 2)

struct Case {
  std::string name;
  fyc_gemm_args a;
  std::vector<std::pair<int, int>> tuning;
  bool no_ws = false, want_rp = false;
};

// mode index: 0 PLAIN, 1 CONV3X3 stride 1, 2 CONV3X3 stride 2, 3 CONV3X3_UP2, 4 CONV_T3.  Convolutions: 8x8 outputs (M / 64 frames).
bool shape_ok(int mi, int K) { return mi == 0 || (mi == 4 ? (K % 3 == 0 && (K / 3) % 64 == 0) : (K % 9 == 0 && (K / 9) % 64 == 0)); }
Case base(int dtype, int mi, int M, int N, int K, const char* var) {
  Case c;
  char buf[96];
  snprintf(buf, sizeof(buf), "%s %s %dx%dx%d %s", DT_NAME[dtype], MODE_NAME[mi], M, N, K, var);
  c.name = buf;
  fyc_gemm_args& a = c.a;
  memset(&a, 0, sizeof(a));
  a.a = fake(P_A); a.w = fake(P_W); a.out = fake(P_OUT); a.bias = (const float*)fake(P_BIAS);
  a.M = M; a.N = N; a.K = K; a.ldw = K; a.ldo = N; a.ldr = N; a.batch = 1; a.out_scale = 1.f; a.dtype = dtype;
  a.epilogue = FYC_EPI_LINEAR; a.rows_per_batch = M;
  if (mi == 0) { a.mode = FYC_GEMM_PLAIN; a.lda = K; }
  else if (mi == 4) { a.mode = FYC_GEMM_CONV_T3; a.Cin = K / 3; a.lda = a.Cin; a.t3_frames = 4; a.t3_rows = 16; }
  else {
    a.mode = mi == 3 ? FYC_GEMM_CONV3X3_UP2 : FYC_GEMM_CONV3X3;
    a.Cin = K / 9; a.lda = a.Cin; a.Hout = a.Wout = 8; a.conv_stride = mi == 2 ? 2 : 1; a.conv_pad = 1;
    a.Hin = a.Win = mi == 2 ? 16 : mi == 3 ? 4 : 8;
  }
  return c;
}

typedef std::function<void(Case&)> Var;
struct NamedVar { std::string tag; Var f; };
NamedVar both(const NamedVar& x, const NamedVar& y) { return {x.tag + "+" + y.tag, [x, y](Case& c) { x.f(c); y.f(c); }}; }
NamedVar tile_var(int t) { char b[16]; snprintf(b, sizeof(b), "tile%x", t); return {b, [t](Case& c) { c.a.tile = t; }}; }
NamedVar key_var(int k, int v) { char b[16]; snprintf(b, sizeof(b), "key%d=%d", k, v); return {b, [k, v](Case& c) { c.tuning.push_back({k, v}); }}; }
NamedVar rb_var(int rpb) {   // rpb 0: one group = the whole problem
  char b[16]; snprintf(b, sizeof(b), "rb%d", rpb);
  return {b, [rpb](Case& c) { c.a.rowbias = (const float*)fake(P_RB); c.a.rows_per_batch = rpb > 0 ? rpb : c.a.M; }};
}
NamedVar cp_var(int rows) { char b[16]; snprintf(b, sizeof(b), "cp%d", rows); return {b, [rows](Case& c) { c.a.chan_parts = (float*)fake(P_CP); c.a.cs_rows = rows; }}; }
const NamedVar V_RES{"res", [](Case& c) { c.a.residual = fake(P_RES); }};
const NamedVar V_LN{"ln", [](Case& c) { c.a.ln_stats = (const float*)fake(P_LNS); c.a.ln_colsum = (const float*)fake(P_LNC); }};
const NamedVar V_RP{"rp", [](Case& c) { c.a.row_parts = (float*)fake(P_RP); c.want_rp = true; }};
const NamedVar V_A2{"a2", [](Case& c) { c.a.a2 = fake(P_A2); c.a.k_split = 64; c.a.lda2 = c.a.K - 64; }};
const NamedVar V_GEGLU{"geglu", [](Case& c) { c.a.epilogue = FYC_EPI_GEGLU; c.a.ldo = c.a.N / 2; }};
const NamedVar V_HEADS{"heads", [](Case& c) {
  fyc_gemm_args& a = c.a;
  int nseg = 1;
  while (nseg < 3 && (a.N % nseg != 0 || a.N / nseg > 4096)) ++nseg;
  a.epilogue = FYC_EPI_HEADS; a.seg_cols = a.N / nseg; a.heads = a.seg_cols % 64 == 0 ? a.seg_cols / 64 : a.seg_cols / 8; a.tokens = 64;
  for (int s = 0; s < 3; ++s) a.seg_out[s] = fake(P_SEG + s);
}};
const NamedVar V_ACT1{"act1", [](Case& c) { c.a.act = FYC_ACT_GELU; }};
const NamedVar V_ACT2{"act2", [](Case& c) { c.a.act = FYC_ACT_QUICK_GELU; }};
const NamedVar V_BATCH{"batch4", [](Case& c) { c.a.batch = 4; c.a.stride_a = (int64_t)c.a.M * c.a.K; c.a.stride_w = (int64_t)c.a.N * c.a.K; c.a.stride_o = (int64_t)c.a.M * c.a.N; }};
const NamedVar V_OUT2{"out+2", [](Case& c) { c.a.out = (char*)c.a.out + 2; }};
const NamedVar V_LDO{"ldo_odd", [](Case& c) { c.a.ldo += 1; }};
const NamedVar V_NOWS{"no_ws", [](Case& c) { c.no_ws = true; }};

std::vector<Case> grid() {
  std::vector<Case> out;
  const int Ms[] = {64, 512, 2048, 4096, 8192, 16384, 32768, 131072};
  const int Ns[] = {64, 128, 264, 320, 640, 960, 1280, 2560, 3840, 5120, 10240};
  const int Ks[] = {64, 320, 640, 1280, 2560, 5760, 11520};
  // (1) every shape at default flags
  for (int dtype : {FYC_BF16, FYC_F16, FYC_F32})
    for (int mi = 0; mi < 5; ++mi)
      for (int M : Ms) for (int N : Ns) for (int K : Ks)
        if (shape_ok(mi, K)) out.push_back(base(dtype, mi, M, N, K, "base"));
  // (2) one feature at a time, and the pairs the host code couples, on a few shapes of every regime (split-K eligible or not, 320 k widths
  // or not, short K, each M class of the tile rule)
  std::vector<NamedVar> vars = {V_RES, V_LN, rb_var(0), rb_var(64), rb_var(48), cp_var(64), cp_var(256), cp_var(1024), V_RP, V_A2, V_GEGLU, V_HEADS,
                                V_ACT1, V_ACT2, V_BATCH, V_OUT2, V_LDO, V_NOWS, key_var(1, 5), key_var(2, 3), key_var(6, 1), key_var(7, 1), key_var(10, 2), key_var(14, 1),
                                both(V_HEADS, key_var(7, 1)), both(V_RES, V_LN)};
  const int tiles[] = {1, 5, 6, 8, 10, 11, 0x301};
  for (int t : tiles) vars.push_back(tile_var(t));
  for (int rows : {64, 256})
    for (const NamedVar& v : {V_LN, V_RP, V_RES, key_var(6, 1), V_NOWS}) vars.push_back(both(cp_var(rows), v));
  for (int rpb : {0, 64, 48}) for (int t : tiles) vars.push_back(both(rb_var(rpb), tile_var(t)));
  for (int t : {6, 11}) vars.push_back(both(V_GEGLU, tile_var(t)));
  const int shapes[][3] = {{512, 5120, 2560}, {2048, 1280, 2560}, {2048, 1280, 5760}, {2048, 264, 2560}, {64, 128, 320}, {4096, 640, 640}, {4096, 2560, 640},
                           {8192, 2560, 320}, {16384, 1280, 1280}, {32768, 640, 640}, {131072, 320, 320}, {2048, 320, 11520}};
  for (const auto& s : shapes)
    for (int mi : {0, 1, 4})
      for (int dtype : {FYC_BF16, FYC_F32}) {
        if (!shape_ok(mi, s[2]) || (dtype == FYC_F32 && (mi != 0 || &s - shapes >= 3))) continue;      // (f32: the first three shapes)
        for (const NamedVar& v : vars) {
          Case c = base(dtype, mi, s[0], s[1], s[2], v.tag.c_str());
          v.f(c);
          out.push_back(c);
        }
      }
  // (3) the shapes of tests/test_kernels_gpu.py::test_gemm_split_k_output_statistics, as that test calls them
  const struct { int mi, M, N, K, cs_rows, res; } sk[] = {{1, 2048, 1280, 11520, 64, 1}, {1, 2048, 1280, 23040, 64, 0}, {0, 2048, 1280, 6400, 64, 1},
                                                          {0, 1008, 640, 2560, 48, 0}, {1, 512, 320, 5760, 64, 0}, {0, 512, 5120, 2560, 64, 0}};
  for (int dtype : {FYC_BF16, FYC_F16})
    for (const auto& t : sk)
      for (int ln = 0; ln < (t.mi == 0 ? 2 : 1); ++ln) {
        NamedVar v = cp_var(t.cs_rows);
        if (t.res) v = both(v, V_RES);
        if (ln) v = both(v, V_LN);
        Case c = base(dtype, t.mi, t.M, t.N, t.K, ("splitk_stats:" + v.tag).c_str());
        v.f(c);
        out.push_back(c);
      }
  return out;
}

// the plan fyc_gemm executed for `a` (the call succeeded: the plan does)
fycg::GemmPlan executed_plan(const fyc_gemm_args& a) {
  fycg::GemmPlan pl;
  char err[512];
  (void)fycg::plan_gemm(&a, (a.chan_parts != nullptr ? fycg::GEMM_STATS_CHAN : 0) | (a.row_parts != nullptr ? fycg::GEMM_STATS_ROW : 0), false, pl, err);
  return pl;
}

// ---- second mode: the cases of a file ---------------------------------------------------------------------------------------------
bool parse_case(const std::string& line, Case& c, std::string& why) {
  std::vector<std::string> tok;
  for (size_t i = 0; i < line.size();) {
    while (i < line.size() && (line[i] == ' ' || line[i] == '\t')) ++i;
    size_t j = i;
    while (j < line.size() && line[j] != ' ' && line[j] != '\t') ++j;
    if (j > i) tok.push_back(line.substr(i, j - i));
    i = j;
  }
  if (tok.empty()) { why = "empty line"; return false; }
  c = Case();
  c.name = tok[0];
  fyc_gemm_args& a = c.a;
  memset(&a, 0, sizeof(a));
  a.a = fake(P_A); a.w = fake(P_W); a.out = fake(P_OUT);
  a.batch = 1; a.out_scale = 1.f; a.epilogue = FYC_EPI_LINEAR; a.conv_stride = 1; a.conv_pad = 1;
  long long out_off = 0, rb_off = 0, res_off = 0;
  int res = 0;
  for (size_t t = 1; t < tok.size(); ++t) {
    const size_t eq = tok[t].find('=');
    if (eq == std::string::npos) { why = "field without '=': " + tok[t]; return false; }
    const std::string k = tok[t].substr(0, eq), vs = tok[t].substr(eq + 1);
    if (k == "tune") {
      const size_t colon = vs.find(':');
      if (colon == std::string::npos) { why = "tune wants <key>:<value>"; return false; }
      c.tuning.push_back({atoi(vs.substr(0, colon).c_str()), atoi(vs.substr(colon + 1).c_str())});
      continue;
    }
    if (k == "seg_tr" || k == "seg_ld" || k == "seg_off") {      // comma-separated, one entry per segment
      int s = 0;
      for (size_t i = 0; i <= vs.size() && s < 3; ++s) {
        size_t j = vs.find(',', i);
        if (j == std::string::npos) j = vs.size();
        const long long e = atoll(vs.substr(i, j - i).c_str());
        if (k == "seg_tr") a.seg_transposed[s] = (int)e;
        else if (k == "seg_ld") a.seg_ld[s] = (int)e;
        else a.seg_out[s] = (char*)fake(P_SEG + s) + e;
        i = j + 1;
      }
      continue;
    }
    const long long v = atoll(vs.c_str());
    if (k == "epilogue") a.epilogue = (int)v; else if (k == "act") a.act = (int)v;
    else if (k == "ln") { a.ln_stats = v ? (const float*)fake(P_LNS) : nullptr; a.ln_colsum = v ? (const float*)fake(P_LNC) : nullptr; a.ln_eps = 1e-5f; }
    else if (k == "ln_nparts") a.ln_nparts = (int)v;
    else if (k == "a2") a.a2 = v ? fake(P_A2) : nullptr; else if (k == "k_split") a.k_split = (int)v; else if (k == "lda2") a.lda2 = (int)v;
    else if (k == "seg_cols") a.seg_cols = (int)v; else if (k == "heads") a.heads = (int)v; else if (k == "tokens") a.tokens = (int)v;
    else if (k == "dtype") a.dtype = (int)v; else if (k == "mode") a.mode = (int)v;
    else if (k == "M") a.M = (int)v; else if (k == "N") a.N = (int)v; else if (k == "K") a.K = (int)v;
    else if (k == "lda") a.lda = (int)v; else if (k == "ldw") a.ldw = (int)v; else if (k == "ldo") a.ldo = (int)v;
    else if (k == "ldr") a.ldr = (int)v; else if (k == "ldrb") a.ldrb = (int)v; else if (k == "rpb") a.rows_per_batch = (int)v;
    else if (k == "tile") a.tile = (int)v; else if (k == "batch") a.batch = (int)v;
    else if (k == "stride_a") a.stride_a = v; else if (k == "stride_w") a.stride_w = v; else if (k == "stride_o") a.stride_o = v;
    else if (k == "cs_rows") a.cs_rows = (int)v;
    else if (k == "Hout") a.Hout = (int)v; else if (k == "Wout") a.Wout = (int)v; else if (k == "Hin") a.Hin = (int)v; else if (k == "Win") a.Win = (int)v;
    else if (k == "Cin") a.Cin = (int)v; else if (k == "stride") a.conv_stride = (int)v; else if (k == "pad") a.conv_pad = (int)v;
    else if (k == "t3_frames") a.t3_frames = (int)v; else if (k == "t3_rows") a.t3_rows = (int)v;
    else if (k == "bias") a.bias = v ? (const float*)fake(P_BIAS) : nullptr;
    else if (k == "rowbias") a.rowbias = v ? (const float*)fake(P_RB) : nullptr;
    else if (k == "chan") a.chan_parts = v ? (float*)fake(P_CP) : nullptr;
    else if (k == "residual") res = (int)v;
    else if (k == "out_off") out_off = v; else if (k == "rb_off") rb_off = v; else if (k == "res_off") res_off = v;
    else { why = "unknown key " + k; return false; }
  }
  a.out = (char*)a.out + out_off;
  if (a.rowbias != nullptr) a.rowbias = (const float*)((const char*)a.rowbias + rb_off);
  if (res == 2) a.residual = a.out;
  else if (res == 1) a.residual = (char*)fake(P_RES) + res_off;
  if (a.mode != FYC_GEMM_CONV3X3) { a.conv_stride = 0; a.conv_pad = 0; }
  return true;
}

int run_file(FILE* f) {
  int bad = 0;
  char buf[4096];
  while (fgets(buf, sizeof(buf), f) != nullptr) {
    std::string line = buf;
    while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
    if (line.empty() || line[0] == '#') continue;
    Case c;
    std::string why;
    if (!parse_case(line, c, why)) { fprintf(stderr, "gemm_plan_harness: %s in: %s\n", why.c_str(), line.c_str()); return 4; }
    fyc_gemm_args& a = c.a;
    for (auto& kv : c.tuning) fyc_set_tuning(kv.first, kv.second);
    const long long need = (long long)fyc_gemm_workspace_bytes(&a);
    if (need > 0) { a.workspace = fake(P_WS); a.workspace_bytes = need; }
    g_rec = Rec{"-", 0, 0, 0, 0, 0, 0, 0, 0};
    int rc = fyc_gemm(&a, nullptr);
    std::string msg = rc != 0 ? fyc_last_error() : "";
    if (rc == -3 && g_rec.calls == 1 && g_rec.splitk > 1 && msg.find("fyc_gemm split-K finish") == 0) { rc = 0; msg.clear(); }   // (no device: see the head of the file)
    (void)hipGetLastError();
    if (msg.size() > 160) msg.resize(160);
    fycg::GemmPlan pl = {};
    std::string decided = "-";
    if (rc == 0 && g_rec.calls == 1) {
      pl = executed_plan(a);
      const fycg::GemmGeom g = {fycg::gemm_tile(pl.run_cfg), pl.run_ns, pl.wide != 0, g_rec_p.act != FYC_ACT_NONE ? fycg::EPI_LINEAR_ACT : g_rec_p.epilogue, g_rec_p.mode,
                                fycg::gemm_is16(pl.dtype) ? 2 : 4};
      if (fycg::gemm_built(g)) {
        const fycg::GemmLaunch d = fycg::gemm_launch_plan(g_rec_p, g, g_fyc_tuning, 256, g_rec.batch);
        char buf[192];
        snprintf(buf, sizeof(buf), "pre=%d fast1=%d heads_pk=%d res_acc=%d rb_tile=%d rb_slots=%d strip=%d lds=%d grid=%u", d.pre, d.fast1, d.heads_pk, d.res_acc, d.rb_tile,
                 d.rb_slots, d.strip, d.smem, d.grid);
        decided = buf;
      }
    } else {
      ++bad;
    }
    printf("%s | %s %d %d %d %d %d %d %d | %d %dx%d | %d%s%s | %s\n", c.name.c_str(), g_rec.fam, g_rec.cfg, g_rec.ns, g_rec.wide, g_rec.colc, g_rec.splitk, g_rec.cs_slots,
           g_rec.batch, pl.run_cfg, pl.run_bm, pl.run_bn, rc, msg.empty() ? "" : " ", msg.c_str(), decided.c_str());
    for (auto& kv : c.tuning) fyc_set_tuning(kv.first, 0);
  }
  fflush(stdout);
  return bad ? 1 : 0;
}
}  // namespace

int main(int argc, char** argv) {
  setenv("HIP_VISIBLE_DEVICES", "-1", 1);
  setenv("ROCR_VISIBLE_DEVICES", "-1", 1);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
    fprintf(stderr, "gemm_plan_harness: a GPU is visible; this program passes made-up pointers and must not launch anything\n");
    return 3;
  }
  (void)hipGetLastError();
  void* zero = aligned_alloc(256, 4096);
  memset(zero, 0, 4096);
  if (fyc_init(zero) != 0) return 2;
  if (argc > 1) {
    FILE* f = strcmp(argv[1], "-") == 0 ? stdin : fopen(argv[1], "r");
    if (f == nullptr) { fprintf(stderr, "gemm_plan_harness: cannot read %s\n", argv[1]); return 4; }
    return run_file(f);
  }
  int bad = 0;
  for (Case& c : grid()) {
    fyc_gemm_args& a = c.a;
    for (auto& kv : c.tuning) fyc_set_tuning(kv.first, kv.second);
    const int rp = fyc_gemm_row_parts(&a);
    if (c.want_rp) a.row_nparts = rp;
    const long long need = (long long)fyc_gemm_workspace_bytes(&a);
    int32_t tile_rows = 0, slots = 0;
    const int nt = fyc_gemm_stat_layout(&a, &tile_rows, &slots);
    if (need > 0 && !c.no_ws) { a.workspace = fake(P_WS); a.workspace_bytes = need; }
    g_rec = Rec{"-", 0, 0, 0, 0, 0, 0, 0, 0};
    int rc = fyc_gemm(&a, nullptr);
    std::string msg = rc != 0 ? fyc_last_error() : "";
    if (rc == -3 && g_rec.calls == 1 && g_rec.splitk > 1 && msg.find("fyc_gemm split-K finish") == 0) { rc = 0; msg.clear(); }   // (no device: see the head of the file)
    (void)hipGetLastError();
    const size_t c1 = msg.find(':'), c2 = c1 == std::string::npos ? c1 : msg.find(':', c1 + 1);
    if (c2 != std::string::npos) msg.resize(c2);
    if (msg.size() > 100) msg.resize(100);
    std::string flags;
    if (rc == 0 && g_rec.calls == 1) {
      const fycg::GemmPlan pl = executed_plan(a);
      const int bm = pl.run_bm, bn = pl.run_bn;
      const bool split = g_rec.splitk > 1;
      if (a.chan_parts != nullptr) {
        fyc_gemm_args q = a;
        q.a = q.a2 = q.w = q.residual = nullptr; q.out = nullptr; q.bias = q.rowbias = q.ln_stats = q.ln_colsum = nullptr;
        q.chan_parts = q.row_parts = nullptr; q.workspace = nullptr; q.workspace_bytes = 0;
        for (int s = 0; s < 3; ++s) q.seg_out[s] = nullptr;
        int32_t q_rows = 0, q_slots = 0;
        (void)fyc_gemm_stat_layout(&q, &q_rows, &q_slots);
        const bool q_split = fyc_gemm_workspace_bytes(&q) > 0;
        if ((split ? 128 : bm) != q_rows || g_rec.cs_slots != q_slots || split != q_split) flags += " !I1";
      }
      if (a.row_parts != nullptr && a.row_nparts != (a.N + bn - 1) / bn) flags += " !I2";
      if (!c.no_ws && (need > 0) != split) flags += " !I3";
    } else if (rc == 0) {
      flags += " !launches";
    }
    if (!flags.empty()) ++bad;
    printf("%s | %lld %d %d/%d/%d | %s %d %d %d %d %d %d %d | %d%s%s%s\n", c.name.c_str(), need, rp, nt, (int)tile_rows, (int)slots, g_rec.fam, g_rec.cfg, g_rec.ns,
           g_rec.wide, g_rec.colc, g_rec.splitk, g_rec.cs_slots, g_rec.batch, rc, msg.empty() ? "" : " ", msg.c_str(), flags.c_str());
    for (auto& kv : c.tuning) fyc_set_tuning(kv.first, 0);
  }
  fflush(stdout);
  return bad ? 1 : 0;
}
