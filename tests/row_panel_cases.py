"""The cases of the row-panel kernels (csrc/panel_linear.hip, csrc/ff_block.hip, csrc/temporal_block.hip, csrc/temporal_block_rr.hip) as data: what a case launches (traits(): the instantiation and the host-side
branches restated from the kernel source, each with the line it mirrors), its operands from seeded generators, its output inside a guarded buffer, its reference from
EmuOps(acc=torch.float64) with a per-element bound (derivation: tests/kernel_compare.py) and a torch model of the kernel's rounding points (f32 tensors combined in the
kernel's order) with the defects the bound is there to catch.  A helper, not a test module; no GPU is touched here.
tests/test_row_panel_cases.py (CPU: coverage, model inside the bound, defects outside, share caps) and tests/test_row_panel_bounds_gpu.py use it.

Every output - the chan_parts buffer of fyc_ff_block included - is a window [rows][cols] of a flat buffer prefilled with the bit pattern FILL: 64 elements in front,
two rows behind.  With an aliased residual the window holds the residual before the launch.

Defects (applied in the model; a case lists the ones that must leave its bound):
  panel_linear  tile_copy   tile 1 holds tile 0's rows                       sample0     the sample index ignores gn_rows_per_sample: sample 0's statistics everywhere
                fold_short  one statistics sample too few is folded          drop_kstep  the last 32-wide k-step is dropped
                pass_w      the second column pass uses the first's weights  pass_bias   ... the first pass's bias      res_cols  the residual of the other pass's columns
  ff_block      drop39      chunk 39 is dropped                              bias_prev   chunk c uses chunk c - 1's bias
                swap_vg     value and gate are swapped in chunk 17           proj_xn     the projection reads the normalised tokens
                mean0       the large-mean rows are normalised with mean 0   stats_slot  the statistics of tile 1 are written to tile 0's slot
  temporal      mask_last   the last frame is masked                         pe_next     the positional term of frame f + 1 is used
                head_shift  head 3's stripe holds head 4's attention output  swap_tiles  the two pixel tiles of a clip are swapped      swap_clips  the two clips are swapped

What these cases do NOT see, and why (the share caps XN_CAP / HID_CAP are conditions on the inputs that every case has to meet):
  * the f16 fyc_ff_block cases give six of the 32 hidden units of a chunk a value path (other six in every chunk); the other 26 are exact zeros.  A defect confined to one
    (chunk, register slot) pair of the GEGLU / FF2 path is seen in f16 only where that pair is live; the bf16 cases have all of them live.  A dense f16 case would have every
    hidden element beside a rounding boundary, i.e. a share of 100 %;
  * the constant rows have a value whose f32 mean is exact, so x - mean is 0 and a wrong rstd on that row (rsqrt(eps), about 362) multiplies 0 and cannot be seen.  A constant
    whose f32 mean is one ulp off makes all 320 normalised values of the row 362 ulp_f32 instead of 0: a row with 100 % of its elements charged;
  * the error of the LayerNorm statistics is COMPUTED by ff_stats_sim / tb_stats_sim, which repeat the order of additions of ff_block.hip:136-156, temporal_block_rr.hip:109-129
    and temporal_block.hip:70-84.  A reordering of those loops that is harmless in itself moves the kernel's mean by an ulp and can fail these tests: the simulations then
    have to follow the new order;
  * the temporal bound is wide (tens of bf16 ulps): the attention output is charged on every element, and the charge goes through |Wo| of all 320 columns in absolute value.
"""
import math
import zlib
from dataclasses import dataclass, replace
from functools import lru_cache
from types import SimpleNamespace as NS
from typing import Tuple

import torch

import kernel_compare as KC
import norm_cases as NC
from emu_ops import EmuOps

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
FRONT, BACK_ROWS = 64, 2
FILL = {2: 0x7B7B, 4: 0x7B7B7B7B}      # as attention_cases.FILL: finite in every type, no NaN, unlikely as an output
u = 2.0 ** -24
D53 = 2.0 ** -53
# the global tolerances of the existing tests of the same op (test_kernels_gpu.py, test_kernels_f16_gpu.py)
RTOL = {"panel_linear": {"bf16": 5e-3, "f16": 1e-3}, "ff_block": {"bf16": 6e-3, "f16": 1.5e-3}, "temporal_block": {"bf16": 6e-3, "f16": 1.5e-3}}
GN_EPS, LN_EPS = 2.0 ** -20, 2.0 ** -17      # exact in f32: the kernels take eps as a float
C_FF, HID = 320, 1280
CHUNKS = HID // 32
PARTS_L = 22 + 6      # ff_block.hip:347 (rows rsl, rsl + 6, ... < 128: at most 22 per thread), :374 (the 6 row slices added in order)
XN_CAP, HID_CAP = 0.01, 0.25      # the largest share of boundary-charged elements in any row

# geglu_one (csrc/fyc_common.h): Phi(g) = 0.5 + 0.5 xc R(xc^2), xc = clamp(g, -4.2, 4.2); the coefficients as the f32 numbers the compiler makes of the literals
GEGLU_CLAMP = 4.2
GEGLU_COEF = (-1.803605736e-09, 1.588336848e-07, -6.076054488e-06, 1.337840930e-04, -1.901335453e-03, 1.859653848e-02, -1.310565435e-01, 7.969318188e-01)
DG = 1.13      # |d/dg (g Phi(g))| = |Phi(g) + g phi(g)| <= 1.1290 (at g = sqrt 2); asserted on a grid by tests/test_row_panel_cases.py


def f32c(v):
    return float(torch.tensor(v, dtype=torch.float32))


def Phi(g):
    return 0.5 * (1.0 + torch.special.erf(g / math.sqrt(2.0)))


def phi_poly(g):
    """the polynomial of geglu_one in f64 (no f32 rounding: its roundings are charged separately)"""
    xc = g.double().clamp(-f32c(GEGLU_CLAMP), f32c(GEGLU_CLAMP))
    t = xc * xc
    r = torch.full_like(t, f32c(GEGLU_COEF[0]))
    for c in GEGLU_COEF[1:]:
        r = r * t + f32c(c)
    return 0.5 + 0.5 * xc * r


def phi_poly_error(lo=-8.0, hi=8.0, n=(1 << 21) + 1):
    """max |Phi_poly(g) - Phi(g)| over a dense grid (beyond the clamp the polynomial is constant, and so is the error's growth: 1 - Phi(4.2) at most)"""
    g = torch.linspace(lo, hi, n, dtype=torch.float64)
    return float((phi_poly(g) - Phi(g)).abs().max())


def phi_rounding(g):
    """the f32 evaluation of the polynomial against its exact value: xc^2, seven fmaf (16 u of sum |c_i| xc^2i on r, Horner), xc * r and the last fmaf (3 u)"""
    xc = g.double().clamp(-GEGLU_CLAMP, GEGLU_CLAMP)
    t = xc * xc
    A = torch.zeros_like(t)
    for cf in GEGLU_COEF:
        A = A * t + abs(cf)
    return 0.5 * xc.abs() * 16 * u * A + 3 * u


PHI_ERR = phi_poly_error()      # what the bound of the gate uses; never a number copied from a comment


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Panel:
    name: str
    dt: str
    rows: int
    K: int
    N: int
    gn: str = "none"                # "none", "cs" (f64 channel sums), "parts" (row-tile partials folded by the kernel)
    rps: int = 0                    # gn_rows_per_sample
    ss: int = 1                     # gn_stat_samples
    groups: int = 32
    bm: int = 0                     # parts: rows per producer tile (gn_tile_rows)
    bias: bool = True
    res: str = "none"               # "none", "sep", "alias" (residual == out)
    defects: Tuple[str, ...] = ()
    op = "panel_linear"

    @property
    def cols(self):
        return self.N

    @property
    def problem(self):
        return replace(self, name="", defects=())


@dataclass(frozen=True)
class FF:
    name: str
    dt: str
    rows: int
    res: str = "sep"
    cs_rows: int = 0                # 0: no chan_parts
    recipe: str = "random"          # "random", "integer" (identity projection, zero FF weights, integer tokens and residual: exact output statistics)
    defects: Tuple[str, ...] = ()
    op = "ff_block"

    @property
    def cols(self):
        return C_FF

    @property
    def problem(self):
        return replace(self, name="", defects=())


SALT = 0      # part of every seed.  The share caps (XN_CAP, HID_CAP) are a condition on the INPUTS, checked from the reference alone by tests/test_row_panel_cases.py.  With 320
# elements in a row the 1 % cap is three elements.  The recipes keep the expected number low by construction - LayerNorm rows of distinct tokens (distinct_tokens), f16 operands
# away from zero: 0.05 (bf16) to 0.25 (f16) per row - but the list has ~2 10^4 rows, and a row with four does turn up for about every second value of this constant (five of
# 0 .. 9 keep every row of every case under both caps).  Should an edit of a recipe push a row over, change the recipe or this, never the caps.


def _seed(c):
    return zlib.crc32((repr(c.problem) + f"/{SALT}").encode()) & 0x7FFFFFF


def rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def distinct_tokens(rows, C, T, seed, lo, hi, pos=0.6):
    """[rows][C] of type T: every row holds C DIFFERENT numbers of T with lo <= |x| < hi, the share `pos` of them positive (a row mean away from zero).  Tokens drawn from a
    continuous law repeat within a row once they are rounded to 16 bits (a bf16 binade has 128 numbers), equal tokens have equal normalised values, and those sit beside a
    rounding boundary together: one unlucky value then costs a row several of the three elements XN_CAP allows it"""
    bits = torch.arange(1, 0x7C00 if T == torch.float16 else 0x7F80, dtype=torch.int32).to(torch.int16).view(T)
    cand = bits[(bits.float() >= lo) & (bits.float() < hi)]
    g = torch.Generator().manual_seed(seed)
    npos = int(round(pos * C))
    assert cand.numel() >= npos
    out = torch.empty(rows, C, dtype=T)
    for r in range(rows):
        row = torch.cat([cand[torch.randperm(cand.numel(), generator=g)[:npos]], -cand[torch.randperm(cand.numel(), generator=g)[:C - npos]]])
        out[r] = row[torch.randperm(C, generator=g)]
    return out


# ---- what a case executes ---------------------------------------------------------------------------------------------------------------
def traits(c):
    if c.op == "panel_linear":
        t = dict(inst=(c.dt, c.K // 32, c.N // 320),            # panel_linear.hip:237-242 launch<T, KS, NPASS> by dtype, K == 320, N == 320
                 tiles=c.rows // 128,                          # :202 dim3(rows / ROWS)
                 gn=c.gn,                                      # :83 if (p.gn_cs != nullptr || p.gn_parts.parts != nullptr), :93 parts or sums
                 bias=c.bias,                                  # :175 if (p.bias != nullptr)
                 residual=c.res,                               # :150, :177 if (p.res != nullptr); :229 residual may alias out
                 passes=c.N // 320)                            # :141 for (pass < NPASS), :193 the barrier between passes
        if c.gn != "none":
            t.update(tiles_per_sample=c.rps // 128,            # :88 sample = row0 / gn_rows_per_sample
                     samples=c.rows // c.rps, stat_samples=c.ss,      # :96 for (f < gn_stat_samples)
                     cpg=c.K // c.groups,                      # :88 cpg = K / gn_groups, :107 the loop over a group's channels
                     channel_laps=-(-c.K // 256))              # :91 for (c = tid; c < K; c += NT)
        if c.gn == "parts":
            cs_rows = c.rps // c.ss                            # :235 ChanParts.cs_rows = gn_rows_per_sample / gn_stat_samples
            slots = NC.slots_of(c.bm, cs_rows)
            fast = slots == 1 and cs_rows % c.bm == 0          # chan_parts.h:30
            t0, t1 = NC.tile_range(c.bm, cs_rows, c.rows, 0, c.ss)
            n = t1 - t0 + 1
            t.update(fold="fast" if fast else "general", slots=slots, fold_unrolled=fast and n >= 4,      # chan_parts.h:34 for (; t + 3 <= r.t1; t += 4)
                     fold_tail=fast and n % 4 != 0,                                                        # chan_parts.h:47
                     missing_samples=bool(torch.isnan(NC.build_parts(torch.zeros(c.rows, 1), c.bm, cs_rows, slots)).any()))
        return t
    if c.op == "ff_block":
        return dict(inst=c.dt,                                 # ff_block.hip:413 ff_block_kernel<f16_t> or <bf16_t>
                    tiles=c.rows // 128,                       # :410 ntiles = rows / ROWS
                    residual=c.res,                            # :304, :329 if (p.res != nullptr)
                    parts=c.cs_rows > 0,                       # :350, :360 if (p.parts != nullptr)
                    cs_rows=c.cs_rows)                         # :398 cs_rows % ROWS == 0 && rows % cs_rows == 0
    if c.op == "temporal_block":
        return dict(inst=(c.dt, "rr" if c.rr else "lds"),      # temporal_block.hip:298 wstream != nullptr -> the rr launcher; :305 / temporal_block_rr.hip:353 <f16_t> or <bf16_t>
                    workgroups=c.clips * (c.P // 8),           # :305 dim3(clips * (pixels / PIX))
                    tiles_per_clip=c.P // 8,                   # :55-56 clip = blockIdx.x / tiles_per_clip, p0 = ...
                    pe=c.pe)                                   # temporal_block.hip:163 if (p.pe_bias); the rr kernel has it folded into the stream's tables
    raise KeyError(c.op)


def built():
    """every instantiation of the four files"""
    return ({("panel_linear", (dt, ks, np_)) for dt in DT for ks in (10, 20) for np_ in (1, 2)} | {("ff_block", dt) for dt in DT}
            | {("temporal_block", (dt, k)) for dt in DT for k in ("rr", "lds")})


# ---- guarded buffers and rounding helpers ---------------------------------------------------------------------------------------------------
def guarded(rows, cols, T):
    n = FRONT + (rows + BACK_ROWS) * cols
    size = torch.empty(0, dtype=T).element_size()
    buf = torch.full((n,), FILL[size], dtype={2: torch.int16, 4: torch.int32}[size]).view(T)
    mask = torch.zeros(n, dtype=torch.bool)
    mask[FRONT:FRONT + rows * cols] = True
    return buf, mask


def window(buf, rows, cols):
    return buf[FRONT:FRONT + rows * cols].view(rows, cols)


def round_T(x, T):
    return x.to(T).double()


def spread(x, e, T):
    """how far the T number of a value within e of x can lie from the T number of x: 0 where no rounding boundary of T is within e of x, else >= ulp_T"""
    mid, lo, hi = round_T(x, T), round_T(x - e, T), round_T(x + e, T)
    return torch.maximum(hi - mid, mid - lo)


def fma32(a, b, c):
    """fmaf on f32 tensors, correctly rounded: the product of two f32 numbers is exact in f64; the f64 sum t is rounded once more on its way to f32, which can only go the
    wrong way where t is exactly the middle of two f32 numbers (25 bits) and the exact sum is not: there the residual of the sum (TwoSum) decides"""
    p, q = a.double() * b.double(), c.double()
    p, q = torch.broadcast_tensors(p, q)
    t = p + q
    bb = t - p
    err = (p - (t - bb)) + (q - bb)
    r = t.float()
    d = r.double() - t                                  # > 0: rounded up
    nxt = torch.nextafter(r, torch.where(d > 0, -torch.ones_like(r), torch.ones_like(r)) * float("inf"))      # the f32 neighbour on the other side of t
    tie = (d != 0) & ((nxt.double() - t).abs() == d.abs())
    wrong = tie & (((d > 0) & (err < 0)) | ((d < 0) & (err > 0)))
    return torch.where(wrong, nxt, r)


def labels(c):
    if c.op == "temporal_block":
        return tb_labels(c)
    if c.op == "panel_linear":
        return KC.Labels(lambda i: f"tile {i // 128}, wave {i % 128 // 32}, row {i % 32} of it" + (f", sample {i // c.rps}" if c.gn != "none" else ""),
                         lambda j: f"pass {j // 320}, column block {j % 320 // 16}, lane column {j % 16}")
    return KC.Labels(lambda i: f"tile {i // 128}, wave {i % 128 // 32}, token {i % 32} of it", lambda j: f"feature block {j // 32}, feature {j % 32} of it")


# =========================================================================================================================================
# fyc_panel_linear
# =========================================================================================================================================
SAMPLE_MS = [(0.4, 1.3), (-1.0, 2.0), (1.5, 3.0), (0.2, 0.6)]      # (mean, scale) of the rows of GroupNorm sample s: the samples' statistics differ strongly


def panel_operands(c):
    from followyourclick_amd.engine.weights import pack_panel_linear
    T, s = DT[c.dt], _seed(c)
    w = (rnd((c.N, c.K), s + 1) * c.K ** -0.5).to(T)
    o = NS(w=w, ws=pack_panel_linear(w), win=(c.rows, c.N))
    o.bias = (rnd((c.N,), s + 2) * 0.2 + torch.linspace(-0.3, 0.3, c.N)).float() if c.bias else None      # distinct per column, of order 0.2
    x = rnd((c.rows, c.K), s + 3)
    if c.gn == "none":
        x = x * 1.3 + 0.4
    else:
        S = c.rows // c.rps
        ms = torch.tensor([SAMPLE_MS[i % 4] for i in range(S)])
        x = (x.view(S, c.rps, c.K) * ms[:, 1, None, None] + ms[:, 0, None, None]).reshape(c.rows, c.K)
    o.x = x.to(T)
    o.res = rnd((c.rows, c.N), s + 4).to(T) if c.res != "none" else None
    if c.gn != "none":
        # bf16: gamma near 1, beta near 0.  f16: the normalised operand is kept away from zero (gamma near 0.5, beta near 2.5): towards zero the f16 grid becomes finer
        # than the f32 error of scale and shift (which stays of the size of u |x sc|), and a row would have more than XN_CAP of its elements beside a boundary
        o.gamma = (rnd((c.K,), s + 5) * (0.2 if c.dt == "bf16" else 0.1) + (1.0 if c.dt == "bf16" else 0.5)).float()
        o.beta = (rnd((c.K,), s + 6) * 0.2 + (0.0 if c.dt == "bf16" else 2.5)).float()
        cs_rows = c.rps // c.ss
        if c.gn == "cs":
            xs = o.x.double().reshape(c.rows // cs_rows, cs_rows, c.K)
            o.gn_cs = torch.stack([xs.sum(1), (xs * xs).sum(1)], dim=-1).contiguous()      # [samples * ss][K][2]
        else:
            o.slots = NC.slots_of(c.bm, cs_rows)
            o.parts = NC.build_parts(o.x, c.bm, cs_rows, o.slots).contiguous()           # NaN where a statistics sample does not exist
    o.buf, o.mask = guarded(c.rows, c.N, T)
    if c.res == "alias":
        window(o.buf, c.rows, c.N).copy_(o.res)
    return o


def panel_sums(c, ops, defect=None):
    """[samples][K][2] f64: the channel sums of every GroupNorm sample, its statistics samples added in order"""
    S = c.rows // c.rps
    if c.gn == "cs":
        per = ops.gn_cs.reshape(S, c.ss, c.K, 2)
    else:
        per = torch.stack([NC.fold(ops.parts, c.bm, c.rps // c.ss, c.rows, f, 1)[0] for f in range(S * c.ss)]).reshape(S, c.ss, c.K, 2)
    if defect == "fold_short":
        per = per[:, :-1]
    return per.sum(dim=1)


def panel_group_stats(c, sums):
    S, cpg = sums.shape[0], c.K // c.groups
    st = sums.reshape(S, c.groups, cpg, 2).sum(dim=2)
    cnt = c.rps * cpg
    mean = st[..., 0] / cnt
    ex2 = st[..., 1] / cnt
    var = (ex2 - mean * mean).clamp_min(0.0)
    expand = lambda t: t[:, :, None].expand(S, c.groups, cpg).reshape(S, c.K)      # noqa: E731
    return expand(mean), expand(var), expand(ex2)


def panel_reference(c, ops):
    T, emu = DT[c.dt], EmuOps(acc=torch.float64)
    out = torch.zeros(c.rows, c.N, dtype=T)
    kw = {}
    if c.gn != "none":
        sums = ops.gn_cs if c.gn == "cs" else panel_sums(c, ops)
        kw = dict(gn_cs=sums, gn_gamma=ops.gamma, gn_beta=ops.beta, gn_rows_per_sample=c.rps, gn_stat_samples=c.ss if c.gn == "cs" else 1, gn_groups=c.groups, gn_eps=GN_EPS)
    emu.panel_linear(ops.x, out, wstream=ops.ws, rows=c.rows, N=c.N, K=c.K, bias=ops.bias, residual=ops.res, **kw)
    W, X = ops.w.double(), ops.x.double()
    charge = torch.zeros(c.rows, c.K, dtype=torch.float64)
    if c.gn != "none":
        S = c.rows // c.rps
        mean, var, ex2 = panel_group_stats(c, panel_sums(c, ops))
        rstd = 1.0 / torch.sqrt(var + GN_EPS)
        sc = rstd * ops.gamma.double()
        sh = ops.beta.double() - mean * sc
        rep = lambda t: t[:, None, :].expand(S, c.rps, c.K).reshape(c.rows, c.K)      # noqa: E731
        sc_r, sh_r, m_r = rep(sc), rep(sh), rep(mean)
        xn = X * sc_r + sh_r
        # panel_linear.hip:109-115, :131: var = q / cnt - mean^2 in f64 (cancellation: 8 2^-53 (q / cnt + mean^2) on var, half of that relative to var + eps on rstd; 64 2^-53
        # for the order of the f64 sums), rstd -> f32 (u), sc = rstd * gamma (u), (float)mean (u), mean * sc (u), beta - that (u |sh|), one fma per element (u |xn|)
        rel64 = rep(8 * D53 * (ex2 + mean * mean) / (2 * (var + GN_EPS))) + 64 * D53
        e = ((X * sc_r).abs() * (2 * u + rel64) + (m_r * sc_r).abs() * (4 * u + rel64) + u * sh_r.abs() + u * xn.abs()) * (1 + 16 * u)
        charge = spread(xn, e, T)
        X = round_T(xn, T)
        ops.info = NS(xn_share=(charge > 0).double().mean(dim=1).max().item())
    else:
        ops.info = NS(xn_share=0.0)
    S_ = X.abs() @ W.abs().t()
    if c.bias:
        S_ = S_ + ops.bias.double().abs()
    if c.res != "none":
        S_ = S_ + ops.res.double().abs()
    ref = ops.buf.clone()
    window(ref, c.rows, c.N).copy_(out)
    bound = KC.ulp(out.double(), c.dt) + (c.K + 8) * u * S_ + charge @ W.abs().t()
    return ref, bound


def panel_model(c, ops, defect=None):
    T = DT[c.dt]
    a, W = ops.x.float(), ops.w.float()
    if c.gn != "none":
        S = c.rows // c.rps
        mean, var, _ = panel_group_stats(c, panel_sums(c, ops, defect))
        rstd = (1.0 / torch.sqrt(var + GN_EPS)).float()
        sc = rstd * ops.gamma
        sh = ops.beta - mean.float() * sc
        if defect == "sample0":
            sc, sh = sc[:1].expand(S, c.K), sh[:1].expand(S, c.K)
        a = fma32(a.view(S, c.rps, c.K), sc[:, None], sh[:, None]).reshape(c.rows, c.K).to(T).float()
    ks = c.K // 32 - (1 if defect == "drop_kstep" else 0)
    y = torch.empty(c.rows, c.N)
    for p in range(c.N // 320):
        wp = 0 if defect == "pass_w" else p
        acc = torch.zeros(c.rows, 320)
        for s in range(ks):
            acc = acc + a[:, 32 * s:32 * s + 32] @ W[320 * wp:320 * wp + 320, 32 * s:32 * s + 32].t()
        if c.bias:
            bp = 0 if defect == "pass_bias" else p
            acc = acc + ops.bias[320 * bp:320 * bp + 320]
        if c.res != "none":
            rp = c.N // 320 - 1 - p if defect == "res_cols" else p
            acc = acc + ops.res[:, 320 * rp:320 * rp + 320].float()
        y[:, 320 * p:320 * p + 320] = acc
    y = y.to(T)
    if defect == "tile_copy":
        y[128:256] = y[0:128]
    buf = ops.buf.clone()
    window(buf, c.rows, c.N).copy_(y)
    return buf


def panel_defects(c):
    d = ["tile_copy", "drop_kstep"]
    if c.gn != "none" and c.rows // c.rps >= 2:
        d.append("sample0")
    if c.gn != "none" and c.ss >= 2:
        d.append("fold_short")
    if c.N == 640:
        d += ["pass_w"] + (["pass_bias"] if c.bias else []) + (["res_cols"] if c.res != "none" else [])
    return tuple(d)


# =========================================================================================================================================
# fyc_ff_block
# =========================================================================================================================================
BIG_ROWS, CONST_ROWS = (5, 133), (9, 200)      # rows with a large mean (x * 40 + 100) and constant rows (variance 0), one of each in tiles 0 and 1
ACTIVE_F16 = 6                                  # f16: hidden units per chunk of 32 with a value path (see ff_operands)
SWAP_CHUNK = 17


def ff_stats_sim(x32, eps, zero_mean_rows=()):
    """ff_block.hip:136-156 in f32, operation by operation (the bound DEPENDS on this order: see the module docstring): lane (token, kh) adds its 160 values as pairs, k-step by k-step (:139-143), the two lanes of a row meet
    (halves_sum), * (1.0f / C); then the sum of squares about that mean by fmaf (:147-155).  Additions and fmaf are correctly rounded and their order is fixed (no
    contraction: -ffp-contract=off), so mean and variance are the kernel's bit for bit; rsqrtf is not (1 ulp), hence 1 / sqrt correctly rounded here."""
    rows = x32.shape[0]
    X = x32.reshape(rows, 20, 2, 4, 2)      # [row][k-step][kh][pair e][lo, hi]
    inv = torch.tensor(1.0 / C_FF, dtype=torch.float32)
    s = torch.zeros(rows, 2)
    for k in range(20):
        for e in range(4):
            s = s + (X[:, k, :, e, 0] + X[:, k, :, e, 1])
    mu = (s[:, 0] + s[:, 1]) * inv
    for r in zero_mean_rows:
        mu[r] = 0.0
    q = torch.zeros(rows, 2)
    m = mu[:, None]
    for k in range(20):
        for e in range(4):
            a, b = X[:, k, :, e, 0] - m, X[:, k, :, e, 1] - m
            q = fma32(a, a, q)
            q = fma32(b, b, q)
    v = (q[:, 0] + q[:, 1]) * inv + torch.tensor(eps, dtype=torch.float32)
    rs = (1.0 / v.double().sqrt()).float()
    return mu, rs, x32 - m, v


def ff_operands(c):
    from followyourclick_amd.engine.weights import Packed, pack_ff_block
    T, s, C, rows = DT[c.dt], _seed(c), C_FF, c.rows
    o = NS(win=(rows, C), big_rows=(), const_rows=())
    if c.recipe == "integer":
        g = torch.Generator().manual_seed(s)
        # every row a permutation of the same integers: one mean, one rstd and seven normalised values for the whole case (they feed zero weights, but the cap on the share of
        # boundary-charged elements holds for them as for every case)
        base = torch.randint(-3, 4, (C,), generator=g)
        o.x = torch.stack([base[torch.randperm(C, generator=g)] for _ in range(rows)]).to(T)
        o.res = torch.randint(-3, 4, (rows, C), generator=g).to(T)
        o.Wp, o.W2 = torch.eye(C).to(T), torch.zeros(C, HID, dtype=T)
        o.W1v = o.W1g = torch.zeros(HID, C, dtype=T)
        o.b1v = o.b1g = torch.zeros(HID)
        o.b_out = torch.zeros(C)
    else:
        # bf16: magnitudes over five binades; f16: over one, so that the normalised tokens stay away from zero - a LayerNorm output crosses zero, and towards zero the f16 grid
        # becomes finer than the f32 error of x - mean: a row would have more than XN_CAP of its elements beside a rounding boundary
        x = distinct_tokens(rows, C, T, s + 6, *((0.125, 4.0) if c.dt == "bf16" else (1.0, 2.0)))
        o.big_rows, o.const_rows = tuple(r for r in BIG_ROWS if r < rows), tuple(r for r in CONST_ROWS if r < rows)
        for r in o.big_rows:
            x[r] = (x[r].float() * 40 + 100).to(T)             # a row with a large mean
        for r in o.const_rows:
            # a constant whose f32 mean comes out exact (s * (1.0f / 320) rounds back to it): x - mean is then 0 in the kernel as in the reference
            cands = [v for v in (0.75, 1.0, 0.5, 1.25, 1.5, 2.0) if bool((ff_stats_sim(torch.full((1, C), v), LN_EPS)[2] == 0).all())]
            x[r] = cands[0]
        o.x = x
        o.res = rnd((rows, C), s + 8).to(T) if c.res != "none" else None
        o.Wp = (rnd((C, C), s + 1) * (C + HID) ** -0.5).to(T)
        o.W2 = (rnd((C, HID), s + 2) * (C + HID) ** -0.5 * 2).to(T)
        # FF1 rows with about 8 non-zero weights of size 0.35 / 0.25 (pre-activations of unit scale): (K + 8) 2^-24 sum |xn w| of a dense row is a quarter of a bf16 ulp of
        # the hidden value, and more than HID_CAP of a row's hidden elements would sit within that of a rounding boundary
        keep = torch.rand((2, HID, C), generator=torch.Generator().manual_seed(s + 3)) < 8.0 / C
        w1 = rnd((2, HID, C), s + 4) * torch.tensor([0.35, 0.25])[:, None, None] * keep
        b1 = rnd((2, HID), s + 5) * 0.2 + torch.linspace(-0.2, 0.2, HID)
        # gates mostly positive (1.5 +- 0.75): the gate carries |v g| PHI_ERR whatever Phi(g) is, and where Phi(g) is small that alone exceeds the spacing of v g Phi(g)
        b1[1] = b1[1] + 1.5
        if c.dt == "f16":
            # f16: (K + 8) 2^-24 sum |xn w| is of the size of the f16 spacing itself, so every hidden element with a value path is beside a boundary; ACTIVE_F16 units
            # of a chunk have one (another six in every chunk, so every register slot has one in some chunk), the others are exact zeros on both sides
            unit = torch.arange(HID)
            active = ((unit % 32 + 32 - (5 * (unit // 32)) % 32) % 32) < ACTIVE_F16
            w1[0] = w1[0] * active[:, None]
            b1[0] = b1[0] * active
        o.W1v, o.W1g = w1[0].to(T), w1[1].to(T)
        o.b1v, o.b1g = b1[0].float(), b1[1].float()
        o.b_out = (rnd((C,), s + 9) * 0.1).float()
    if c.res == "none":
        o.res = None
    # the GEGLU-packed FF1 of engine/weights.py::_ff: 16 value rows, their 16 gate rows, ...
    w1p = torch.stack([o.W1v.reshape(HID // 16, 16, C), o.W1g.reshape(HID // 16, 16, C)], dim=1).reshape(2 * HID, C).contiguous()
    b1p = torch.stack([o.b1v.reshape(HID // 16, 16), o.b1g.reshape(HID // 16, 16)], dim=1).reshape(2 * HID).contiguous()
    o.ff = Packed(w1=w1p, b1=b1p, cs1=w1p.float().sum(dim=1).contiguous(), po_w=torch.cat([o.Wp, o.W2], dim=1).contiguous(), po_b=o.b_out)
    o.ws = pack_ff_block(o.ff)
    o.buf, o.mask = guarded(rows, C, T)
    if c.res == "alias":
        window(o.buf, rows, C).copy_(o.res)
    if c.cs_rows:
        o.pwin = (rows // 128, 2 * C)
        o.pbuf, o.pmask = guarded(rows // 128, 2 * C, torch.float32)
    return o


def ff_reference(c, ops):
    T, emu, C, rows = DT[c.dt], EmuOps(acc=torch.float64), C_FF, c.rows
    out = torch.zeros(rows, C, dtype=T)
    emu.ff_block(ops.x, ops.res, out, wstream=ops.ws, b_out=ops.b_out, rows=rows, C_=C, hidden=HID, eps=LN_EPS)
    X = ops.x.double()
    mean = X.mean(-1, keepdim=True)
    rstd = (X.var(-1, unbiased=False, keepdim=True) + LN_EPS).rsqrt()
    xn = (X - mean) * rstd
    # the kernel's value before the rounding to T (ff_block.hip:187): (x - mu) * rs with mu and the variance v as ff_stats_sim has them (bit for bit), rs within 1 ulp of
    # 1 / sqrt(v) (rsqrtf: 2 u), one product (u)
    mu32, _, a32, v32 = ff_stats_sim(ops.x.float(), LN_EPS)
    e_xn = (a32.double() / v32.double().sqrt()[:, None] - xn).abs() + 3 * u * xn.abs()
    ch_xn = spread(xn, e_xn, T)
    xnT = round_T(xn, T)
    W1v, W1g, W2, Wp = ops.W1v.double(), ops.W1g.double(), ops.W2.double(), ops.Wp.double()
    v = xnT @ W1v.t() + ops.b1v.double()
    g = xnT @ W1g.t() + ops.b1g.double()
    # FF1 (ff_block.hip:222-223, bias :204): an f32 MFMA sum over K = 320 plus the bias, and the boundary charges of xn through |W1|
    dv = (C + 8) * u * (xnT.abs() @ W1v.abs().t() + ops.b1v.double().abs()) + ch_xn @ W1v.abs().t()
    dg = (C + 8) * u * (xnT.abs() @ W1g.abs().t() + ops.b1g.double().abs()) + ch_xn @ W1g.abs().t()
    gphi = g * Phi(g)
    h = v * gphi
    # geglu_one: Phi by the polynomial (PHI_ERR) evaluated in f32 - xc^2, seven fmaf, xc * r, one fmaf: 16 u of sum |c_i| xc^2i on r, times xc / 2, 3 u for the rest -,
    # then g * phi and h * that (u each, 3 u |h| with slack); the pre-activations' own errors through |g Phi(g)| and |v| DG
    e_phi = PHI_ERR + phi_rounding(g)
    e_h = dv * gphi.abs() + v.abs() * (DG * dg + g.abs() * e_phi) + DG * dv * dg + 3 * u * h.abs()
    ch_h = spread(h, e_h, T)
    hT = round_T(h, T)
    S_ = X.abs() @ Wp.abs().t() + hT.abs() @ W2.abs().t() + ops.b_out.double().abs()
    if ops.res is not None:
        S_ = S_ + ops.res.double().abs()
    ref = ops.buf.clone()
    window(ref, rows, C).copy_(out)
    # the last stage: one f32 chain over the projection (K = 320) and FF2 (K = 1280), bias and residual (ff_block.hip:173, :241, :331)
    bound = KC.ulp(out.double(), c.dt) + (C + HID + 8) * u * S_ + ch_h @ W2.abs().t()
    ops.info = NS(xn_share=(ch_xn > 0).double().mean(dim=1).max().item(), hid_share=(ch_h > 0).double().mean(dim=1).max().item(),
                  hid_share_mean=(ch_h > 0).double().mean().item())
    return ref, bound


def geglu32(h, g):
    """geglu_one in f32, operation by operation"""
    cl = torch.tensor(GEGLU_CLAMP, dtype=torch.float32)
    xc = torch.minimum(torch.maximum(g, -cl), cl)
    t = xc * xc
    r = torch.full_like(t, GEGLU_COEF[0])
    for cf in GEGLU_COEF[1:]:
        r = fma32(r, t, torch.tensor(cf, dtype=torch.float32))
    phi = fma32(xc * r, torch.tensor(0.5), torch.tensor(0.5))
    return h * (g * phi)


def ff_parts_model(y32):
    """ff_block.hip:339-378: thread (column group, row slice rsl) adds rows rsl, rsl + 6, ... of the stored tile, the six slices are added in order"""
    t = y32.reshape(-1, 128, y32.shape[1])
    S, Q = torch.zeros(t.shape[0], t.shape[2]), torch.zeros(t.shape[0], t.shape[2])
    part = []
    for rsl in range(6):
        cs, cq = torch.zeros_like(S), torch.zeros_like(S)
        for r in range(rsl, 128, 6):
            cs = cs + t[:, r]
            cq = fma32(t[:, r], t[:, r], cq)
        part.append((cs, cq))
    for cs, cq in part:
        S, Q = S + cs, Q + cq
    return torch.stack([S, Q], dim=-1)      # [tiles][C][2]


def ff_model(c, ops, defect=None):
    """-> (output buffer, chan_parts buffer or None)"""
    T, C, rows = DT[c.dt], C_FF, c.rows
    x32 = ops.x.float()
    mu, rs, a, _ = ff_stats_sim(x32, LN_EPS, ops.big_rows if defect == "mean0" else ())
    xnT = (a * rs[:, None]).to(T).float()
    Wp, W1v, W1g, W2 = ops.Wp.float(), ops.W1v.float(), ops.W1g.float(), ops.W2.float()
    src = xnT if defect == "proj_xn" else x32
    acc = torch.zeros(rows, C)
    for s in range(20):
        acc = acc + src[:, 16 * s:16 * s + 16] @ Wp[:, 16 * s:16 * s + 16].t()
    for ch in range(CHUNKS):
        if defect == "drop39" and ch == CHUNKS - 1:
            continue
        u0 = 32 * ch
        v, g = torch.zeros(rows, 32), torch.zeros(rows, 32)
        for s in range(20):
            xs = xnT[:, 16 * s:16 * s + 16]
            v = v + xs @ W1v[u0:u0 + 32, 16 * s:16 * s + 16].t()
            g = g + xs @ W1g[u0:u0 + 32, 16 * s:16 * s + 16].t()
        b0 = u0 - 32 if (defect == "bias_prev" and ch >= 1) else u0
        v, g = v + ops.b1v[b0:b0 + 32], g + ops.b1g[b0:b0 + 32]
        if defect == "swap_vg" and ch == SWAP_CHUNK:
            v, g = g, v
        h = geglu32(v, g).to(T).float()
        for sg in range(2):      # FF2 k-step sg carries the units 16 sg .. 16 sg + 15 of the chunk (engine/weights.py::ff_slot_unit)
            acc = acc + h[:, 16 * sg:16 * sg + 16] @ W2[:, u0 + 16 * sg:u0 + 16 * sg + 16].t()
    acc = acc + ops.b_out
    if ops.res is not None:
        acc = acc + ops.res.float()
    y = acc.to(T)
    buf = ops.buf.clone()
    window(buf, rows, C).copy_(y)
    pbuf = None
    if c.cs_rows:
        parts = ff_parts_model(y.float())
        pbuf = ops.pbuf.clone()
        pw = window(pbuf, *ops.pwin)
        pw.copy_(parts.reshape(rows // 128, 2 * C))
        if defect == "stats_slot":
            pw[0] = pw[1]
            pw[1] = window(ops.pbuf, *ops.pwin)[1]
    return buf, pbuf


def parts_reference(stored):
    """stored [rows][C] (any type): the f64 {sum, sum sq} per 128-row tile of the values as stored, [tiles][2 C] laid out as chan_parts (f64: compare() judges the kernel's f32
    entries against the f64 sums themselves), and the bound of the module docstring of kernel_compare: L 2^-24 sum |x| and (L + 1) 2^-24 sum x^2, nothing added"""
    t = stored.double().reshape(-1, 128, stored.shape[1])
    ref = torch.stack([t.sum(1), (t * t).sum(1)], dim=-1)
    mag = torch.stack([PARTS_L * u * t.abs().sum(1), (PARTS_L + 1) * u * (t * t).sum(1)], dim=-1)
    n = ref.shape[0]
    return ref.reshape(n, -1), mag.clamp_min(NC.TINY).reshape(n, -1), ref.reshape(n, -1)


def ff_defects(c):
    if c.recipe != "random":
        return ()
    return ("drop39", "bias_prev", "swap_vg", "proj_xn", "mean0") + (("stats_slot",) if c.cs_rows else ())


# =========================================================================================================================================
# fyc_temporal_block (csrc/temporal_block.hip: the LDS-tile kernel; csrc/temporal_block_rr.hip: the register-resident one, taken when the packed stream is passed)
# =========================================================================================================================================
TB_H, TB_D, TB_F, TB_C = 8, 40, 16, 320
TB_SCALE = TB_D ** -0.5
SHIFT_HEAD = 3


@dataclass(frozen=True)
class TBlock:
    name: str
    dt: str
    clips: int
    P: int                          # pixels
    rr: bool                        # the register-resident kernel (wstream) or the LDS-tile kernel
    pe: bool                        # with pe_bias
    defects: Tuple[str, ...] = ()
    op = "temporal_block"

    @property
    def rows(self):
        return self.clips * TB_F * self.P

    @property
    def cols(self):
        return TB_C

    @property
    def problem(self):
        return replace(self, name="", defects=())


def tb_stats_sim(x32, eps, rr):
    """the LayerNorm statistics of the two kernels in f32, operation by operation (see ff_stats_sim).  rr (temporal_block_rr.hip:109-129): lane (frame, quad g) adds its 80 tokens
    x[32 k + 8 g ..] pair by pair, the four lanes of a row meet as (0 + 1) + (2 + 3), * (1.0f / C), then the squares about that mean by fmaf -> (mu, v = var + eps, x - mu).
    LDS-tile (temporal_block.hip:70-84): four threads per row, 80 consecutive tokens each, s += x and q = fmaf(x, x, q); v = max(q / C - mu mu, 0) + eps -> (mu, v, None)."""
    rows = x32.shape[0]
    inv, e32 = torch.tensor(1.0 / TB_C, dtype=torch.float32), torch.tensor(eps, dtype=torch.float32)
    tree = lambda t: (t[:, 0] + t[:, 1]) + (t[:, 2] + t[:, 3])      # noqa: E731
    if rr:
        X = x32.reshape(rows, 10, 4, 4, 2)
        s = torch.zeros(rows, 4)
        for k in range(10):
            for e in range(4):
                s = s + (X[:, k, :, e, 0] + X[:, k, :, e, 1])
        mu = tree(s) * inv
        m, q = mu[:, None], torch.zeros(rows, 4)
        for k in range(10):
            for e in range(4):
                a, b = X[:, k, :, e, 0] - m, X[:, k, :, e, 1] - m
                q = fma32(a, a, q)
                q = fma32(b, b, q)
        return mu, tree(q) * inv + e32, x32 - m
    X = x32.reshape(rows, 4, 80)
    s, q = torch.zeros(rows, 4), torch.zeros(rows, 4)
    for j in range(80):
        s = s + X[:, :, j]
        q = fma32(X[:, :, j], X[:, :, j], q)
    mu = tree(s) * inv
    return mu, (tree(q) * inv - mu * mu).clamp_min(0.0) + e32, None


def tb_operands(c):
    from followyourclick_amd.engine.weights import Packed, pack_temporal_block
    T, s, C = DT[c.dt], _seed(c), TB_C
    gain = torch.cat([torch.full((2 * C,), 2.0), torch.ones(C)])[:, None]      # q and k of twice the unit scale: peaked attention rows, where a wrong weight shows
    o = NS(win=(c.rows, C))
    o.W = (rnd((3 * C, C), s + 1) * C ** -0.5 * gain).to(T)
    o.b = (rnd((3 * C,), s + 2) * 0.1).float()
    o.pe_w = (rnd((24, 3 * C), s + 3) * 0.5).float() if c.pe else None
    o.Wo = (rnd((C, C), s + 4) * C ** -0.5).to(T)
    o.bo = (rnd((C,), s + 5) * 0.1 + torch.linspace(-0.2, 0.2, C)).float()
    o.cs = o.W.float().sum(dim=1)
    o.kw = pack_temporal_block(Packed(qkv_f=(o.W, o.b, o.cs), pe_w=o.pe_w, o_w=o.Wo, o_b=o.bo), TB_H, TB_F)
    if not c.rr:
        del o.kw["wstream"]
    o.x = distinct_tokens(c.rows, C, T, s + 6, *((0.125, 4.0) if c.dt == "bf16" else (1.0, 2.0)))      # as for fyc_ff_block
    o.tab = o.b[None, :] + (o.pe_w[:TB_F] if c.pe else torch.zeros(TB_F, 3 * C))      # [F][3 C]: bias + positional term of the frame
    o.buf, o.mask = guarded(c.rows, C, T)
    return o


def _heads(t, c):
    """[clips][F][P][3 C] -> q, k, v as [clips][P][H][F][d]"""
    t = t.reshape(c.clips, TB_F, c.P, 3, TB_H, TB_D).permute(3, 0, 2, 4, 1, 5)
    return t[0], t[1], t[2]


def _unheads(o, c):
    """[clips][P][H][F][d] -> [rows][C]"""
    return o.permute(0, 3, 1, 2, 4).reshape(c.rows, TB_C)


def tb_reference(c, ops):
    T, emu, C = DT[c.dt], EmuOps(acc=torch.float64), TB_C
    out = torch.zeros(c.rows, C, dtype=T)
    emu.temporal_block(ops.x, out, **ops.kw, clips=c.clips, frames=TB_F, pixels=c.P, heads=TB_H, d=TB_D, scale=TB_SCALE, eps=LN_EPS)
    X, W = ops.x.double(), ops.W.double()
    tab = ops.tab.double()[None, :, None, :].expand(c.clips, TB_F, c.P, 3 * C).reshape(c.rows, 3 * C)
    mean = X.mean(-1, keepdim=True)
    rstd = (X.var(-1, unbiased=False, keepdim=True) + LN_EPS).rsqrt()
    mu32, v32, a32 = tb_stats_sim(ops.x.float(), LN_EPS, c.rr)
    rs_t = 1.0 / v32.double().sqrt()[:, None]
    xn_share = 0.0
    if c.rr:
        xn = (X - mean) * rstd
        e_xn = (a32.double() * rs_t - xn).abs() + 3 * u * xn.abs()
        ch_xn = spread(xn, e_xn, T)
        xn_share = (ch_xn > 0).double().mean(dim=1).max().item()
        xnT = round_T(xn, T)
        qkv = xnT @ W.t() + tab
        e_qkv = (C + 8) * u * (xnT.abs() @ W.abs().t() + tab.abs()) + ch_xn @ W.abs().t()
    else:
        A, cs = X @ W.t(), ops.cs.double()[None, :]
        qkv = rstd * (A - mean * cs) + tab
        core = rs_t * (A - mu32.double()[:, None] * cs)
        e_qkv = (core + tab - qkv).abs() + rs_t * ((C + 1) * u * (X.abs() @ W.abs().t()) + 2 * u * (mu32.double()[:, None] * cs).abs()) + 6 * u * (core.abs() + tab.abs() + qkv.abs())
    dqkv = spread(qkv, e_qkv, T)
    q, k, v = _heads(round_T(qkv, T), c)
    dq, dk, dv = _heads(dqkv, c)
    o, rest, w = KC.softmax_bound_terms(q, k, v, scale=TB_SCALE, dtype=c.dt, kind="temporal", dq=dq, dk=dk, dv=dv)
    # the reference's own attention output before its rounding (EmuOps.temporal_block): within r sum w |v| of o
    sc = (q @ k.transpose(-1, -2)) * TB_SCALE
    if c.rr:
        E = torch.exp(sc - sc.max(dim=-1, keepdim=True).values)
        o_ref = (round_T(E, T) @ v) / E.sum(dim=-1, keepdim=True)
    else:
        o_ref = round_T(sc.softmax(dim=-1), T) @ v
    e_o = rest + KC.R[c.dt] * (w @ v.abs())
    d_o = _unheads(spread(o_ref, e_o, T), c)
    oT = _unheads(round_T(o_ref, T), c)
    Wo = ops.Wo.double()
    S_ = X.abs() + oT.abs() @ Wo.abs().t() + ops.bo.double().abs()
    ref = ops.buf.clone()
    window(ref, c.rows, C).copy_(out)
    bound = KC.ulp(out.double(), c.dt) + (TB_H * 64 + 8) * u * S_ + d_o @ Wo.abs().t()
    ops.info = NS(xn_share=xn_share, qkv_share=(dqkv > 0).double().mean().item(), o_share=(d_o > 0).double().mean().item())
    return ref, bound


def tb_model(c, ops, defect=None):
    T, C = DT[c.dt], TB_C
    x32, W, Wo = ops.x.float(), ops.W.float(), ops.Wo.float()
    tab = ops.tab
    if defect == "pe_next":
        tab = torch.roll(tab, -1, dims=0)
    tab = tab[None, :, None, :].expand(c.clips, TB_F, c.P, 3 * C).reshape(c.rows, 3 * C)
    mu, v32, a = tb_stats_sim(x32, LN_EPS, c.rr)
    rs = (1.0 / v32.double().sqrt()).float()[:, None]
    acc = torch.zeros(c.rows, 3 * C)
    src = (a * rs).to(T).float() if c.rr else x32
    for s in range(C // 32):
        acc = acc + src[:, 32 * s:32 * s + 32] @ W[:, 32 * s:32 * s + 32].t()
    qkv = acc + tab if c.rr else rs * (acc - mu[:, None] * ops.cs[None, :]) + ops.b[None, :] + (tab - ops.b[None, :])
    q, k, v = _heads(qkv.to(T).float(), c)
    sl2e = torch.tensor(TB_SCALE * 1.44269504088896340736, dtype=torch.float32)
    st = q @ k.transpose(-1, -2)
    if c.rr:
        sv = st * sl2e
        e = torch.exp2(sv - sv.max(dim=-1, keepdim=True).values)
    else:
        e = torch.exp2((st - st.max(dim=-1, keepdim=True).values) * sl2e)
    if defect == "mask_last":
        e = e.clone()
        e[..., TB_F - 1] = 0.0
    inv = 1.0 / e.sum(dim=-1, keepdim=True)
    o = (e.to(T).float() @ v) * inv if c.rr else (e * inv).to(T).float() @ v
    o = o.to(T).float()
    if defect == "head_shift":
        o = o.clone()
        o[:, :, SHIFT_HEAD] = o[:, :, SHIFT_HEAD + 1]
    oT = _unheads(o, c)
    acc = torch.zeros(c.rows, C)
    for h in range(TB_H):
        acc = acc + oT[:, TB_D * h:TB_D * h + TB_D] @ Wo[:, TB_D * h:TB_D * h + TB_D].t()
    y = (acc + ops.bo + x32).to(T).reshape(c.clips, TB_F, c.P, C)
    if defect == "swap_tiles":
        y = torch.cat([y[:, :, 8:16], y[:, :, 0:8]], dim=2)
    if defect == "swap_clips":
        y = y.flip(0)
    buf = ops.buf.clone()
    window(buf, c.rows, C).copy_(y.reshape(c.rows, C))
    return buf


def tb_defects(c):
    return ("mask_last", "head_shift") + (("pe_next",) if c.pe else ()) + (("swap_tiles",) if c.P >= 16 else ()) + (("swap_clips",) if c.clips >= 2 else ())


def tb_labels(c):
    return KC.Labels(lambda i: f"clip {i // (TB_F * c.P)}, frame {i // c.P % TB_F}, pixel {i % c.P} (tile {i % c.P // 8})", lambda j: f"column block {j // 16}, lane column {j % 16}")


# =========================================================================================================================================
_OPS = {"panel_linear": (panel_operands, panel_reference, panel_model), "ff_block": (ff_operands, ff_reference, ff_model),
        "temporal_block": (tb_operands, tb_reference, tb_model)}


def operands(c):
    return _OPS[c.op][0](c)


def reference(c, ops):
    """-> (reference buffer, per-element bound [rows][cols] f64); the shares of boundary-charged elements are left in ops.info"""
    return _OPS[c.op][1](c, ops)


def model(c, ops, defect=None):
    return _OPS[c.op][2](c, ops, defect)


def rtol(c):
    return RTOL[c.op][c.dt]


# ---- the case lists -------------------------------------------------------------------------------------------------------------------------
def _panel_cases():
    out = []

    def add(c):
        out.append(replace(c, defects=panel_defects(c)))
    plain = [(320, 320, True, "sep"), (320, 640, True, "alias"), (640, 320, False, "none"), (640, 640, True, "sep")]
    gn_cs = [(320, 320, 256, 128, 1, 32, True, "none"), (320, 640, 512, 256, 2, 32, False, "sep"), (640, 320, 512, 128, 4, 8, True, "alias"),
             (640, 640, 512, 256, 4, 32, True, "sep"), (320, 320, 512, 256, 1, 8, False, "alias")]
    # parts: (K, N, rps, ss, bm): tiles of 192 rows over samples of 128 (general fold, 3 slots, NaN for the samples past the end), four 64-row tiles per sample (fast fold,
    # unrolled), two 128-row tiles per sample (fast fold, tail loop), two samples per 128-row tile (general fold, 2 slots)
    gn_parts = [(320, 640, 256, 2, 192), (640, 320, 256, 1, 64), (320, 320, 256, 1, 128), (640, 640, 128, 2, 128)]
    for dt in DT:
        for K, N, bias, res in plain:
            add(Panel(f"plain-{dt}-K{K}-N{N}-res_{res}{'' if bias else '-nobias'}", dt, 256, K, N, bias=bias, res=res))
        for K, N, rows, rps, ss, G, bias, res in gn_cs:
            add(Panel(f"cs-{dt}-K{K}-N{N}-rows{rows}-rps{rps}-ss{ss}-g{G}-res_{res}{'' if bias else '-nobias'}", dt, rows, K, N, gn="cs", rps=rps, ss=ss, groups=G, bias=bias, res=res))
        for K, N, rps, ss, bm in gn_parts:
            add(Panel(f"parts-{dt}-K{K}-N{N}-rps{rps}-ss{ss}-bm{bm}", dt, 512, K, N, gn="parts", rps=rps, ss=ss, bm=bm, res="sep"))
    return out


def _ff_cases():
    out = []
    for dt in DT:
        for rows, res, cs_rows in [(256, "sep", 128), (384, "alias", 0), (256, "none", 256), (384, "sep", 128)]:
            c = FF(f"ff-{dt}-rows{rows}-res_{res}-cs{cs_rows}", dt, rows, res=res, cs_rows=cs_rows)
            out.append(replace(c, defects=ff_defects(c)))
        out.append(FF(f"ff-{dt}-integer", dt, 256, res="sep", cs_rows=128, recipe="integer"))
    return out


def _tb_cases():
    out = []
    for dt in DT:
        for rr in (True, False):
            for pe in (True, False):
                for clips, P in ((2, 16), (1, 8)):      # four workgroups, two per clip; one workgroup
                    c = TBlock(f"tblock-{dt}-{'rr' if rr else 'lds'}-{'pe' if pe else 'nope'}-clips{clips}-P{P}", dt, clips, P, rr, pe)
                    out.append(replace(c, defects=tb_defects(c)))
    return out


PANEL_CASES = _panel_cases()
FF_CASES = _ff_cases()
TB_CASES = _tb_cases()
CASES = PANEL_CASES + FF_CASES + TB_CASES
assert len({c.name for c in CASES}) == len(CASES)


def case_ids(cases):
    return [c.name for c in cases]


@lru_cache(maxsize=2)
def problem(c):
    """operands, reference buffer and bound of a case: computed once, never modified (the latest two only: the cases of a test run in order)"""
    ops = operands(c)
    return (ops,) + tuple(reference(c, ops))
