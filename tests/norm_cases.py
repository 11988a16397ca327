"""The cases of the normalisation kernels (csrc/norm.hip, csrc/chan_parts.h) as data: what a case launches (traits(): the host-side launch choices of
norm.hip restated in Python), its operands inside guarded buffers, its plain f64 reference, its per-element bound (derivation: tests/kernel_compare.py)
and a torch model of the kernel's rounding points (f32 tensors combined in the kernel's order) with the defects the bound is there to catch.
A helper, not a test module: tests/test_norm_cases.py (CPU: coverage, model inside the bound, defects outside) and tests/test_norm_bounds_gpu.py use it.

Every output - the statistics buffers included - is a window [rows][cols] (row stride ld) of a flat prefilled buffer: 64 elements in front, two rows behind,
the pad columns [cols, ld) between the rows."""
from types import SimpleNamespace as NS

import torch

from kernel_compare import RTOL, ulp

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
DTS = ("bf16", "f16", "f32")
u = 2.0 ** -24
D53 = 2.0 ** -53
TINY = 2.0 ** -200      # the bound of an element that must be exact (any other value of any storage type is further away)
FRONT, BACK_ROWS = 64, 2
FILL = 7.25             # the prefill of every guarded buffer (exact in every type)
LOG2E_F = float(torch.tensor(1.4426950408889634, dtype=torch.float32))
RSQRT_U = 2.0           # rsqrtf: 1 ulp in the HIP math API's accuracy table = up to 2 u relative
EXP_U = 2.0             # expf (OCML) and the exp2 instruction behind __expf: 1 ulp documented = up to 2 u relative


def cdiv(a, b):
    return -(-a // b)


class Case(NS):
    def __hash__(self):
        return hash(self.name)

    def __eq__(self, other):
        return self.name == other.name


# ---- guarded buffers -------------------------------------------------------------------------------------------------------------------
def guarded(rows, cols, ld, T):
    n = FRONT + (rows + BACK_ROWS) * ld
    buf = torch.full((n,), FILL, dtype=T)
    mask = torch.zeros(n, dtype=torch.bool)
    mask[FRONT:FRONT + rows * ld].view(rows, ld)[:, :cols] = True
    return buf, mask


def window(buf, rows, cols, ld):
    return buf[FRONT:FRONT + rows * ld].view(rows, ld)[:, :cols]


def gauss(shape, seed, ms=0.0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) + ms) * scale


# ---- launch geometry (norm.hip, host side) ------------------------------------------------------------------------------------------------
def nthr_of(C8):
    return cdiv(C8, 64) * 64 if C8 >= 256 else 256


def stats_geometry(samples, rps):
    chunks = cdiv(1024, samples)
    rpb = max(cdiv(rps, chunks), 128)
    return cdiv(rps, rpb), rpb


def cs_geometry(samples, rps, rpi):
    chunks = cdiv(2048, samples)
    rpb = max(cdiv(rps, chunks), 8 * rpi)
    return cdiv(rps, rpb), rpb


def walk(block_rows, rpi):
    """the `r + 3 rpi < row_end` loop and its tail over blocks of these row counts: (unrolled loop runs, tail runs, most rows one thread walks)"""
    counts = [cdiv(n - r0, rpi) for n in block_rows for r0 in range(min(rpi, n))]
    return any(k >= 4 for k in counts), any(k % 4 for k in counts), max(counts)


def block_rows(rps, chunks, rpb):
    return [min(rpb, rps - k * rpb) for k in range(chunks)]


def slots_of(bm, cs_rows):
    """gemm_plan.h: sample slots of a row tile of bm rows when a statistics sample has cs_rows rows"""
    return 1 if cs_rows % bm == 0 else bm // cs_rows if bm % cs_rows == 0 else (bm - 1) // cs_rows + 2


def tile_range(bm, cs_rows, rows, o, group):
    row0 = o * group * cs_rows
    row1 = row0 + group * cs_rows
    return row0 // bm, min((row1 - 1) // bm, cdiv(rows, bm) - 1)


def fold_traits(bm, slots, cs_rows, rows, group):
    fast = slots == 1 and cs_rows % bm == 0
    t0, t1 = tile_range(bm, cs_rows, rows, 0, group)
    n = t1 - t0 + 1
    return dict(bm=bm, slots=slots, fast=fast, tiles=n, unroll_tiles=4 * (n // 4) if fast else 0, tail_tiles=n % 4 if fast else 0, partial_last_tile=rows % bm != 0)


def ln_maxch(C):
    need = cdiv(C // 8, 16)
    return need, next(m for m in (3, 5, 10, 16) if need <= m)


def traits(c):
    if c.op == "gn_stats":
        C8 = c.C // 8
        nthr = nthr_of(C8)
        rpi = nthr // C8
        chunks, rpb = stats_geometry(c.S, c.rps)
        br = block_rows(c.rps, chunks, rpb)
        un, tail, most = walk(br, rpi)
        return dict(C8=C8, nthr=nthr, nthr_rule="c8" if C8 >= 256 else "256", rpi=rpi, idle=nthr - rpi * C8, chunks=chunks, rpb=rpb, last_rows=br[-1], unroll=un, tail=tail,
                    walked=most, group_laps=cdiv(c.G, nthr), workspace=c.S * chunks * 2 * c.G * 4 if chunks > 1 else 0)
    if c.op == "gn_apply":
        chunks = c.S * c.rps * (c.C // 8)
        blocks = min(cdiv(chunks, 256), 8192)
        return dict(chunks=chunks, blocks=blocks, laps=cdiv(chunks, blocks * 256), straddle=(c.C // c.G) % 8 != 0)
    if c.op == "gn_apply_cs":
        C = c.C1 + c.C2
        C8, cpg = C // 8, C // c.G
        nthr = nthr_of(C8)
        rpi = nthr // C8
        chunks, rpb = cs_geometry(c.S, c.rps, rpi)
        un, tail, _ = walk(block_rows(c.rps, chunks, rpb), rpi)
        t = dict(nthr=nthr, rpi=rpi, chunks=chunks, rpb=rpb, unroll=un, tail=tail, source=[1 if k * 8 < c.C1 else 2 for k in range(C8)], straddle=c.C2 > 0 and c.C1 % cpg != 0,
                 stat_samples=c.ss, path=c.path)
        if c.path == "parts":
            t["fold"] = [fold_traits(bm, slots_of(bm, c.pcs), c.pcs, c.S * c.rps, c.rps // c.pcs) for bm in ((c.bm1, c.bm2) if c.C2 else (c.bm1,))]
        return t
    if c.op == "chan_stats_reduce":
        group = c.out_mult if c.out_mult else c.nsamp
        t0, t1 = tile_range(c.bm, c.cs_rows, c.nsamp * c.cs_rows, 0, group)
        return dict(slots=slots_of(c.bm, c.cs_rows), tiles=t1 - t0 + 1, group=group, partial_last_tile=(c.nsamp * c.cs_rows) % c.bm != 0)
    if c.op in ("layernorm", "row_stats"):
        need, maxch = ln_maxch(c.C)
        return dict(need=need, maxch=maxch, idle_lanes=max(0, 16 - c.C // 8), partial_block=c.rows % 16 != 0)
    if c.op == "softmax_rows":
        widths = [min(c.cols, r % c.causal + 1) if c.causal else c.cols for r in range(c.rows)]
        return dict(laps=cdiv(max(widths), 256), idle_waves=sum(1 for w in range(4) if w * 64 >= min(widths)), widths=widths)
    raise KeyError(c.op)


# ---- partial channel sums as a producer's epilogue lays them out ----------------------------------------------------------------------------
def build_parts(x, bm, cs_rows, slots):
    """x [rows][N] (any type) -> [tiles][slots][N][2] f32: the f64 sums over the rows of tile t that belong to sample (t bm) / cs_rows + sl, rounded to f32; 0 where the
    sample has no row in the tile, NaN where the sample does not exist (a correct consumer never reads it)"""
    xd = x.double()
    rows, N = xd.shape
    tiles, nsamp = cdiv(rows, bm), rows // cs_rows
    parts = torch.full((tiles, slots, N, 2), float("nan"), dtype=torch.float64)
    for t in range(tiles):
        for sl in range(slots):
            f = t * bm // cs_rows + sl
            if f >= nsamp:
                continue
            a, b = max(t * bm, f * cs_rows), min(min((t + 1) * bm, rows), (f + 1) * cs_rows)
            parts[t, sl] = torch.stack([xd[a:b].sum(0), (xd[a:b] ** 2).sum(0)], dim=-1) if a < b else 0.0
    return parts.float()


def fold(parts, bm, cs_rows, rows, o, group, defect=None):
    """{sum, sum sq} [N][2] f64 of output sample o (= `group` statistics samples) from the partials, tiles and slots ascending, and the sum of the absolute values of the terms
    and their number (for the 2^-53 charge).  f64 additions of f32 values in the kernel's order: reference and model at once.
    defects: "slot" (slot sl taken for sample first + sl + 1), "last_tile" (the clamp applied with rows / bm tiles: a partial last tile is lost)"""
    slots, nsamp = parts.shape[1], rows // cs_rows
    tiles_m = rows // bm if defect == "last_tile" else cdiv(rows, bm)
    row0 = o * group * cs_rows
    t0, t1 = row0 // bm, min((row0 + group * cs_rows - 1) // bm, tiles_m - 1)
    acc, mag, n = torch.zeros(parts.shape[2], 2, dtype=torch.float64), torch.zeros(parts.shape[2], 2, dtype=torch.float64), 0
    for t in range(t0, t1 + 1):
        for sl in range(slots):
            f = t * bm // cs_rows + sl + (1 if defect == "slot" else 0)
            if f < o * group or f >= (o + 1) * group or f >= nsamp:
                continue
            acc, mag, n = acc + parts[t, sl].double(), mag + parts[t, sl].double().abs(), n + 1
    return acc, mag, n


# =========================================================================================================================================
# GroupNorm statistics
# =========================================================================================================================================
def thread_sums(xb, rpi, drop_tail=False):
    """xb [S][nrows][C] f32, one block per sample: the per-thread {s, q} [S][rpi][C] of gn_stats_kernel (4 rows added as a tree while 4 are left, then one by one)"""
    S, nrows, C = xb.shape
    nit = cdiv(nrows, 4 * rpi)
    xp = torch.cat([xb, torch.zeros(S, nit * 4 * rpi - nrows, C)], dim=1).view(S, nit, 4, rpi, C)
    ok = (torch.arange(nit * 4 * rpi) < nrows).view(nit, 4, rpi, 1)
    s, q = torch.zeros(S, rpi, C), torch.zeros(S, rpi, C)
    for it in range(nit):
        v = xp[:, it]
        sq = v * v
        sf = s + ((v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3]))
        qf = q + ((sq[:, 0] + sq[:, 1]) + (sq[:, 2] + sq[:, 3]))
        ss, qs = s, q
        for j in range(0 if not drop_tail else 4, 3):
            ss, qs = torch.where(ok[it, j], ss + v[:, j], ss), torch.where(ok[it, j], qs + sq[:, j], qs)
        s, q = torch.where(ok[it, 3], sf, ss), torch.where(ok[it, 3], qf, qs)
    return s, q


def gn_stats_operands(c):
    g = torch.Generator().manual_seed(c.seed)
    shape = (c.S * c.rps, c.C)
    if c.kind == "int":
        x = torch.randint(-3, 4, shape, generator=g).float()
    elif c.kind == "one":
        x = torch.zeros(shape)
        x[-1, -1] = 1.5
    else:
        x = gauss(shape, c.seed, c.ms)
    buf, mask = guarded(c.S * c.G, 2, 2, torch.float64)
    return NS(x=x.to(DT[c.dt]), buf=buf, mask=mask, win=(c.S * c.G, 2, 2))


def gn_stats_sums(c, x):
    xd = x.double().view(c.S, c.rps, c.G, c.C // c.G)
    return (torch.stack([xd.sum((1, 3)), (xd * xd).sum((1, 3))], dim=-1).view(-1, 2),
            torch.stack([xd.abs().sum((1, 3)), (xd * xd).sum((1, 3))], dim=-1).view(-1, 2))


def gn_stats_chain(c):
    """L of the bound: the longest chain of f32 additions a term passes through, and the f64 chunk additions"""
    t = traits(c)
    return t["walked"] + t["rpi"] + c.C // c.G, t["chunks"]


def gn_stats_reference(c, ops):
    ref, mag = gn_stats_sums(c, ops.x)
    L, chunks = gn_stats_chain(c)
    bound = mag * torch.tensor([L * u, (L + (1 if c.dt == "f32" else 0)) * u]) + chunks * D53 * mag + TINY
    if c.kind == "int":       # every f32 partial is an integer below 2^24: exact
        bound = torch.full_like(bound, TINY)
    out = ops.buf.clone()
    window(out, *ops.win).copy_(ref)
    return out, bound


def gn_stats_model(c, ops, defect=None):
    t = traits(c)
    x = ops.x.float().view(c.S, c.rps, c.C)
    tot = torch.zeros(c.S, c.G, 2, dtype=torch.float64)
    nchunks = t["chunks"] - (1 if defect == "drop_last_chunk" else 0)
    for k in range(nchunks):
        s, q = thread_sums(x[:, k * t["rpb"]:min((k + 1) * t["rpb"], c.rps)], t["rpi"], drop_tail=defect == "drop_tail")
        cs, cq = torch.zeros(c.S, c.C), torch.zeros(c.S, c.C)
        for r0 in range(t["rpi"]):
            cs, cq = cs + s[:, r0], cq + q[:, r0]
        cs, cq = cs.view(c.S, c.G, -1), cq.view(c.S, c.G, -1)
        gs, gq = torch.zeros(c.S, c.G), torch.zeros(c.S, c.G)
        for i in range(c.C // c.G):
            gs, gq = gs + cs[:, :, i], gq + cq[:, :, i]
        tot = tot + torch.stack([gs, gq], dim=-1).double()
    return tot.view(-1, 2)


# =========================================================================================================================================
# the shared tail of the apply kernels: SiLU and the store
# =========================================================================================================================================
def silu_terms(o, Eo):
    """o f64 (the exact pre-activation), Eo its absolute error -> (silu(o), its absolute error before the store).  silu_f = o / (1 + __expf(-o)), __expf = exp2(-o log2e):
    the exponential E carries u |o| from the rounded product (u |o| log2e in log2 units, times ln 2), 0.25 u |o| from log2e as an f32 constant (its relative error is 1.3e-8 = 0.22 u)
    and the instruction's EXP_U u; then one addition and one division"""
    E = torch.exp(-o)
    sig = 1.0 / (1.0 + E)
    y = o * sig
    dy = (sig * (1.0 + o * (1.0 - sig))).abs()
    epsE = u * (1.25 * o.abs() + EXP_U)
    return y, dy * Eo + o.abs() * E * sig * sig * epsE + 2 * u * y.abs()


def silu_f32(o):
    return o / (1.0 + torch.exp2(-o * LOG2E_F))


def fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def norm_rho(var, dvar, eps):
    """relative error of rstd = rsqrtf((float)var + eps): var off by dvar, one rounding of the conversion, one of the addition, RSQRT_U u of the instruction"""
    t = var + eps
    return 0.5 * (dvar + u * var + u * t) / t + RSQRT_U * u, t


def eps32(c):
    return float(torch.tensor(c.eps, dtype=torch.float32))


# =========================================================================================================================================
# gn_apply
# =========================================================================================================================================
def gn_apply_operands(c):
    cpg = c.C // c.G
    x = gauss((c.S, c.rps, c.G, cpg), c.seed, c.ms)
    if c.const_group is not None:
        x[:, :, c.const_group, :] = 0.75
    x = x.view(c.S * c.rps, c.C).to(DT[c.dt])
    g = torch.Generator().manual_seed(c.seed + 1)
    gamma = (torch.rand(c.C, generator=g) * 8 - 4) if c.silu else gauss((c.C,), c.seed + 1) * 0.1 + 1
    beta = gauss((c.C,), c.seed + 2) * (0.5 if c.silu else 0.1)
    buf, mask = guarded(c.S * c.rps, c.C, c.C, DT[c.dt])
    sc = Case(op="gn_stats", name=c.name + "/stats", dt=c.dt, C=c.C, G=c.G, rps=c.rps, S=c.S, kind="gauss", ms=c.ms, seed=c.seed)
    return NS(x=x, gamma=gamma, beta=beta, buf=buf, mask=mask, win=(c.S * c.rps, c.C, c.C), stats_case=sc, stats=gn_stats_sums(sc, x)[0])


def gn_apply_reference(c, ops):
    cpg, n, eps = c.C // c.G, c.rps * (c.C // c.G), eps32(c)
    st, mag = gn_stats_sums(ops.stats_case, ops.x)
    m, qn = (st[:, 0] / n), st[:, 1] / n
    var = (qn - m * m).clamp_min(0.0)
    dm, dvar = u * m.abs(), 4 * D53 * (qn + m * m)
    if c.chained:       # the kernel's own statistics: their bound, through var = q / n - m^2
        L, chunks = gn_stats_chain(ops.stats_case)
        ds, dq = (L * u + chunks * D53) * mag[:, 0] / n, ((L + (1 if c.dt == "f32" else 0)) * u + chunks * D53) * mag[:, 1] / n
        dm, dvar = dm + ds, dvar + dq + 2 * m.abs() * ds
    if c.const_group is not None:      # n c and its quotient are exact, c is a number of T: mean_f = c, x - mean_f = 0
        dm = dm.view(c.S, c.G).clone()
        dm[:, c.const_group] = 0.0
        dm = dm.view(-1)
    rho, t = norm_rho(var, dvar, eps)
    e = lambda v: v.view(c.S, 1, c.G, 1)
    d = ops.x.double().view(c.S, c.rps, c.G, cpg) - e(m)
    rstd = e(t.rsqrt())
    gam, bet = ops.gamma.double().view(1, 1, c.G, cpg), ops.beta.double().view(1, 1, c.G, cpg)
    pg = d * rstd * gam
    o = pg + bet
    # four f32 roundings (x - mean, * rstd, * g, + b): the library is built with -ffp-contract=off (followyourclick_amd/_build.py), so * g + b is not fused
    Eo = gam.abs() * rstd * e(dm) + pg.abs() * (e(rho) + 3 * u) + u * o.abs()
    del d, pg
    if c.silu:
        o, Eo = silu_terms(o, Eo)
    out = ops.buf.clone()
    w = window(out, *ops.win)
    w.copy_(o.reshape(-1, c.C))
    return out, Eo.reshape(-1, c.C) + ulp(w.double(), c.dt) + TINY


def gn_apply_model(c, ops, stats=None, defect=None, contract=False):
    cpg, n = c.C // c.G, c.rps * (c.C // c.G)
    st = ops.stats if stats is None else stats
    m = st[:, 0] * (1.0 / n)
    var = (st[:, 1] * (1.0 / n) - m * m).clamp_min(0.0)
    mean = m.float().view(c.S, c.G)
    rstd = torch.rsqrt(var.float() + (0.0 if defect == "no_eps" else torch.tensor(c.eps, dtype=torch.float32))).view(c.S, c.G)
    if defect == "neighbour_mean":
        mean = mean.roll(1, dims=1)
    gamma = ops.gamma.roll(8) if defect == "gamma_chunk" else ops.gamma
    e = lambda v: v.view(c.S, 1, c.G, 1)
    p = (ops.x.float().view(c.S, c.rps, c.G, cpg) - e(mean)) * e(rstd)
    gam, bet = gamma.view(1, 1, c.G, cpg), ops.beta.view(1, 1, c.G, cpg)
    o = fma32(p, gam, bet) if contract else p * gam + bet
    if c.silu:
        o = silu_f32(o)
    return o.reshape(-1, c.C).to(DT[c.dt])


# =========================================================================================================================================
# gn_apply_cs (statistics per (statistics sample, channel): reduced f64 sums or the producer's row-tile partials) and chan_stats_reduce
# =========================================================================================================================================
def cs_operands(c):
    rows, T = c.S * c.rps, DT[c.dt]
    C = c.C1 + c.C2
    xs = [gauss((rows, c.C1), c.seed, c.ms).to(T)] + ([gauss((rows, c.C2), c.seed + 1, -0.5 * c.ms - 0.2, 1.5).to(T)] if c.C2 else [])
    g = torch.Generator().manual_seed(c.seed + 2)
    gamma = (torch.rand(C, generator=g) * 8 - 4) if c.silu else gauss((C,), c.seed + 2) * 0.1 + 1
    beta = gauss((C,), c.seed + 3) * (0.5 if c.silu else 0.1)
    buf, mask = guarded(rows, C, C, T)
    ops = NS(xs=xs, gamma=gamma, beta=beta, buf=buf, mask=mask, win=(rows, C, C), cs=[None, None], parts=[None, None], bms=[c.bm1, c.bm2] if c.path == "parts" else None)
    for i, x in enumerate(xs):
        if c.path == "cs":
            xd = x.double().view(c.S * c.ss, c.rps // c.ss, -1)
            ops.cs[i] = torch.stack([xd.sum(1), (xd * xd).sum(1)], dim=-1).contiguous()      # [S ss][Ci][2] f64, exact sums rounded once
        else:
            ops.parts[i] = build_parts(x, ops.bms[i], c.pcs, slots_of(ops.bms[i], c.pcs))
    return ops


def cs_channel_sums(c, ops, defect=None):
    """per (sample, channel of the concatenation) {s, q} [S][C][2] in f64 as the kernel's prologue reads them, the sum of the absolute values of the terms, and their number"""
    acc, mag, n = [], [], 0
    for i in range(len(ops.xs)):
        if c.path == "cs":
            v = ops.cs[i].view(c.S, c.ss, -1, 2)
            acc.append(v.sum(1)), mag.append(v.abs().sum(1))
            n = c.ss
        else:
            per = [fold(ops.parts[i], ops.bms[i], c.pcs, c.S * c.rps, o, c.rps // c.pcs, defect) for o in range(c.S)]
            acc.append(torch.stack([p[0] for p in per])), mag.append(torch.stack([p[1] for p in per]))
            n = max(n, max(p[2] for p in per))
    return torch.cat(acc, dim=1), torch.cat(mag, dim=1), n


def cs_group_stats(c, ops, defect=None):
    C = c.C1 + c.C2
    cpg = C // c.G
    acc, mag, nt = cs_channel_sums(c, ops, defect)
    n = c.rps * cpg
    gs, gm = acc.view(c.S, c.G, cpg, 2).sum(2), mag.view(c.S, c.G, cpg, 2).sum(2)
    return gs, gm, nt * cpg + 8, n


def cs_concat(c, ops, defect=None):
    if not c.C2:
        return ops.xs[0]
    x2 = ops.xs[1]
    if defect == "c1_chunk":      # the first chunk of x2 taken one chunk off
        x2 = torch.cat([x2[:, 8:16], x2[:, 8:]], dim=1)
    return torch.cat([ops.xs[0], x2], dim=1)


def cs_reference(c, ops):
    C, eps = c.C1 + c.C2, eps32(c)
    gs, gm, nterms, n = cs_group_stats(c, ops)
    m, qn = gs[..., 0] / n, gs[..., 1] / n
    var = (qn - m * m).clamp_min(0.0)
    dm = u * m.abs() + nterms * D53 * gm[..., 0] / n
    dvar = 4 * D53 * (qn + m * m) + nterms * D53 * gm[..., 1] / n + 2 * m.abs() * nterms * D53 * gm[..., 0] / n
    rho, t = norm_rho(var, dvar, eps)
    cpg = C // c.G
    e = lambda v: v.view(c.S, 1, c.G, 1)
    x = cs_concat(c, ops).double().view(c.S, c.rps, c.G, cpg)
    gam, bet = ops.gamma.double().view(1, 1, c.G, cpg), ops.beta.double().view(1, 1, c.G, cpg)
    sc = e(t.rsqrt()) * gam
    msc = e(m) * sc
    sf = bet - msc
    o = x * sc + sf
    # sc = rstd g (rho, one rounding); mean sc (dm, the error of sc, one rounding: the u |mean sc| term); sf = beta - mean sc (one rounding); one fused multiply-add
    Eo = x.abs() * sc.abs() * (e(rho) + u) + e(dm) * sc.abs() + msc.abs() * (e(rho) + u) + u * msc.abs() + u * sf.abs() + u * o.abs()
    if c.silu:
        o, Eo = silu_terms(o, Eo)
    out = ops.buf.clone()
    w = window(out, *ops.win)
    w.copy_(o.reshape(-1, C))
    return out, Eo.reshape(-1, C) + ulp(w.double(), c.dt) + TINY


def cs_model(c, ops, defect=None, contract=False):
    C = c.C1 + c.C2
    cpg = C // c.G
    gs, _, _, n = cs_group_stats(c, ops, defect)
    m = gs[..., 0] * (1.0 / n)
    var = (gs[..., 1] * (1.0 / n) - m * m).clamp_min(0.0)
    e = lambda v: v.view(c.S, 1, c.G, 1)
    mean, rstd = e(m.float()), e(torch.rsqrt(var.float() + torch.tensor(c.eps, dtype=torch.float32)))
    gam, bet = ops.gamma.view(1, 1, c.G, cpg), ops.beta.view(1, 1, c.G, cpg)
    sc = rstd * gam
    sf = fma32(-mean, sc, bet) if contract else bet - mean * sc
    o = fma32(cs_concat(c, ops, defect).float().view(c.S, c.rps, c.G, cpg), sc, sf)
    if c.silu:
        o = silu_f32(o)
    return o.reshape(-1, C).to(DT[c.dt])


def reduce_operands(c):
    g = torch.Generator().manual_seed(c.seed)
    rows = c.nsamp * c.cs_rows
    x = torch.randint(-3, 4, (rows, c.N), generator=g).float()      # integer-valued: every partial and every sum is exact
    group = traits(c)["group"]
    nout = c.nsamp // group
    buf, mask = guarded(nout * c.N, 2, 2, torch.float64)
    return NS(parts=build_parts(x, c.bm, c.cs_rows, slots_of(c.bm, c.cs_rows)), buf=buf, mask=mask, win=(nout * c.N, 2, 2), rows=rows, group=group, nout=nout, x=x)


def reduce_model(c, ops, defect=None):
    return torch.cat([fold(ops.parts, c.bm, c.cs_rows, ops.rows, o, ops.group, defect)[0] for o in range(ops.nout)])


def reduce_reference(c, ops):
    xd = ops.x.double().view(ops.nout, ops.group * c.cs_rows, c.N)      # straight from the rows, not from the partials
    out = ops.buf.clone()
    window(out, *ops.win).copy_(torch.stack([xd.sum(1), (xd * xd).sum(1)], dim=-1).view(-1, 2))
    return out, torch.full((ops.nout * c.N, 2), TINY, dtype=torch.float64)


# =========================================================================================================================================
# LayerNorm / row_stats: 16 lanes per row, two passes
# =========================================================================================================================================
def ln_operands(c):
    x = gauss((c.rows, c.C), c.seed, c.ms)
    if c.const_row is not None:
        x[c.const_row] = 1.5      # every partial sum k 1.5 is exact in f32, and so is its quotient
    x = x.to(DT[c.dt])
    gamma, beta = gauss((c.C,), c.seed + 1) * 0.1 + 1, gauss((c.C,), c.seed + 2) * 0.1
    pe = gauss((c.pe[1], c.C), c.seed + 3) if c.pe else None
    if c.op == "row_stats":
        buf, mask = guarded(c.rows, 2, 2, torch.float32)
        win = (c.rows, 2, 2)
    else:
        buf, mask = guarded(c.rows, c.C, c.C, DT[c.dt])
        win = (c.rows, c.C, c.C)
    return NS(x=x, gamma=gamma, beta=beta, pe=pe, buf=buf, mask=mask, win=win)


def ln_pe_rows(c, defect=None):
    r = torch.arange(c.rows)
    return (r % c.pe[1]) // c.pe[0] if defect == "pe_index" else (r // c.pe[0]) % c.pe[1]


def ln_reference(c, ops):
    eps, C = eps32(c), c.C
    need, _ = ln_maxch(C)
    xd = ops.x.double()
    m = xd.mean(1, keepdim=True)
    d = xd - m
    var = (d * d).mean(1, keepdim=True)
    L = 8 * need + 4      # a lane's chain of additions, then 4 shuffles
    dm = L * u * xd.abs().sum(1, keepdim=True) / C + u * m.abs()      # the sum, then the division by C
    # q = sum of fl(fl(x - mean_f)^2): the common shift dm adds C dm^2 (sum (x - m) = 0), each difference and each square one rounding, the sum its chain
    dd = (d.abs() + dm) ** 2
    dvar = dm * dm + (L + 3) * u * dd.sum(1, keepdim=True) / C + u * var      # + the division by C
    rho, t = norm_rho(var, dvar, eps)
    rho = rho - 0.5 * u * var / t      # (no conversion from f64 here: q / C is f32 already)
    rstd = t.rsqrt()
    out = ops.buf.clone()
    w = window(out, *ops.win)
    if c.op == "row_stats":
        w.copy_(torch.cat([m, rstd], dim=1))
        return out, torch.cat([dm, rstd * rho], dim=1) + ulp(w.double(), "f32") + TINY
    gam, bet = ops.gamma.double(), ops.beta.double()
    pg = d * rstd * gam
    o = pg + bet
    Eo = gam.abs() * rstd * dm + pg.abs() * (rho + 3 * u) + u * o.abs()
    if c.pe:
        o = o + ops.pe.double()[ln_pe_rows(c)]
        Eo = Eo + u * o.abs()
    if c.const_row is not None:      # mean_f = 1.5 exactly, x - mean_f = 0, q = 0: beta (+ pe, one rounding that the reference makes too)
        Eo[c.const_row] = 0.0
    w.copy_(o)
    return out, Eo + ulp(w.double(), c.dt) + TINY


def ln_model(c, ops, defect=None, contract=False):
    C, C8 = c.C, c.C // 8
    need, maxch = ln_maxch(C)
    live = need - (1 if defect == "drop_chunk" and need == maxch else 0)      # chunk k = MAXCH - 1 neither loaded nor stored
    xf = torch.cat([ops.x.float().view(c.rows, C8, 8), torch.zeros(c.rows, need * 16 - C8, 8)], dim=1).view(c.rows, need, 16, 8)
    ok = (torch.arange(need * 16) < C8).view(1, need, 16, 1) & (torch.arange(need) < live).view(1, need, 1, 1)
    lanes = torch.arange(16)

    def lane_sum(v):
        s = torch.zeros(c.rows, 16)
        for k in range(need):
            for i in range(8):
                s = s + v[:, k, :, i]
        for o in (8, 4, 2, 1):
            s = s + s[:, lanes ^ o]
        return s[:, :1]
    mean = lane_sum(torch.where(ok, xf, torch.zeros(()))) / float(C)
    d = torch.where(ok, xf - mean.view(-1, 1, 1, 1), torch.zeros(()))
    rstd = torch.rsqrt(lane_sum(d * d) / float(C) + torch.tensor(c.eps, dtype=torch.float32))
    if c.op == "row_stats":
        return torch.cat([mean, rstd], dim=1)
    p = (ops.x.float() - mean) * rstd
    o = fma32(p, ops.gamma, ops.beta) if contract else p * ops.gamma + ops.beta
    if c.pe:
        o = o + ops.pe[ln_pe_rows(c, defect)]
    y = o.to(DT[c.dt])
    if live < need:
        dead = ((torch.arange(C8) // 16) >= live).repeat_interleave(8)
        y[:, dead] = FILL
    return y


# =========================================================================================================================================
# row softmax in place
# =========================================================================================================================================
def softmax_operands(c):
    x = gauss((c.rows, c.cols), c.seed, 0.0, 4.0)
    if c.kind == "offset+":
        x = x + 80
    elif c.kind == "offset-":
        x = x - 80
    elif c.kind == "spike":
        x[:, max(c.cols - 3, 256)] += 30      # in a lap past the first, also where cols = 257
    elif c.kind == "equal":
        x[:] = -2.5
    buf, mask = guarded(c.rows, c.cols, c.ld, DT[c.dt])
    window(buf, c.rows, c.cols, c.ld).copy_(x)
    return NS(buf=buf, mask=mask, win=(c.rows, c.cols, c.ld))


def softmax_reference(c, ops):
    t = traits(c)
    x = window(ops.buf, *ops.win).double()
    live = torch.arange(c.cols).view(1, -1) < torch.tensor(t["widths"]).view(-1, 1)
    xm = torch.where(live, x, torch.full((), -float("inf"), dtype=torch.float64))
    z = xm - xm.max(1, keepdim=True).values
    p = torch.softmax(xm, dim=1)
    # x - max: one rounding (the maximum itself is exact); expf: EXP_U u; the sum: laps + 6 shuffles + 3 additions; the reciprocal and the product: one each
    eta = torch.where(live, u * z.abs() + EXP_U * u, torch.zeros((), dtype=torch.float64))
    rel = eta + (p * eta).sum(1, keepdim=True) + (t["laps"] + 6 + 3 + 2) * u
    out = ops.buf.clone()
    w = window(out, *ops.win)
    w.copy_(p)
    return out, torch.where(live, p * rel + ulp(w.double(), c.dt), torch.zeros((), dtype=torch.float64)) + TINY


def softmax_model(c, ops, defect=None):
    widths = traits(c)["widths"]
    src = window(ops.buf, *ops.win)
    out = src.clone()
    for r in range(c.rows):
        w = widths[r]
        if defect == "causal_width" and c.causal:
            w = max(1, min(c.cols, r % c.causal))
        seen = min(w, 256) if defect == "skip_laps" else w
        x = src[r, :seen].float()
        e = torch.exp(x - x.max())
        ep = torch.cat([e, torch.zeros(cdiv(seen, 256) * 256 - seen)]).view(-1, 256)
        s = torch.zeros(256)
        for lap in range(ep.shape[0]):
            s = s + ep[lap]
        s = s.view(4, 64)
        lanes = torch.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ o]
        inv = 1.0 / (((s[0, 0] + s[1, 0]) + s[2, 0]) + s[3, 0])
        out[r, :seen] = (e * inv).to(out.dtype)
        out[r, w:] = 0
    return out


# =========================================================================================================================================
# dispatch
# =========================================================================================================================================
_OPS = {"gn_stats": (gn_stats_operands, gn_stats_reference, gn_stats_model), "gn_apply": (gn_apply_operands, gn_apply_reference, gn_apply_model),
        "gn_apply_cs": (cs_operands, cs_reference, cs_model), "chan_stats_reduce": (reduce_operands, reduce_reference, reduce_model),
        "layernorm": (ln_operands, ln_reference, ln_model), "row_stats": (ln_operands, ln_reference, ln_model), "softmax_rows": (softmax_operands, softmax_reference, softmax_model)}


def operands(c):
    return _OPS[c.op][0](c)


def reference(c, ops):
    """(the guarded buffer with the f64 reference stored in its window, the per-element bound [rows][cols] f64)"""
    return _OPS[c.op][1](c, ops)


def model(c, ops, **kw):
    return _OPS[c.op][2](c, ops, **kw)


def rtol(c):
    """the global tolerance of the op's existing test on the well-conditioned cases; the ill-conditioned ones (mean / std > 0.35) are judged by finiteness, bound and guards alone"""
    if getattr(c, "ms", 0.0) > 0.35:
        return float("inf")
    return 1e-5 if c.op in ("gn_stats", "chan_stats_reduce", "row_stats") else RTOL[c.dt]


def labels(c):
    from kernel_compare import Labels
    if c.op in ("gn_stats",):
        return Labels(lambda i: f"sample {i // c.G}, group {i % c.G}", lambda j: ("sum", "sum sq")[j])
    if c.op == "chan_stats_reduce":
        return Labels(lambda i: f"output sample {i // c.N}, channel {i % c.N}", lambda j: ("sum", "sum sq")[j])
    if c.op == "row_stats":
        return Labels(lambda i: f"row {i}", lambda j: ("mean", "rstd")[j])
    if c.op == "softmax_rows":
        return Labels(lambda i: f"row {i}", lambda j: f"column {j}, lap {j // 256}")
    rps = getattr(c, "rps", None)
    return Labels((lambda i: f"sample {i // rps}, row {i % rps}") if rps else (lambda i: f"row {i}, block {i // 16}"), lambda j: f"channel {j}, 8-chunk {j // 8}")


# =========================================================================================================================================
# the cases
# =========================================================================================================================================
def _mk(op, dt, name, **kw):
    return Case(op=op, dt=dt, name=f"{op}-{dt}-{name}", seed=sum(map(ord, name)) % 9973 + 11, **kw)


def _gn_stats_cases():
    shapes = [  # C, groups, rows per sample, samples
        (8, 1, 7 * 256 + 3, 1), (8, 8, 300, 2), (64, 8, 4 * 32 + 1, 2), (320, 32, 4 * 6 + 1, 2), (320, 320, 7 * 6 + 3, 2), (960, 32, 389, 2), (1920, 32, 37, 2), (2040, 255, 9, 2),
        (2048, 512, 5, 2), (2048, 32, 4, 1), (2056, 257, 6, 2), (2560, 32, 7, 1), (2560, 2560, 4, 3), (4096, 32, 130, 1), (4096, 1, 5, 2), (4096, 512, 1, 1), (64, 32, 3, 1025)]
    shapes += [(64, 32, r, 3) for r in (1, 31, 32, 127, 128, 129, 227)]      # rpi = 32: around the unroll
    shapes += [(320, 32, 129, 2), (320, 32, 389, 2)]      # chunks > 1, a last chunk of 1 and of 5 rows
    out = []
    for dt in DTS:
        out += [_mk("gn_stats", dt, f"C{C}-g{G}-r{r}-s{S}-int", C=C, G=G, rps=r, S=S, kind="int", ms=0.0) for C, G, r, S in shapes]
        for C, G, r, S in ((320, 32, 389, 2), (64, 32, 227, 3), (1920, 32, 37, 2)):
            out += [_mk("gn_stats", dt, f"C{C}-g{G}-r{r}-s{S}-ms{ms:g}", C=C, G=G, rps=r, S=S, kind="gauss", ms=ms) for ms in (0.0, 0.35, 8.0, 64.0)]
        out += [_mk("gn_stats", dt, f"C{C}-g{G}-r{r}-s{S}-one", C=C, G=G, rps=r, S=S, kind="one", ms=0.0) for C, G, r, S in ((320, 32, 389, 2), (64, 32, 129, 3), (2056, 257, 6, 2))]
    return out


def _gn_apply_cases():
    out = []
    for dt in DTS:
        for i, (cpg, G) in enumerate(((1, 32), (2, 32), (4, 32), (8, 32), (10, 32), (30, 32), (60, 32), (128, 4))):
            for silu in (False, True):
                eps = (1e-5, 1e-6)[(i + silu) % 2]
                out.append(_mk("gn_apply", dt, f"cpg{cpg}-g{G}-silu{int(silu)}-eps{eps:g}", C=cpg * G, G=G, rps=5, S=2, silu=silu, eps=eps, ms=0.35, const_group=None, chained=False))
        for silu in (False, True):
            out.append(_mk("gn_apply", dt, f"cpg10-g32-silu{int(silu)}-const", C=320, G=32, rps=7, S=2, silu=silu, eps=1e-5, ms=0.35, const_group=3, chained=False))
        for ms in (8.0, 64.0):
            out.append(_mk("gn_apply", dt, f"cpg10-g32-silu1-ms{ms:g}", C=320, G=32, rps=9, S=2, silu=True, eps=1e-5, ms=ms, const_group=None, chained=False))
        out.append(_mk("gn_apply", dt, "cpg10-g32-silu1-chained", C=320, G=32, rps=389, S=2, silu=True, eps=1e-5, ms=0.35, const_group=None, chained=True))
        for ms in (8.0, 64.0):      # what the f32 partial sums of the statistics pass cost: the GroupNorm the engine runs, statistics then apply
            out.append(_mk("gn_apply", dt, f"cpg10-g32-silu0-chained-ms{ms:g}", C=320, G=32, rps=389, S=2, silu=False, eps=1e-5, ms=ms, const_group=None, chained=True))
    out.append(_mk("gn_apply", "bf16", "cpg64-g32-silu1-second-lap", C=2048, G=32, rps=8200, S=1, silu=True, eps=1e-5, ms=0.35, const_group=None, chained=False))
    return out


PARTS_CS_ROWS = (16, 48, 64, 80, 144, 192, 576, 1024)
BMS = (128, 256)      # every tile height gemm_plan.h::gemm_tile_bm can report


def _cs_cases():
    out = []
    cs = [  # C1, C2, groups, rows per sample, samples, statistics samples per norm sample, silu, mean / std
        (320, 0, 32, 25, 2, 5, False, 0.35), (320, 0, 32, 6, 3, 1, True, 0.35), (320, 0, 32, 48, 1, 1, True, 8.0), (8, 56, 32, 256, 2, 16, True, 0.35), (8, 56, 32, 32, 2, 1, False, 64.0),
        (40, 24, 8, 256, 1, 64, False, 0.35), (40, 24, 8, 127, 2, 1, True, 0.35), (40, 24, 8, 129, 2, 1, False, 8.0), (1280, 640, 32, 8, 2, 2, True, 0.35), (1280, 640, 32, 3, 2, 1, False, 64.0),
        (1280, 1280, 32, 5, 2, 1, True, 0.35), (1280, 1280, 32, 1, 2, 1, False, 0.35), (2048, 2048, 32, 4, 2, 2, False, 0.35), (2048, 2048, 32, 9, 1, 1, True, 8.0)]
    # rows per sample = k parts_cs_rows; (bm of source 1, of source 2); every (bm, cs_rows) whose slot rule gives 1 .. 4 slots appears as one of the two
    parts = [(48, 96, 3, 128, 128), (64, 64, 5, 128, 256), (80, 80, 13, 128, 128), (144, 288, 2, 128, 256), (192, 192, 3, 256, 128), (576, 576, 2, 128, 256), (1024, 1024, 2, 128, 256)]
    parts += [(128, 128 * k, 2, 128, 256) for k in (1, 3, 4, 5, 8)]      # source 1 on the fast path with k tiles per norm sample; source 2: two samples per 256-row tile
    for dt in DTS:
        for C1, C2, G, rps, S, ss, silu, ms in cs:
            out.append(_mk("gn_apply_cs", dt, f"cs-{C1}+{C2}-g{G}-r{rps}-s{S}-ss{ss}-silu{int(silu)}-ms{ms:g}", C1=C1, C2=C2, G=G, rps=rps, S=S, ss=ss, silu=silu, eps=1e-5, ms=ms, path="cs",
                           pcs=0, bm1=0, bm2=0))
        for i, (pcs, rps, S, bm1, bm2) in enumerate(parts):
            C1, C2, G = ((40, 24, 8), (8, 56, 32))[i % 2]
            out.append(_mk("gn_apply_cs", dt, f"parts-{C1}+{C2}-pcs{pcs}-r{rps}-s{S}-bm{bm1}+{bm2}", C1=C1, C2=C2, G=G, rps=rps, S=S, ss=rps // pcs, silu=bool(i % 2), eps=1e-5,
                           ms=(0.35, 0.35, 8.0)[i % 3], path="parts", pcs=pcs, bm1=bm1, bm2=bm2))
    return out


def _reduce_cases():
    out = []
    for i, k in enumerate((1, 7, 8, 9, 17)):      # k tiles per output sample: the 8-lane stride of the tile loop
        out.append(_mk("chan_stats_reduce", "f32", f"N{(8, 32, 40, 320)[i % 4]}-bm128-cs{128 * k}-n2-out1", N=(8, 32, 40, 320)[i % 4], bm=128, cs_rows=128 * k, nsamp=2, out_mult=1))
    for N, bm, cs_rows, nsamp, mult in ((320, 128, 48, 6, 2), (8, 128, 80, 13, 0), (40, 256, 64, 5, 1), (32, 256, 144, 4, 2), (40, 128, 192, 3, 0), (8, 256, 576, 2, 1), (32, 128, 64, 6, 2),
                                        (40, 256, 192, 4, 2), (8, 128, 1024, 2, 0), (32, 128, 144, 2, 1)):
        out.append(_mk("chan_stats_reduce", "f32", f"N{N}-bm{bm}-cs{cs_rows}-n{nsamp}-out{mult or 'all'}", N=N, bm=bm, cs_rows=cs_rows, nsamp=nsamp, out_mult=mult))
    return out


LN_C = (8, 64, 120, 128, 136, 320, 384, 392, 640, 648, 768, 1024, 1280, 1288, 2048)
LN_ROWS = (1, 15, 16, 17, 33)


def _ln_cases(op):
    out = []
    for dt in DTS:
        for i, C in enumerate(LN_C):
            rows = LN_ROWS[i % 5]
            pe = (None, (1, 1), (3, 5), (16, 2), (rows + 1, 4))[(i + i // 5) % 5] if op == "layernorm" else None
            out.append(_mk(op, dt, f"C{C}-r{rows}-pe{'x'.join(map(str, pe)) if pe else 'none'}-ms0.33", C=C, rows=rows, pe=pe, eps=1e-5, ms=0.33, const_row=None))
        for C, rows, ms in ((320, 17, 0.0), (2048, 15, 0.0), (320, 33, 32.0), (1288, 17, 32.0), (2048, 16, 32.0)):
            out.append(_mk(op, dt, f"C{C}-r{rows}-penone-ms{ms:g}", C=C, rows=rows, pe=None, eps=1e-5, ms=ms, const_row=None))
        out.append(_mk(op, dt, "C648-r17-const-row", C=648, rows=17, pe=(3, 5) if op == "layernorm" else None, eps=1e-5, ms=0.33, const_row=16))
    return out


def _softmax_cases():
    out = []
    kinds = ("gauss", "offset+", "offset-", "equal")
    for dt in DTS:
        for i, cols in enumerate((1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 4096)):
            rows, ld = (1, 3)[i % 2], cols + 8 * ((i // 2) % 2)
            out.append(_mk("softmax_rows", dt, f"c{cols}-ld{ld}-r{rows}-{kinds[i % 4]}", cols=cols, ld=ld, rows=rows, causal=0, kind=kinds[i % 4]))
        for cols, ld in ((257, 265), (513, 513), (4096, 4104)):
            out.append(_mk("softmax_rows", dt, f"c{cols}-ld{ld}-r3-spike", cols=cols, ld=ld, rows=3, causal=0, kind="spike"))
        for cols, rows, causal in ((5, 10, 5), (300, 600, 300), (7, 6, 3)):      # heads n rows with causal_rows = n (two heads); causal_rows < cols
            out.append(_mk("softmax_rows", dt, f"c{cols}-ld{cols + 8}-r{rows}-causal{causal}", cols=cols, ld=cols + 8, rows=rows, causal=causal, kind="gauss"))
    return out


CASES = _gn_stats_cases() + _gn_apply_cases() + _cs_cases() + _reduce_cases() + _ln_cases("layernorm") + _ln_cases("row_stats") + _softmax_cases()
assert len({c.name for c in CASES}) == len(CASES)


def by_op(op):
    return [c for c in CASES if c.op == op]


def case_ids(cases):
    return [c.name for c in cases]
