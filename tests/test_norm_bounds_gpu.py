"""fyc_gn_stats, fyc_gn_apply, fyc_gn_apply_cs, fyc_chan_stats_reduce, fyc_layernorm, fyc_row_stats and fyc_softmax_rows on the cases of tests/norm_cases.py (what each case
launches and that the list reaches every instantiation and host-side branch is proven on the CPU by tests/test_norm_cases.py).  Every case is one launch into an output - the
statistics buffers included - that lies inside a larger, prefilled buffer (64 elements in front, two rows behind, the pad columns of the softmax between the rows), compared with
the plain f64 reference by kernel_compare.compare: finite, EVERY element within the bound derived from the kernel's rounding points (tests/kernel_compare.py), nothing outside the
output touched; the global relative L2 at the tolerance of the existing test of the same op (RTOL[dt], 1e-5 for statistics) on the cases with mean / std <= 0.35, recorded only on
the ill-conditioned ones.  Integer-valued statistics inputs must give the f64 sums bit for bit.

FYC_NORM_FIGURES=<file>: append the figures of every comparison to that file (profiles/norm_bound_coverage.txt was made from it)."""
import ctypes
import os

import pytest
import torch

import norm_cases as N
from kernel_compare import Guard, compare, ulp
from test_kernels_gpu import hip  # noqa: F401  (the module-scoped library fixture)

pytestmark = pytest.mark.gpu

FIGURES = os.environ.get("FYC_NORM_FIGURES")
_cache = {}


def problem(c):
    """operands, reference buffer and bound of a case: computed once, never modified (the latest only: the cases of a test run in order)"""
    if c.name not in _cache:
        _cache.clear()
        ops = N.operands(c)
        _cache[c.name] = (ops,) + tuple(N.reference(c, ops))
    return _cache[c.name]


def flat(buf, ops):
    """the output as the kernel sees it: the buffer from the first element of the window on"""
    rows, _, ld = ops.win
    return buf[N.FRONT:N.FRONT + rows * ld]


def judge(c, ops, ref, bound, got, note=""):
    fig = compare(N.window(got, *ops.win), N.window(ref, *ops.win), dtype=c.dt, bound=bound, rtol=N.rtol(c), labels=N.labels(c), guard=Guard(ops.buf, got, ops.mask), tag=c.name)
    print(f"{c.name}: global rel-L2 {fig['global_rel']:.3e} (tolerance {N.rtol(c):.1e}), worst element at {fig['elem_ratio']:.3f} of its bound{note}")
    if FIGURES:
        with open(FIGURES, "a") as f:
            f.write(f"{c.op} {c.dt} {c.name} ms={getattr(c, 'ms', 0.0):g} {fig['global_rel']:.3e} {fig['elem_ratio']:.4f}{note}\n")
    return fig


def launch_gn_stats(hip, c, ops):  # noqa: F811
    buf = ops.buf.cuda()
    hip.gn_stats(ops.x.cuda(), flat(buf, ops), rows=c.S * c.rps, C_=c.C, groups=c.G, rows_per_sample=c.rps)
    torch.cuda.synchronize()
    return buf.cpu()


GN_STATS, GN_APPLY, GN_APPLY_CS, REDUCE, LAYERNORM, ROW_STATS, SOFTMAX = (N.by_op(op) for op in ("gn_stats", "gn_apply", "gn_apply_cs", "chan_stats_reduce", "layernorm", "row_stats",
                                                                                                   "softmax_rows"))


@pytest.mark.parametrize("case", GN_STATS, ids=N.case_ids(GN_STATS))
def test_gn_stats(hip, case):  # noqa: F811
    """sums and sums of squares bounded entry by entry; integer-valued inputs exact; the same bits from a second launch; the workspace the library asks for is the one traits() derives"""
    from followyourclick_amd import _lib as L
    c = case
    a = L.GnStatsArgs()
    a.rows, a.C, a.groups, a.rows_per_sample = c.S * c.rps, c.C, c.G, c.rps
    assert int(hip.lib.fyc_gn_stats_workspace(ctypes.byref(a))) == N.traits(c)["workspace"]
    ops, ref, bound = problem(c)
    got = launch_gn_stats(hip, c, ops)
    judge(c, ops, ref, bound, got, " exact" if c.kind == "int" else "")
    again = launch_gn_stats(hip, c, ops)
    assert torch.equal(again.view(torch.int64), got.view(torch.int64)), f"{c.name}: a second launch gave other bits"


@pytest.mark.parametrize("case", GN_APPLY, ids=N.case_ids(GN_APPLY))
def test_gn_apply(hip, case):  # noqa: F811
    """from the exact f64 statistics (the apply step alone) or, chained, from fyc_gn_stats' own; a constant group gives silu?(beta) to one ulp"""
    c = case
    ops, ref, bound = problem(c)
    if c.chained:
        sops = N.operands(ops.stats_case)
        sops.x = ops.x      # the very tensor the apply launch reads
        stats = flat(launch_gn_stats(hip, ops.stats_case, sops), sops).cuda()
    else:
        stats = ops.stats.contiguous().cuda()
    buf = ops.buf.cuda()
    hip.gn_apply(ops.x.cuda(), stats, ops.gamma.cuda(), ops.beta.cuda(), flat(buf, ops), rows=c.S * c.rps, C_=c.C, groups=c.G, rows_per_sample=c.rps, eps=c.eps, silu=c.silu)
    torch.cuda.synchronize()
    got = buf.cpu()
    judge(c, ops, ref, bound, got)
    if c.const_group is not None and not c.silu:
        cpg = c.C // c.G
        sl = slice(c.const_group * cpg, (c.const_group + 1) * cpg)
        g, r = N.window(got, *ops.win)[:, sl].double(), N.window(ref, *ops.win)[:, sl].double()
        assert bool(((g - r).abs() <= ulp(r, c.dt)).all()), f"{c.name}: the constant group is not beta to one ulp"


def cs_launch(hip, c, ops, cs=None):  # noqa: F811
    buf = ops.buf.cuda()
    two = bool(c.C2)
    kw = dict(rows=c.S * c.rps, C1=c.C1, C2=c.C2, groups=c.G, rows_per_sample=c.rps, eps=c.eps, silu=c.silu, x2=ops.xs[1].cuda() if two else None)
    if cs is not None:
        kw.update(cs1=cs[0], cs2=cs[1] if two else None)
    elif c.path == "cs":
        kw.update(cs1=ops.cs[0].cuda(), cs2=ops.cs[1].cuda() if two else None, cs_rows=c.rps // c.ss)
    else:
        kw.update(cs1=None, parts1=ops.parts[0].cuda(), tile_rows1=c.bm1, slots1=N.slots_of(c.bm1, c.pcs), parts_cs_rows=c.pcs)
        if two:
            kw.update(parts2=ops.parts[1].cuda(), tile_rows2=c.bm2, slots2=N.slots_of(c.bm2, c.pcs))
    hip.gn_apply_cs(ops.xs[0].cuda(), kw.pop("cs1"), ops.gamma.cuda(), ops.beta.cuda(), flat(buf, ops), **kw)
    torch.cuda.synchronize()
    return buf.cpu()


@pytest.mark.parametrize("case", GN_APPLY_CS, ids=N.case_ids(GN_APPLY_CS))
def test_gn_apply_cs(hip, case):  # noqa: F811
    """one or two sources, statistics as reduced f64 sums or as synthetic row-tile partials (NaN where a correct fold never reads); on the parts path the same output again from the
    sums fyc_chan_stats_reduce makes of those partials"""
    c = case
    ops, ref, bound = problem(c)
    got = cs_launch(hip, c, ops)
    judge(c, ops, ref, bound, got)
    if c.path == "parts":
        cs = []
        for i, x in enumerate(ops.xs):
            out = torch.full((c.S, x.shape[1], 2), float("nan"), dtype=torch.float64, device="cuda")
            hip.chan_stats_reduce(ops.parts[i].cuda(), out, rows=c.S * c.rps, N=x.shape[1], cs_rows=c.pcs, tile_rows=ops.bms[i], slots=N.slots_of(ops.bms[i], c.pcs), out_rows=c.rps)
            cs.append(out)
            torch.cuda.synchronize()
            for o in range(c.S):      # the launch against the fold of the same f32 values in the consumer's order: f64 sums, n 2^-53 sum |terms|
                acc, mag, n = N.fold(ops.parts[i], ops.bms[i], c.pcs, c.S * c.rps, o, c.rps // c.pcs)
                d = (out[o].cpu() - acc).abs()
                assert bool((d <= n * N.D53 * mag).all()), f"{c.name}: fyc_chan_stats_reduce and the fold disagree on source {i + 1}, sample {o}: {d.max().item():.3e}"
        via = cs_launch(hip, c, ops, cs=cs)
        judge(c, ops, ref, bound, via, " via-reduce")
        # not asserted equal: the fold adds the f64 terms tile by tile, the reduce launch on 8 strided lanes, so the sums may differ in their last bit and a mean that sits
        # beside an f32 rounding boundary may then move by one unit; both outputs are held to the same bound above, the count is for the log
        differ = int((N.window(via, *ops.win).double() != N.window(got, *ops.win).double()).sum())
        print(f"{c.name}: {differ} elements differ between the fold in the kernel and fyc_chan_stats_reduce")


@pytest.mark.parametrize("case", REDUCE, ids=N.case_ids(REDUCE))
def test_chan_stats_reduce(hip, case):  # noqa: F811
    """integer-valued partials: the f64 sums of the rows themselves, bit for bit"""
    c = case
    ops, ref, bound = problem(c)
    buf = ops.buf.cuda()
    hip.chan_stats_reduce(ops.parts.cuda(), flat(buf, ops), rows=ops.rows, N=c.N, cs_rows=c.cs_rows, tile_rows=c.bm, slots=N.slots_of(c.bm, c.cs_rows), out_rows=ops.group * c.cs_rows)
    torch.cuda.synchronize()
    judge(c, ops, ref, bound, buf.cpu(), " exact")


@pytest.mark.parametrize("case", LAYERNORM + ROW_STATS, ids=N.case_ids(LAYERNORM + ROW_STATS))
def test_layernorm_and_row_stats(hip, case):  # noqa: F811
    """every MAXCH at and past its edge, partial last blocks, the positional table by (row / pe_div) % pe_rows; row_stats judged on mean and rstd separately"""
    c = case
    ops, ref, bound = problem(c)
    buf = ops.buf.cuda()
    if c.op == "row_stats":
        hip.row_stats(ops.x.cuda(), flat(buf, ops), rows=c.rows, C_=c.C, eps=c.eps)
    else:
        kw = dict(pe=ops.pe.cuda(), pe_div=c.pe[0], pe_rows=c.pe[1]) if c.pe else {}
        hip.layernorm(ops.x.cuda(), ops.gamma.cuda(), ops.beta.cuda(), flat(buf, ops), rows=c.rows, C_=c.C, eps=c.eps, **kw)
    torch.cuda.synchronize()
    judge(c, ops, ref, bound, buf.cpu())


@pytest.mark.parametrize("case", SOFTMAX, ids=N.case_ids(SOFTMAX))
def test_softmax_rows(hip, case):  # noqa: F811
    """in place: 1 .. 16 laps of the column loop, pad columns [cols, ld) that keep their bits, causal rows whose masked part is exact zeros"""
    c = case
    ops, ref, bound = problem(c)
    buf = ops.buf.cuda()
    hip.softmax_rows(flat(buf, ops), rows=c.rows, cols=c.cols, ld=c.ld, causal_rows=c.causal)
    torch.cuda.synchronize()
    judge(c, ops, ref, bound, buf.cpu())
