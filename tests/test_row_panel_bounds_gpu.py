"""fyc_panel_linear, fyc_ff_block and fyc_temporal_block (both kernels) on the cases of tests/row_panel_cases.py (what each case launches and that the list reaches every instantiation and host-side branch is
proven on the CPU by tests/test_row_panel_cases.py).  Every case is one launch into an output - the chan_parts buffer of fyc_ff_block included - that lies inside a larger,
prefilled buffer (64 elements in front, two rows behind), compared with the reference of EmuOps(acc=float64) by kernel_compare.compare: finite, the global relative L2 at the
tolerance of the existing test of the same op, the relative L2 of every row and of every column, EVERY element within the bound derived from the kernel's rounding points
(tests/kernel_compare.py), nothing outside the output touched.  chan_parts is held, entry by entry, against the f64 sums of the values the kernel stored; an integer-valued
output must give exact sums.  A residual that aliases the output must give the bits of the out-of-place launch.  Misaligned operands and unsupported shapes are refused by the
host-side validation before any launch.

FYC_PANEL_FIGURES=<file>: append the figures of every comparison to that file (profiles/row_panel_bound_coverage.txt was made from it)."""
import os

import pytest
import torch

import row_panel_cases as RP
from kernel_compare import Guard, compare
from test_kernels_gpu import hip  # noqa: F401  (the module-scoped library fixture)

pytestmark = pytest.mark.gpu

FIGURES = os.environ.get("FYC_PANEL_FIGURES")


def flat(buf, rows, cols):
    """the output as the kernel sees it: the buffer from the first element of the window on"""
    return buf[RP.FRONT:RP.FRONT + rows * cols]


def cu(t):
    return t.cuda() if t is not None else None


def judge(c, ops, ref, bound, got, note=""):
    fig = compare(RP.window(got, *ops.win), RP.window(ref, *ops.win), dtype=c.dt, bound=bound, rtol=RP.rtol(c), labels=RP.labels(c), lines=True,
                  guard=Guard(ops.buf, got, ops.mask), tag=c.name)
    print(f"{c.name}: global rel-L2 {fig['global_rel']:.3e} (tolerance {RP.rtol(c):.1e}), worst element at {fig['elem_ratio']:.3f} of its bound{note}")
    if FIGURES:
        with open(FIGURES, "a") as f:
            f.write(f"{c.op} {c.dt} {c.name} {fig['global_rel']:.3e} {fig['elem_ratio']:.4f}{note}\n")
    return fig


def panel_kw(c, ops):
    kw = dict(wstream=ops.ws.cuda(), rows=c.rows, N=c.N, K=c.K, bias=cu(ops.bias))
    if c.gn != "none":
        kw.update(gn_gamma=ops.gamma.cuda(), gn_beta=ops.beta.cuda(), gn_rows_per_sample=c.rps, gn_stat_samples=c.ss, gn_groups=c.groups, gn_eps=RP.GN_EPS)
        if c.gn == "cs":
            kw.update(gn_cs=ops.gn_cs.cuda())
        else:
            kw.update(gn_parts=ops.parts.cuda(), gn_tile_rows=c.bm, gn_slots=ops.slots)
    return kw


@pytest.mark.parametrize("case", RP.PANEL_CASES, ids=RP.case_ids(RP.PANEL_CASES))
def test_panel_linear(hip, case):  # noqa: F811
    """all eight instantiations; GroupNorm from f64 sums (one or two tiles per sample, 1 / 2 / 4 statistics samples, 32 or 8 groups) or from row-tile partials with NaN where a
    correct fold never reads; bias present and absent; residual absent, separate, and aliasing the output (the bits of the out-of-place launch, whose residual stays as it was)"""
    c = case
    ops, ref, bound = RP.problem(c)
    kw = panel_kw(c, ops)
    x = ops.x.cuda()
    buf = ops.buf.cuda()
    out = flat(buf, c.rows, c.N)
    hip.panel_linear(x, out, residual=out if c.res == "alias" else cu(ops.res), **kw)
    torch.cuda.synchronize()
    got = buf.cpu()
    judge(c, ops, ref, bound, got)
    if c.res == "alias":
        buf2 = RP.guarded(c.rows, c.N, RP.DT[c.dt])[0].cuda()
        res2 = ops.res.cuda()
        hip.panel_linear(x, flat(buf2, c.rows, c.N), residual=res2, **kw)
        torch.cuda.synchronize()
        assert torch.equal(RP.window(buf2.cpu(), *ops.win).view(torch.int16), RP.window(got, *ops.win).view(torch.int16)), f"{c.name}: the aliased residual gave other bits"
        assert torch.equal(res2.cpu().view(torch.int16), ops.res.view(torch.int16)), f"{c.name}: the out-of-place launch wrote to its residual"


@pytest.mark.parametrize("case", RP.FF_CASES, ids=RP.case_ids(RP.FF_CASES))
def test_ff_block(hip, case):  # noqa: F811
    """both types; residual absent, separate and aliased; with and without chan_parts (guarded too, every entry against the f64 sums of the values as stored); rows with a large
    mean and constant rows; an integer-valued output whose statistics must be exact"""
    c = case
    ops, ref, bound = RP.problem(c)
    tiles = c.rows // 128
    kw = dict(wstream=ops.ws.cuda(), b_out=ops.b_out.cuda(), rows=c.rows, C_=RP.C_FF, hidden=RP.HID, eps=RP.LN_EPS, cs_rows=c.cs_rows)
    assert ops.ws.numel() * 2 == hip.ff_block_wstream_bytes()
    x = ops.x.cuda()
    buf = ops.buf.cuda()
    out = flat(buf, c.rows, RP.C_FF)
    pbuf = ops.pbuf.cuda() if c.cs_rows else None
    hip.ff_block(x, out if c.res == "alias" else cu(ops.res), out, chan_parts=flat(pbuf, *ops.pwin) if c.cs_rows else None, **kw)
    torch.cuda.synchronize()
    got = buf.cpu()
    judge(c, ops, ref, bound, got)
    if c.cs_rows:
        pgot = pbuf.cpu()
        pref, pbound, exact = RP.parts_reference(RP.window(got, *ops.win))
        fig = compare(RP.window(pgot, *ops.pwin), pref, dtype="f32", bound=pbound, rtol=2e-5, guard=Guard(ops.pbuf, pgot, ops.pmask), tag=c.name + " statistics",
                      labels=RP.KC.Labels(lambda i: f"tile {i}", lambda j: f"channel {j // 2}, {'sum' if j % 2 == 0 else 'sum of squares'}"))
        print(f"{c.name}: statistics of {tiles} tiles, worst entry at {fig['elem_ratio']:.3f} of its bound")
        if FIGURES:
            with open(FIGURES, "a") as f:
                f.write(f"{c.op} {c.dt} {c.name}/statistics {fig['global_rel']:.3e} {fig['elem_ratio']:.4f}\n")
        if c.recipe == "integer":
            assert torch.equal(RP.window(got, *ops.win).double(), ops.x.double() + ops.res.double()), f"{c.name}: identity projection, zero feed-forward: the output is tokens + residual"
            assert torch.equal(RP.window(pgot, *ops.pwin).double(), exact), f"{c.name}: integer-valued output, but the sums are not exact"
    if c.res == "alias":
        buf2 = RP.guarded(c.rows, RP.C_FF, RP.DT[c.dt])[0].cuda()
        res2 = ops.res.cuda()
        hip.ff_block(x, res2, flat(buf2, c.rows, RP.C_FF), **kw)
        torch.cuda.synchronize()
        assert torch.equal(RP.window(buf2.cpu(), *ops.win).view(torch.int16), RP.window(got, *ops.win).view(torch.int16)), f"{c.name}: the aliased residual gave other bits"
        assert torch.equal(res2.cpu().view(torch.int16), ops.res.view(torch.int16)), f"{c.name}: the out-of-place launch wrote to its residual"


@pytest.mark.parametrize("case", RP.TB_CASES, ids=RP.case_ids(RP.TB_CASES))
def test_temporal_block(hip, case):  # noqa: F811
    """the LDS-tile kernel and the register-resident one (packed stream), both types, with and without pe_bias: two clips of two pixel tiles each (four workgroups) and one tile"""
    c = case
    ops, ref, bound = RP.problem(c)
    shape = dict(clips=c.clips, frames=RP.TB_F, pixels=c.P, heads=RP.TB_H, d=RP.TB_D)
    assert hip.temporal_block_supported(RP.DT[c.dt], **shape)
    buf = ops.buf.cuda()
    hip.temporal_block(ops.x.cuda(), flat(buf, c.rows, RP.TB_C), **{k: cu(v) for k, v in ops.kw.items()}, **shape, scale=RP.TB_SCALE, eps=RP.LN_EPS)
    torch.cuda.synchronize()
    judge(c, ops, ref, bound, buf.cpu())


def _off8(t):
    """the same values 8 bytes further on: a view that is not 16-byte aligned"""
    big = torch.empty(t.numel() + 8, dtype=t.dtype, device="cuda")
    v = big[4:4 + t.numel()] if t.element_size() == 2 else big[2:2 + t.numel()]
    v.copy_(t.reshape(-1))
    assert v.data_ptr() % 16 == 8
    return v


@pytest.mark.parametrize("dt", list(RP.DT))
def test_refusals_before_any_launch(hip, dt):  # noqa: F811
    """host validation only: every call here must raise FycError, and the outputs keep their prefill (nothing was launched)"""
    from followyourclick_amd._lib import FycError
    T = RP.DT[dt]
    c = next(c for c in RP.PANEL_CASES if c.dt == dt and c.gn == "cs" and c.res == "sep")
    ops = RP.operands(c)
    slack = 128 * max(c.N, c.K)      # room for the rows a wrongly accepted call would touch
    x = torch.zeros(c.rows * c.K + slack, dtype=T, device="cuda")[:c.rows * c.K].copy_(ops.x.reshape(-1))
    res = torch.zeros(c.rows * c.N + slack, dtype=T, device="cuda")[:c.rows * c.N].copy_(ops.res.reshape(-1))
    buf = torch.cat([ops.buf, ops.buf[:slack]]).cuda()
    before = buf.clone()
    out = flat(buf, c.rows, c.N)
    kw = panel_kw(c, ops)
    plain = dict(wstream=kw["wstream"], rows=c.rows, N=c.N, K=c.K, bias=kw["bias"])
    hip.panel_linear(x, out, residual=res, **kw)      # the case itself is accepted
    torch.cuda.synchronize()
    buf.copy_(before)
    calls = {
        "x + 8 bytes": lambda: hip.panel_linear(_off8(x), out, residual=res, **plain),
        "out + 8 bytes": lambda: hip.panel_linear(x, buf[RP.FRONT + 4:RP.FRONT + 4 + c.rows * c.N], residual=res, **plain),
        "residual + 8 bytes": lambda: hip.panel_linear(x, out, residual=_off8(res), **plain),
        "wstream + 8 bytes": lambda: hip.panel_linear(x, out, residual=res, **dict(plain, wstream=_off8(kw["wstream"]))),
        "rows + 64": lambda: hip.panel_linear(x, out, residual=res, **dict(plain, rows=c.rows + 64)),
        "gn_rows_per_sample = 64": lambda: hip.panel_linear(x, out, residual=res, **dict(kw, gn_rows_per_sample=64)),
        "gn_cs and gn_parts": lambda: hip.panel_linear(x, out, residual=res, **dict(kw, gn_parts=torch.zeros(c.rows // 128 * c.K * 2, device="cuda"), gn_tile_rows=128, gn_slots=1)),
    }
    for what, call in calls.items():
        with pytest.raises(FycError):
            call()
            pytest.fail(f"fyc_panel_linear accepted {what}")
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int16), before.view(torch.int16)), "a refused fyc_panel_linear call wrote to its output"

    f = next(c for c in RP.FF_CASES if c.dt == dt and c.res == "sep" and c.recipe == "random")
    fo = RP.operands(f)
    n = f.rows * RP.C_FF
    slack = 128 * RP.C_FF
    x = torch.zeros(n + slack, dtype=T, device="cuda")[:n].copy_(fo.x.reshape(-1))
    res = torch.zeros(n + slack, dtype=T, device="cuda")[:n].copy_(fo.res.reshape(-1))
    buf = torch.cat([fo.buf, fo.buf[:slack]]).cuda()
    before = buf.clone()
    out = flat(buf, f.rows, RP.C_FF)
    kw = dict(wstream=fo.ws.cuda(), b_out=fo.b_out.cuda(), rows=f.rows, C_=RP.C_FF, hidden=RP.HID, eps=RP.LN_EPS)
    calls = {
        "x + 8 bytes": lambda: hip.ff_block(_off8(x), res, out, **kw),
        "out + 8 bytes": lambda: hip.ff_block(x, res, buf[RP.FRONT + 4:RP.FRONT + 4 + n], **kw),
        "residual + 8 bytes": lambda: hip.ff_block(x, _off8(res), out, **kw),
        "wstream + 8 bytes": lambda: hip.ff_block(x, res, out, **dict(kw, wstream=_off8(kw["wstream"]))),
        "rows + 64": lambda: hip.ff_block(x, res, out, **dict(kw, rows=f.rows + 64)),
    }
    for what, call in calls.items():
        with pytest.raises(FycError):
            call()
            pytest.fail(f"fyc_ff_block accepted {what}")
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int16), before.view(torch.int16)), "a refused fyc_ff_block call wrote to its output"
