"""The case list of tests/row_panel_cases.py, checked on the CPU: it reaches every instantiation of csrc/panel_linear.hip, csrc/ff_block.hip, csrc/temporal_block.hip and csrc/temporal_block_rr.hip and every host-side branch that
traits() names; the f32 model of each kernel's rounding points stays inside the per-element bound of every case; every declared defect leaves it; the shares of
boundary-charged intermediates stay under their caps (a condition on the inputs, from the reference alone); the error constant of the GEGLU polynomial is the one the bound uses;
every shape is one EmuOps.*_supported accepts."""
import math

import pytest
import torch

import row_panel_cases as RP
from emu_ops import EmuOps
from kernel_compare import Guard, compare, ulp


def _window(c, buf):
    return RP.window(buf, c.rows, c.cols)


def _judge(c, ops, ref, bound, got):
    return compare(_window(c, got), _window(c, ref), dtype=c.dt, bound=bound, rtol=RP.rtol(c), labels=RP.labels(c), lines=True, guard=Guard(ops.buf, got, ops.mask), tag=c.name)


def test_case_list_reaches_every_instantiation_and_branch():
    tr = [(c, RP.traits(c)) for c in RP.CASES]
    assert {(c.op, t["inst"]) for c, t in tr} == RP.built()
    pl = [t for c, t in tr if c.op == "panel_linear"]
    for dt in RP.DT:
        mine = [t for t in pl if t["inst"][0] == dt]
        assert {t["gn"] for t in mine} == {"none", "cs", "parts"}
        assert {t["bias"] for t in mine} == {True, False} and {t["residual"] for t in mine} == {"none", "sep", "alias"}
        gn = [t for t in mine if t["gn"] == "cs"]
        assert {t["tiles_per_sample"] for t in gn} == {1, 2} and {t["stat_samples"] for t in gn} == {1, 2, 4} and all(t["samples"] >= 2 for t in gn)
        assert {t["cpg"] for t in gn} >= {10, 20, 40, 80}                       # 32 groups and 8 groups at both K
        assert {t["channel_laps"] for t in gn} == {2, 3}
        assert {(t["gn"], t["residual"]) for t in mine} >= {("cs", "alias"), ("none", "alias")} and any(t["residual"] == "alias" and t["passes"] == 2 for t in mine)
        parts = [t for t in mine if t["gn"] == "parts"]
        assert {(t["fold"], t["slots"]) for t in parts} == {("fast", 1), ("general", 2), ("general", 3)}
        assert any(t["fold_unrolled"] for t in parts) and any(t["fold_tail"] for t in parts) and any(t["missing_samples"] for t in parts)
    assert {c.rows for c in RP.PANEL_CASES} == {256, 512} and {c.rows for c in RP.FF_CASES} == {256, 384}
    ff = [t for c, t in tr if c.op == "ff_block"]
    for dt in RP.DT:
        mine = [t for t in ff if t["inst"] == dt]
        assert {t["residual"] for t in mine} == {"none", "sep", "alias"} and {t["cs_rows"] for t in mine} == {0, 128, 256}
    tb = [(c, t) for c, t in tr if c.op == "temporal_block"]
    for dt in RP.DT:
        for kern in ("rr", "lds"):
            mine = [(c, t) for c, t in tb if t["inst"] == (dt, kern)]
            assert {(t["pe"], c.clips, c.P, t["workgroups"], t["tiles_per_clip"]) for c, t in mine} == {(pe, cl, P, wg, tpc) for pe in (True, False) for cl, P, wg, tpc in ((2, 16, 4, 2), (1, 8, 1, 1))}
    for op, want in (("temporal_block", {"mask_last", "pe_next", "head_shift", "swap_tiles", "swap_clips"}), ("panel_linear", {"tile_copy", "sample0", "fold_short", "drop_kstep", "pass_w", "pass_bias", "res_cols"}),
                     ("ff_block", {"drop39", "bias_prev", "swap_vg", "proj_xn", "mean0", "stats_slot"})):
        for dt in RP.DT:
            assert {d for c in RP.CASES if c.op == op and c.dt == dt for d in c.defects} == want, (op, dt)


def test_every_shape_is_supported_by_the_emulator():
    emu = EmuOps()
    for c in RP.PANEL_CASES:
        assert emu.panel_linear_supported(RP.DT[c.dt], rows=c.rows, N=c.N, K=c.K, gn_rows_per_sample=c.rps, gn_groups=c.groups), c.name
    for c in RP.TB_CASES:
        assert emu.temporal_block_supported(RP.DT[c.dt], clips=c.clips, frames=RP.TB_F, pixels=c.P, heads=RP.TB_H, d=RP.TB_D), c.name
    for c in RP.FF_CASES:
        assert emu.ff_block_supported(RP.DT[c.dt], rows=c.rows, C_=RP.C_FF, hidden=RP.HID, cs_rows=c.cs_rows), c.name


def test_geglu_polynomial_error_is_the_constant_of_the_bound():
    """the constant comes from the polynomial itself: a second, finer and shifted grid finds nothing larger, it is far from the 9e-5 that csrc/fyc_common.h quotes for
    x Phi(x) (another quantity), the clamp ends are 0 and 1 to well within it, and DG bounds the slope of g Phi(g)"""
    assert RP.PHI_ERR == RP.phi_poly_error()
    fine = RP.phi_poly_error(-6.0 + 1e-7, 6.0, (1 << 23) + 3)
    assert fine <= RP.PHI_ERR * (1 + 1e-6) and fine >= RP.PHI_ERR * 0.999, (fine, RP.PHI_ERR)
    assert 1e-5 < RP.PHI_ERR < 5e-4
    ends = RP.phi_poly(torch.tensor([-5.0, 5.0], dtype=torch.float64))
    assert abs(ends[0].item()) < RP.PHI_ERR and abs(ends[1].item() - 1.0) < RP.PHI_ERR
    g = torch.linspace(-8, 8, (1 << 20) + 1, dtype=torch.float64)
    slope = RP.Phi(g) + g * torch.exp(-g * g / 2) / math.sqrt(2 * math.pi)
    assert slope.abs().max().item() <= RP.DG
    # the f32 evaluation of the model agrees with the f64 polynomial to the roundings the bound charges for it
    g32 = torch.linspace(-6, 6, 100001)
    got, want = RP.geglu32(torch.ones_like(g32), g32).double(), g32.double() * RP.phi_poly(g32)
    assert bool(((got - want).abs() <= g32.double().abs() * RP.phi_rounding(g32) + 3 * RP.u * want.abs()).all())


def test_fma32_is_correctly_rounded():
    a = torch.tensor([1.0 + 2.0 ** -12, 3.0, 1.0 + 2.0 ** -12])
    c = torch.tensor([2.0 ** -60, 2.0 ** -30, -(2.0 ** -60)])
    # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24: exactly between two f32 numbers; the third term decides
    got = RP.fma32(a, a, c)
    assert got[0].item() == 1.0 + 2.0 ** -11 + 2.0 ** -23 and got[2].item() == 1.0 + 2.0 ** -11 and got[1].item() == 9.0


@pytest.mark.parametrize("case", RP.CASES, ids=RP.case_ids(RP.CASES))
def test_model_inside_the_bound_and_defects_outside(case):
    c = case
    ops, ref, bound = RP.problem(c)
    info = ops.info
    assert info.xn_share <= RP.XN_CAP, f"{c.name}: {info.xn_share:.4f} of a row's normalised elements are boundary-charged: change the recipe (or row_panel_cases.SALT), not the cap"
    if c.op == "ff_block":
        assert info.hid_share <= RP.HID_CAP, f"{c.name}: {info.hid_share:.4f} of a row's hidden elements are boundary-charged: change the recipe, not the cap"
    assert torch.isfinite(bound).all() and bool((bound >= ulp(_window(c, ref).double(), c.dt)).all())
    m = RP.model(c, ops)
    pbuf = None
    if c.op == "ff_block":
        m, pbuf = m
    fig = _judge(c, ops, ref, bound, m)
    print(f"{c.name}: model at {fig['elem_ratio']:.3f} of the bound, global rel-L2 {fig['global_rel']:.2e}")

    def parts_ok(out_buf, parts_buf):
        pref, pbound, _ = RP.parts_reference(_window(c, out_buf))
        compare(RP.window(parts_buf, *ops.pwin), pref, dtype="f32", bound=pbound, rtol=2e-5, labels=RP.labels(c), guard=Guard(ops.pbuf, parts_buf, ops.pmask), tag=c.name + " statistics")
    if pbuf is not None:
        parts_ok(m, pbuf)
    for d in c.defects:
        bad = RP.model(c, ops, d)
        with pytest.raises(AssertionError):
            if d == "stats_slot":
                parts_ok(*bad)
            else:
                _judge(c, ops, ref, bound, bad[0] if isinstance(bad, tuple) else bad)
    if c.op == "ff_block" and c.recipe == "integer":
        pref, _, exact = RP.parts_reference(_window(c, m))
        assert torch.equal(RP.window(pbuf, *ops.pwin).double(), exact), f"{c.name}: integer-valued output, but the model's sums are not the f64 sums"
        assert torch.equal(_window(c, m).double(), ops.x.double() + ops.res.double())
