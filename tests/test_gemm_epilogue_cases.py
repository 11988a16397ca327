"""The bounds of the GEGLU, head-split, activation, LayerNorm-fold, dual-source and unsplit-T3 cases of tests/gemm_cases.py are neither trigger-happy nor blind (CPU, no
kernel involved).

Not trigger-happy: a torch model of every form a case declares - f32 tensors combined in the kernel's order, the fold as two FMAs where the source fuses, the polynomial or
the Abramowitz-Stegun gate as the kernel has it, one rounding to the storage type - stays inside the bound of every case, with the constant 1.  The constants the bounds use
(the slopes DG and DQ, the approximation errors PHI_ERR and GELU_AS_ERR) are evaluated on grids here, not copied.

Not blind: every declared single-site defect (gemm_cases.DEFECTS) leaves the bound or trips the guard on at least one case of its group, in every storage type it applies to.

The reference is EmuOps(acc=float64): exact-erf GELU.  The 16-bit GEGLU kernels use a polynomial gate; what that alone costs in the project's global measure is computed by
test_polynomial_gate_alone_is_inside_the_global_tolerances."""
import math

import pytest
import torch

import gemm_cases as G
import row_panel_cases as RP
from kernel_compare import RTOL

NEW = G.by_group(*G.EPILOGUE_GROUPS)
_refs = {}


def reference(c):
    key = G.problem_key(c)
    if key not in _refs:
        ops = G.operands(c)
        _refs[key] = (ops,) + G.epilogue_reference(c, ops)
    return _refs[key]


def _forms():
    """one case per (problem, form): the model does not know tiles or pre-staging"""
    seen, out = set(), []
    for c in NEW:
        key = (G.problem_key(c), c.want_form, c.want_wide)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


FORMS = _forms()


def test_constants_on_grids():
    x = torch.linspace(-12.0, 12.0, (1 << 22) + 1, dtype=torch.float64)
    # slopes: d/dx (x Phi(x)) and d/dx (x sigmoid(1.702 x))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    dg = (RP.Phi(x) + x * pdf).abs().max().item()
    s = torch.sigmoid(G.QUICK_C * x)
    dq = (s + G.QUICK_C * x * s * (1.0 - s)).abs().max().item()
    print(f"max |d gelu| {dg:.4f} (DG {RP.DG}), max |d quick-gelu| {dq:.4f} (DQ {G.DQ})")
    assert 1.12 < dg <= RP.DG and 1.09 < dq <= G.DQ
    # the Abramowitz-Stegun form against the exact GELU on a grid twice as fine as the one the bound was made from
    err = (G.gelu_as(x)[0] - G.gelu_exact(x)).abs().max().item()
    print(f"gelu_erf_f approximation error {err:.3e} (bound constant {G.GELU_AS_ERR:.3e}); polynomial Phi error {RP.PHI_ERR:.3e}")
    assert err <= G.GELU_AS_ERR + 1e-10 and 1e-7 < G.GELU_AS_ERR < 2.5e-7
    # its f32 evaluation, operation by operation, against the f64 evaluation of the same form: inside the running bound
    g32 = torch.linspace(-9.0, 9.0, 200001, dtype=torch.float32)
    val, bound = G.gelu_as(g32)
    got = G._gelu_as32(g32).double()
    ratio = ((got - val).abs() / (bound + 2.0 ** -126)).max().item()
    print(f"f32 evaluation of gelu_erf_f: worst error / running bound {ratio:.3f}")
    assert ratio <= 1.0
    val, bound = G.quick_gelu(g32)
    got = (g32 / (1.0 + torch.exp(torch.tensor(-G.QUICK_C, dtype=torch.float32) * g32))).double()
    ratio = ((got - val).abs() / (bound + 2.0 ** -126)).max().item()
    print(f"f32 evaluation of quick-GELU: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("case", FORMS, ids=G.case_ids(FORMS))
def test_model_stays_inside_the_bound(case):
    ops, ref_bufs, bounds = reference(case)
    figs = G.judge(case, ops, G.model(case, ops), ref_bufs, bounds)
    print(case.name, case.want_form, " ".join(f"{f['tag'].split()[-1]}: global {f['global_rel']:.2e} element/bound {f['elem_ratio']:.3f}" for f in figs))
    for b, r, m in zip(ops.bufs, ref_bufs, ops.masks):      # the reference itself wrote nothing outside its windows
        assert torch.equal(r[~m], b[~m])


def _applies(c, defect):
    if defect == "straddle_first_head":
        return c.heads[0] // c.heads[1] == 40 and not c.heads[3][0] and c.ln == 1
    if defect in ("vt_run_shifted", "vt_pad_write"):
        return 1 in c.heads[3] and c.heads[2] >= 24
    if defect == "gelu_tanh":
        return c.act == 1
    return True


DEFECT_PARAMS = [(g, d, dt) for g in G.EPILOGUE_GROUPS for d in G.DEFECTS[g] for dt in ("bf16", "f16", "f32")]


@pytest.mark.parametrize("group,defect,dt", DEFECT_PARAMS, ids=[f"{g}-{d}-{dt}" for g, d, dt in DEFECT_PARAMS])
def test_declared_defect_leaves_the_bound(group, defect, dt):
    cases = [c for c in FORMS if c.group == group and c.dt == dt and _applies(c, defect)]
    assert cases, "no case of this group and type exposes the defect"
    caught = []
    for c in cases:
        ops, ref_bufs, bounds = reference(c)
        try:
            G.judge(c, ops, G.model(c, ops, defect), ref_bufs, bounds)
        except AssertionError as e:
            caught.append((c.name, str(e)[:220]))
    print(f"{defect} {dt}: caught on {len(caught)} of {len(cases)} forms; first: {caught[:1]}")
    assert caught, f"{defect} stays inside the bound of every {group} case in {dt}"
    if defect == "vt_pad_write":
        assert all("outside the output" in msg for _, msg in caught)      # only the guard can see it: the pad columns belong to no window


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_polynomial_gate_alone_is_inside_the_global_tolerances(dt):
    """the exact reference with nothing changed but the gate's Phi replaced by the kernel's polynomial (in f64): its global relative L2 beside the tolerance close() and compare() use"""
    c = G.BY_NAME[f"geglu-{dt}-ln0-t0"]
    ops = G.operands(c)
    A, W = G.operand_matrix(c, ops).double(), ops.w[:, :c.K].double()
    blk = (A @ W.t() + ops.bias.double()).reshape(c.M, c.N // 32, 2, 16)
    v, g = blk[:, :, 0], blk[:, :, 1]
    exact, poly = v * g * RP.Phi(g), v * g * RP.phi_poly(g)
    rel = ((poly - exact).norm() / exact.norm()).item()
    print(f"{dt}: gate pre-activations of standard deviation {g.std().item():.2f}; polynomial gate alone: rel-L2 {rel:.2e} (tolerance {RTOL[dt]:.0e})")
    assert 0.8 < g.std().item() < 1.3
    assert g.mean(dim=0).min().item() > 0.5      # the condition on the inputs that gemm_cases.epilogue_operands states
    assert rel <= 0.25 * RTOL["f16"]
    g0 = g - G.GEGLU_GATE_BIAS      # the same gates centred on zero, where the polynomial is at its worst relative to the output
    rel0 = ((v * g0 * RP.phi_poly(g0) - v * g0 * RP.Phi(g0)).norm() / (v * g0 * RP.Phi(g0)).norm()).item()
    print(f"{dt}: the same with gates centred on zero: rel-L2 {rel0:.2e}")
    assert rel < rel0 <= 0.25 * RTOL["f16"]
