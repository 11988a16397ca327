"""tests/kernel_compare.py::compare is neither trigger-happy nor blind (CPU, no kernel involved).

Not trigger-happy: for every distinct problem of tests/gemm_cases.py, in all three storage types, the emulator accumulating in f32 passes compare()
against the emulator accumulating in f64 with C_ACC = 1 - the reference stays inside its own bound, which is what lets the per-element bound be
asserted on the GPU without a measured number.  (Tile, ring and tuning do not exist on the emulator: the split-K and batched cases are plain problems.)

Not blind: six planted defects on the f64 reference of the 300 x 328 problem are all caught.  What the old close() says to the three that lie inside
the output, computed at the same tolerance (bf16 4e-3 / f16 5e-4) by test_old_close_verdicts:
    one element replaced by its neighbour's value   close() PASSES: rel-L2 1.0e-3 (bf16) / 1.4e-4 (f16), a quarter of the tolerance by the rule in
                                                    _neighbour, for an element whose whole row fails compare() (row rel-L2 1.7e-2 / 2.4e-3)
    two adjacent rows swapped                       close() still FAILS at M = 300: 2 N elements move by ~sqrt(2) rms, rel-L2 8.9e-2 ~ 2 / sqrt(M);
                                                    a defect confined to a fixed number of rows scales as 1 / sqrt(M) and this one slips under
                                                    4e-3 from M = 147 333 rows (f16, 5e-4: 9.4 million)
    one row-bias group shifted by one row           close() still FAILS at M = 300 (rel-L2 3.9e-2); under 4e-3 from M = 28 730 rows (f16: 1.8 million)
So at the size of these tests the single element is what close() misses; the row defects are missed at the row counts the UNet runs in bf16
(M up to 131 072), not at 300 rows.  The verdicts and the row counts are computed by the test, not assumed."""
import math
from dataclasses import replace

import pytest
import torch

import gemm_cases as G
import kernel_compare as KC
from kernel_compare import BoundTerms, Guard, compare
from test_kernels_gpu import RTOL, close


def _problems():
    seen, out = set(), []
    for c in G.by_group(*G.LINEAR_GROUPS):      # (the groups of the other epilogues have bounds of their own: tests/test_gemm_epilogue_cases.py)
        key = replace(c, name="", group="", dt="", tile=0, ring=0, tuning=(), chan=False, cs_rows=0, want_cfg=0, want_ring=0, want_wide=0, want_split=False)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


PROBLEMS = _problems()


def test_rtol_is_the_projects():
    assert KC.RTOL == RTOL


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("case", PROBLEMS, ids=[c.name for c in PROBLEMS])
def test_reference_stays_inside_its_own_bound(case, dt):
    assert KC.C_ACC >= 1.0
    c = replace(case, dt=dt)
    ops = G.operands(c)
    lo, hi = G.run_emulator(c, ops, torch.float32), G.run_emulator(c, ops, torch.float64)
    fig = compare(G.logical(c, lo), G.logical(c, hi), dtype=dt, bound_terms=BoundTerms(G.bound_terms(c, ops), c.K), guard=Guard(ops.buf, lo, ops.mask), tag=f"{c.name} as {dt}")
    print(f"{c.name} as {dt}: global {fig['global_rel']:.2e} row {fig['row_rel']:.2e} column {fig['column_rel']:.2e} element/bound {fig['elem_ratio']:.3f}")
    assert torch.equal(hi[~ops.mask], ops.buf[~ops.mask]), "the reference itself wrote outside the output"


# ---- planted defects -----------------------------------------------------------------------------------------------------------------
DEFECT_CASE = {"bf16": "plain-bf16-t0r0-rb96", "f16": "plain-f16-t0r0-rb96"}
_cache = {}


def _setup(dt):
    if dt not in _cache:
        c = G.BY_NAME[DEFECT_CASE[dt]]
        assert c.M >= 300 and c.N >= 328 and c.rowbias and c.ldo > c.N
        ops = G.operands(c)
        _cache[dt] = (c, ops, G.run_emulator(c, ops, torch.float64), G.run_emulator(c, ops, torch.float64, storage=torch.float64), G.bound_terms(c, ops))
    return _cache[dt]


def _neighbour(c, ref, dt):
    """element (17, j) takes the value of (17, j + 1), j chosen so that the two differ by a quarter of what moves the global rel-L2 to the tolerance:
    large against the element's own bound (0.47 vs an ulp of 2^-7 in bf16), invisible to close()"""
    target = 0.25 * RTOL[dt] * ref.double().norm().item()
    d = (ref[17, :-1].double() - ref[17, 1:].double()).abs()
    return 17, int((d - target).abs().argmin())


def _plant(defect, dt):
    c, ops, ref_buf, exact_buf, S = _setup(dt)
    got_buf = ref_buf.clone()
    got, ref = G.logical(c, got_buf), G.logical(c, ref_buf)
    o0 = G.out_offset(c)
    if defect == "neighbour":
        i, j = _neighbour(c, ref, dt)
        assert ref[i, j] != ref[i, j + 1]
        got[i, j] = ref[i, j + 1]
    elif defect == "rows_swapped":
        got[[130, 131]] = ref[[131, 130]]
    elif defect == "rowbias_group_shifted":
        g = 2
        rb = torch.as_strided(ops.rb_table, (4, c.N), (c.ldrb, 1), c.rb_off).double()
        got[g * c.rpb] = (G.logical(c, exact_buf)[g * c.rpb] + (rb[g - 1] - rb[g]) * c.out_scale).to(got.dtype)
    elif defect == "run_unwritten":
        got[200, 320:328] = G.logical(c, ops.buf)[200, 320:328]
    elif defect == "pad_column":
        k = o0 + 77 * c.ldo + c.N + 2
        assert not ops.mask[k]
        got_buf[k] = -got_buf[k]
    elif defect == "front":
        assert not ops.mask[o0 - 1]
        got_buf[o0 - 1] = -got_buf[o0 - 1]
    else:
        raise KeyError(defect)
    return c, ops, got_buf, ref_buf, S


DEFECTS = ["neighbour", "rows_swapped", "rowbias_group_shifted", "run_unwritten", "pad_column", "front"]


def _old_close_rel(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm()).item()


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_the_unharmed_reference_passes(dt):
    c, ops, ref_buf, _, S = _setup(dt)
    compare(G.logical(c, ref_buf), G.logical(c, ref_buf), dtype=dt, bound_terms=BoundTerms(S, c.K), guard=Guard(ops.buf, ref_buf, ops.mask), tag="unharmed")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defect_is_caught(defect, dt):
    c, ops, got_buf, ref_buf, S = _plant(defect, dt)
    with pytest.raises(AssertionError) as e:
        compare(G.logical(c, got_buf), G.logical(c, ref_buf), dtype=dt, bound_terms=BoundTerms(S, c.K, G.tile_shape(c.want_cfg)), guard=Guard(ops.buf, got_buf, ops.mask),
                tag=f"planted {defect}")
    msg = str(e.value)
    print(f"{defect} {dt}: old close() rel-L2 {_old_close_rel(G.logical(c, got_buf), G.logical(c, ref_buf)):.3e} (tolerance {RTOL[dt]:.0e}); compare: {msg[:200]}")
    where = {"neighbour": "row 17,", "rows_swapped": "row 130", "rowbias_group_shifted": "row 192", "run_unwritten": "row 200, column 32",
             "pad_column": "outside the output", "front": "-1 from the first output element"}[defect]
    assert where in msg, msg


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_old_close_verdicts(dt):
    """what close() says to the three defects inside the output, computed (see the head of the file)"""
    rel = {}
    for defect in DEFECTS[:3]:
        c, ops, got_buf, ref_buf, S = _plant(defect, dt)
        rel[defect] = _old_close_rel(G.logical(c, got_buf), G.logical(c, ref_buf))
    tol = RTOL[dt]
    # the single element: close() passes it - the gap at any size
    c, ops, got_buf, ref_buf, S = _plant("neighbour", dt)
    close(G.logical(c, got_buf), G.logical(c, ref_buf), "one element", tol)
    assert 0.1 * tol < rel["neighbour"] <= tol
    # the row defects: a defect confined to one or two rows of M scales as 1 / sqrt(M).  At M = 300 close() still sees them; the same
    # defect in the same data repeated to the row counts the engine runs does not reach the tolerance, which is computed here, not assumed
    for defect, rows_hit in (("rows_swapped", 2), ("rowbias_group_shifted", 1)):
        assert rel[defect] > tol, (defect, rel[defect])
        m_pass = math.ceil(c.M * (rel[defect] / tol) ** 2)
        at = rel[defect] * math.sqrt(c.M / m_pass)
        assert at <= tol
        print(f"{defect} {dt}: close() rel-L2 {rel[defect]:.3e} at M = {c.M}; under {tol:.0e} from M = {m_pass} rows")
        if dt == "bf16" and rows_hit == 1:
            assert m_pass <= 131072, "a shifted row-bias group passes close() at a row count the engine runs"
