"""The normalisation cases of tests/norm_cases.py without a GPU: traits() shows that the list reaches every instantiation and every host-side branch of csrc/norm.hip and
csrc/chan_parts.h; a torch model of each kernel's rounding points stays inside kernel_compare.compare() with the derived per-element bound on EVERY case (the bound admits the
design); every planted defect leaves the bound or the exact equality (the bound rejects what it is there to catch), where the global relative L2 of the existing tests
(test_kernels_gpu.close) lets a 1e-4 error of every sum and a single wrong element pass."""
import functools

import pytest
import torch

import norm_cases as N
from kernel_compare import Guard, compare, ulp
from test_kernels_gpu import close

BIG = [c for c in N.CASES if c.op == "gn_apply" and c.S * c.rps * c.C > 1 << 22]
SMALL = [c for c in N.CASES if c not in BIG]


@functools.lru_cache(maxsize=64)
def problem(c):
    ops = N.operands(c)
    return (ops,) + tuple(N.reference(c, ops))


def judge(c, got, rtol=None):
    ops, ref, bound = problem(c)
    buf = ops.buf.clone()
    N.window(buf, *ops.win).copy_(got)
    return compare(N.window(buf, *ops.win), N.window(ref, *ops.win), dtype=c.dt, bound=bound, rtol=N.rtol(c) if rtol is None else rtol, labels=N.labels(c),
                   guard=Guard(ops.buf, buf, ops.mask), tag=c.name)


def rejected(c, got):
    with pytest.raises(AssertionError, match="outside|non-finite"):
        judge(c, got, rtol=float("inf"))


def pick(op, dt=None, **kw):
    for c in N.by_op(op):
        if (dt is None or c.dt == dt) and all(getattr(c, k) == v for k, v in kw.items()):
            return c
    raise KeyError((op, dt, kw))


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------
def test_every_entry_point_runs_in_every_dtype():
    for op in ("gn_stats", "gn_apply", "gn_apply_cs", "layernorm", "row_stats", "softmax_rows"):
        assert {c.dt for c in N.by_op(op)} == set(N.DTS), op
    assert N.by_op("chan_stats_reduce")


def test_gn_stats_coverage():
    for dt in N.DTS:
        cs = [c for c in N.by_op("gn_stats") if c.dt == dt]
        ts = [N.traits(c) for c in cs]
        assert {c.C for c in cs} == {8, 64, 320, 960, 1920, 2040, 2048, 2056, 2560, 4096}
        assert {t["nthr_rule"] for t in ts} == {"256", "c8"} and {255, 256, 257} <= {t["C8"] for t in ts}
        assert {t["nthr"] for t in ts} == {256, 320, 512} and any(t["idle"] == 63 for t in ts) and any(t["idle"] == 1 for t in ts)
        assert {(t["unroll"], t["tail"]) for t in ts} == {(True, False), (False, True), (True, True)}
        assert {t["chunks"] > 1 for t in ts} == {False, True} and {1, 5} <= {t["last_rows"] for t in ts if t["chunks"] > 1}
        assert any(t["group_laps"] >= 2 for t in ts) and any(c.G > t["nthr"] for c, t in zip(cs, ts))
        assert any(c.S == 1025 and t["rpb"] == 128 for c, t in zip(cs, ts))
        assert {1, 32} <= {c.G for c in cs} and any(c.G == c.C // 8 for c in cs) and any(c.G == c.C for c in cs)
        rpi = 32
        assert {c.rps for c in cs if c.C == 64 and c.G == 32 and c.S == 3} >= {1, rpi - 1, rpi, 4 * rpi - 1, 4 * rpi, 4 * rpi + 1, 7 * rpi + 3}
        assert {c.kind for c in cs} == {"int", "gauss", "one"} and {c.ms for c in cs if c.kind == "gauss"} == {0.0, 0.35, 8.0, 64.0}
        assert any(c.C == 4096 and 4 * (t["nthr"] * 16 + 2 * c.C) == 65536 for c, t in zip(cs, ts))      # exactly 64 KB of dynamic LDS


def test_gn_apply_coverage():
    for dt in N.DTS:
        cs = [c for c in N.by_op("gn_apply") if c.dt == dt]
        assert {c.C // c.G for c in cs} >= {1, 2, 4, 8, 10, 30, 60, 128} and {c.silu for c in cs} == {False, True} and {c.eps for c in cs} == {1e-5, 1e-6}
        assert {N.traits(c)["straddle"] for c in cs} == {False, True}
        assert any(c.chained for c in cs) and any(c.const_group is not None for c in cs)
    big = [N.traits(c) for c in BIG]
    assert len(big) == 1 and big[0]["laps"] == 2 and big[0]["blocks"] == 8192 and big[0]["chunks"] == 2099200


def test_gn_apply_cs_coverage():
    for dt in N.DTS:
        cs = [c for c in N.by_op("gn_apply_cs") if c.dt == dt]
        ts = [N.traits(c) for c in cs]
        assert {(c.C1, c.C2, c.G) for c in cs} == {(320, 0, 32), (8, 56, 32), (40, 24, 8), (1280, 640, 32), (1280, 1280, 32), (2048, 2048, 32)}
        assert {t["stat_samples"] for t in ts if t["path"] == "cs"} == {1, 2, 5, 16, 64} and {c.ms for c in cs} == {0.35, 8.0, 64.0}
        assert {t["nthr"] for t in ts} == {256, 320, 512} and {(t["unroll"], t["tail"]) for t in ts} == {(True, False), (False, True), (True, True)}
        assert any(t["straddle"] for t in ts) and any(set(t["source"]) == {1, 2} for t in ts) and {t["chunks"] > 1 for t in ts} == {False, True}
        folds = [f for t in ts if t["path"] == "parts" for f in t["fold"]]
        assert {f["slots"] for f in folds} == {1, 2, 3, 4} and {f["fast"] for f in folds} == {False, True}
        assert {f["tiles"] for f in folds if f["fast"]} >= {1, 3, 4, 5, 8}
        assert {f["unroll_tiles"] > 0 for f in folds if f["fast"]} == {False, True} and {f["tail_tiles"] for f in folds if f["fast"]} >= {0, 1, 3}
        assert any(f["partial_last_tile"] and not f["fast"] for f in folds)
        have = {(bm, c.pcs) for c in cs if c.path == "parts" for bm in (c.bm1, c.bm2)}
        want = {(bm, r) for bm in N.BMS for r in N.PARTS_CS_ROWS if 1 <= N.slots_of(bm, r) <= 4}
        assert want <= have, sorted(want - have)
        assert any(c.bm1 != c.bm2 for c in cs if c.path == "parts")


def test_chan_stats_reduce_coverage():
    cs = N.by_op("chan_stats_reduce")
    ts = [N.traits(c) for c in cs]
    assert {c.N for c in cs} == {8, 32, 40, 320} and {t["tiles"] for t in ts} >= {1, 7, 8, 9, 17} and {t["slots"] for t in ts} == {1, 2, 3, 4}
    assert {c.out_mult for c in cs} == {0, 1, 2} and any(t["partial_last_tile"] for t in ts)


def test_layernorm_coverage():
    for op in ("layernorm", "row_stats"):
        assert {(N.traits(c)["maxch"], c.dt) for c in N.by_op(op)} == {(m, dt) for m in (3, 5, 10, 16) for dt in N.DTS}
        for dt in N.DTS:
            cs = [c for c in N.by_op(op) if c.dt == dt]
            assert {c.C for c in cs} == set(N.LN_C) and {c.rows for c in cs} == set(N.LN_ROWS) and {c.ms for c in cs} == {0.0, 0.33, 32.0}
            assert any(N.traits(c)["idle_lanes"] for c in cs) and {N.traits(c)["partial_block"] for c in cs} == {False, True}
            assert any(N.traits(c)["need"] == N.traits(c)["maxch"] for c in cs) and any(c.const_row is not None for c in cs)
            if op == "layernorm":
                assert {c.pe if c.pe is None or c.pe[0] <= c.rows else "beyond" for c in cs} >= {None, (1, 1), (3, 5), (16, 2), "beyond"}


def test_softmax_coverage():
    for dt in N.DTS:
        cs = [c for c in N.by_op("softmax_rows") if c.dt == dt]
        ts = [N.traits(c) for c in cs]
        assert {c.cols for c in cs} >= {1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 4096} and {c.rows for c in cs} >= {1, 3}
        assert {t["laps"] for t in ts} >= {1, 2, 3, 4, 16} and any(t["idle_waves"] == 3 for t in ts)
        assert {c.ld - c.cols for c in cs} == {0, 8} and {c.kind for c in cs} == {"gauss", "offset+", "offset-", "equal", "spike"}
        assert any(c.causal == c.cols and c.rows == 2 * c.causal for c in cs) and any(0 < c.causal < c.cols for c in cs)
        assert any(c.causal and t["laps"] >= 2 for c, t in zip(cs, ts))


# ---- the model stays inside the bound ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SMALL, ids=N.case_ids(SMALL))
def test_model_inside_bound(case):
    ops = problem(case)[0]
    judge(case, N.model(case, ops))
    if case.op in ("gn_apply", "gn_apply_cs", "layernorm"):      # the library is built with -ffp-contract=off; a fused a * g + b has one rounding less and stays inside too
        judge(case, N.model(case, ops, contract=True))
    if case.op == "gn_apply" and case.chained:      # the statistics the stats model gives, through the apply model
        judge(case, N.model(case, ops, stats=N.model(ops.stats_case, N.operands(ops.stats_case))))


def test_model_inside_bound_second_lap():
    """the 16.8 M-element case of gn_apply, outside the cache of the small ones"""
    (case,) = BIG
    ops = N.operands(case)
    ref, bound = N.reference(case, ops)
    got = N.model(case, ops)
    d = (got.double() - N.window(ref, *ops.win).double()).abs()
    assert torch.isfinite(d).all() and bool((d <= bound).all()), f"{int((d > bound).sum())} elements outside, worst {float((d / bound).max()):.3f} x"


# ---- planted defects --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", ["drop_last_chunk", "drop_tail"])
@pytest.mark.parametrize("kind", ["int", "gauss"])
def test_gn_stats_defects(defect, kind):
    c = pick("gn_stats", "bf16", C=320, G=32, rps=389, S=2, kind=kind, ms=0.0)
    rejected(c, N.model(c, problem(c)[0], defect=defect))


@pytest.mark.parametrize("dt", N.DTS)
@pytest.mark.parametrize("defect", ["neighbour_mean", "no_eps", "gamma_chunk"])
def test_gn_apply_defects(dt, defect):
    c = pick("gn_apply", dt, C=320, const_group=3, silu=False) if defect == "no_eps" else pick("gn_apply", dt, C=320, silu=False, const_group=None)
    rejected(c, N.model(c, problem(c)[0], defect=defect))


@pytest.mark.parametrize("dt", N.DTS)
@pytest.mark.parametrize("defect", ["c1_chunk", "slot", "last_tile"])
def test_gn_apply_cs_defects(dt, defect):
    """c1_chunk: the first chunk past C1 read one chunk off; slot: slot sl taken for sample first + sl + 1 (on the last tile that is the NaN of a sample that does not exist);
    last_tile: the tile range clamped with rows / tile_rows tiles, which loses the partial last tile"""
    c = pick("gn_apply_cs", dt, path="cs", C1=40, rps=127) if defect == "c1_chunk" else pick("gn_apply_cs", dt, path="parts", pcs=80)
    assert defect == "c1_chunk" or N.traits(c)["fold"][0]["partial_last_tile"]
    rejected(c, N.model(c, problem(c)[0], defect=defect))


@pytest.mark.parametrize("defect", ["slot", "last_tile"])
def test_chan_stats_reduce_defects(defect):
    c = pick("chan_stats_reduce", bm=128, cs_rows=80)
    rejected(c, N.model(c, problem(c)[0], defect=defect))


@pytest.mark.parametrize("dt", N.DTS)
def test_fold_and_reduce_agree(dt):
    """what gn_apply_cs folds from the partials is what chan_stats_reduce would hand it, on every parts layout"""
    for c in [c for c in N.by_op("gn_apply_cs") if c.dt == dt and c.path == "parts"]:
        ops = problem(c)[0]
        for i, x in enumerate(ops.xs):
            xd = x.double().view(c.S, c.rps, -1)
            direct = torch.stack([xd.sum(1), (xd * xd).sum(1)], dim=-1)
            for o in range(c.S):
                acc, mag, n = N.fold(ops.parts[i], ops.bms[i], c.pcs, c.S * c.rps, o, c.rps // c.pcs)
                assert bool(((acc - direct[o]).abs() <= (n + 1) * 2.0 ** -24 * mag).all()), (c.name, i, o)      # the partials are sums rounded to f32


@pytest.mark.parametrize("dt", N.DTS)
@pytest.mark.parametrize("op", ["layernorm", "row_stats"])
def test_layernorm_defects(dt, op):
    c = pick(op, dt, C=1280)      # need = MAXCH = 10
    rejected(c, N.model(c, problem(c)[0], defect="drop_chunk"))
    if op == "layernorm":
        c = pick(op, dt, pe=(3, 5), const_row=None)
        rejected(c, N.model(c, problem(c)[0], defect="pe_index"))


@pytest.mark.parametrize("dt", N.DTS)
def test_softmax_defects(dt):
    c = pick("softmax_rows", dt, cols=513, kind="spike")
    rejected(c, N.model(c, problem(c)[0], defect="skip_laps"))
    for c in (pick("softmax_rows", dt, causal=5), pick("softmax_rows", dt, causal=3)):
        rejected(c, N.model(c, problem(c)[0], defect="causal_width"))


@pytest.mark.parametrize("op,kw", [("gn_apply", dict(C=320, silu=False, const_group=None, chained=False)), ("gn_apply_cs", dict(path="cs", C1=320, rps=25)), ("layernorm", dict(C=320, ms=0.33)),
                                   ("softmax_rows", dict(cols=255))])
def test_one_element_two_ulp_off(op, kw):
    """... and the global relative L2 of the existing tests lets it pass"""
    c = pick(op, "bf16", **kw)
    ops, ref, _ = problem(c)
    got = N.window(ref, *ops.win).clone()
    i, j = got.shape[0] // 2, got.shape[1] // 3
    got[i, j] = (got[i, j].double() + 2 * ulp(got[i, j].double(), "bf16")).to(got.dtype)
    rejected(c, got)
    close(got, N.window(ref, *ops.win), c.name, N.rtol(c))


def test_global_l2_passes_a_1e4_error_of_every_sum():
    """the stated reason for the per-entry bound: {sum, sum sq} judged as one vector at 1e-5 does not see the sums"""
    c = pick("gn_stats", "f32", C=320, G=32, rps=389, S=2, kind="gauss", ms=0.0)
    ops, ref, _ = problem(c)
    got = N.window(ref, *ops.win).clone()
    got[:, 0] *= 1 + 1e-4
    close(got, N.window(ref, *ops.win), c.name, 1e-5)
    rejected(c, got)


def test_synthetic_partials():
    """build_parts: the sums of a tile's rows per sample slot, 0 for a sample without a row in the tile, NaN for a sample that does not exist"""
    x = torch.ones(1040, 8)
    p = N.build_parts(x, 128, 80, N.slots_of(128, 80))
    assert p.shape == (9, 3, 8, 2) and p[0, :, 0, 0].tolist() == [80.0, 48.0, 0.0] and p[1, :, 0, 0].tolist() == [32.0, 80.0, 16.0]
    assert p[8, 0, 0, 0].item() == 16.0 and torch.isnan(p[8, 1:]).all() and not torch.isnan(p[:7]).any() and torch.isnan(p[7, 2]).all()
