"""The attention cases of tests/attention_cases.py without a GPU: the list reaches every instantiation the library builds and every compile-time
path that traits() restates; a torch model of each kernel's rounding points stays inside kernel_compare.compare() with the derived per-element bound
(the bound admits the design) and every defect a case declares leaves it (the bound rejects what it is there to catch); the selection cases select."""
import functools

import pytest
import torch

import attention_cases as A
from kernel_compare import Guard, compare

PLACEMENTS = (0.0, 3.0, 6.0)      # of the running max below the row's maximum: the two ends and the middle of the RESCALE_THR window
FLASH_DEFECTS = ("drop_heaviest", "drop_last_key", "pad_key", "swap_rows", "shift_head", "ignore_div", "ignore_mod", "scale_prev", "freeze_max")
TEMPORAL_DEFECTS = ("mask_last", "rope_sign", "rope_next_q")


def _problems(cases):
    seen = {}
    for c in cases:
        seen.setdefault(c.problem, c)
    return list(seen.values())


BOUNDED = _problems([c for c in A.CASES if c.recipe != "select"])
SELECT = _problems([c for c in A.CASES if c.recipe == "select"])


@functools.lru_cache(maxsize=None)
def problem(p):
    ops = A.operands(p)
    return (ops,) + tuple(A.reference(p, ops))


def judge(c, ops, got, ref, bound):
    buf = ops.buf.clone()
    A.window(c, buf).copy_(got)
    return compare(A.window(c, buf), A.window(c, ref), dtype=c.dt, bound=bound, rtol=c.rtol, labels=A.labels(c), guard=Guard(ops.buf, buf, ops.mask), tag=c.name)


# ---- coverage -----------------------------------------------------------------------------------------------------------------------
def test_flash_cases_reach_every_built_instantiation():
    have = {(c.dt, c.d, A.traits(c)["qt"]) for c in A.FLASH_CASES}
    assert have == A.built_flash(), (sorted(A.built_flash() - have), sorted(have - A.built_flash()))
    for c in A.FLASH_CASES:      # a case that names a QT runs it
        assert not c.qt or A.traits(c)["qt"] == c.qt, c.name


def test_temporal_cases_reach_every_built_instantiation():
    have = {(c.dt, t["family"], t["nft"], t["rope"]) for c in A.TEMPORAL_CASES for t in [A.ttraits(c)]}
    assert have == A.built_temporal(), (sorted(map(str, A.built_temporal() - have)), sorted(map(str, have - A.built_temporal())))
    for dt in ("bf16", "f16"):
        mine = [A.ttraits(c) for c in A.TEMPORAL_CASES if c.dt == dt]
        assert {t["family"] for t in mine} == {f[1:] for f in A.FAMILIES} and {t["padded"] for t in mine} == {False, True}
        assert {(t["nft"], t["lazy"]) for t in mine} == {(1, False), (2, False), (2, True), (3, True), (4, True)}
        assert {t["ragged_grid"] for t in mine} == {False, True}
    assert {c.d for c in A.by_group("temporal", "F")} == set(A.TEMPORAL_D) and {c.F for c in A.by_group("temporal", "F")} == {1, 2, 15, 16, 17, 32, 33, 48, 49, 64}
    assert {c.P for c in A.by_group("temporal", "F")} == {1, 5} and {c.H for c in A.by_group("temporal", "F")} == {1, 3, 8}


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_flash_cases_reach_every_trait_value(dt):
    ts = [A.traits(c) for c in A.FLASH_CASES if c.dt == dt]
    def values(name, f=lambda x: x):
        return {f(t[name]) for t in ts}
    assert values("group") == {"small", "medium", "large"}
    assert values("ks") == {0, 1, 2, 3, 4, 5} and values("qt") == {2, 3, 4}
    for name in ("tail", "msub", "pipe", "kxor", "offs_in_lds", "ragged_tile", "xcd"):
        assert values(name) == {False, True}, name
    assert {(t["ks"] > 0, t["tail"]) for t in ts} == {(False, True), (True, False), (True, True)}      # a 16-wide step alone, 32-wide steps alone, both
    assert values("full_tiles") >= {0, 1, 2, 3, 4} and values("steady_tiles") >= {0, 1, 2}
    assert values("last_tile_blocks") == {1, 2} and values("query_blocks", lambda n: min(n, 2)) == {1, 2}
    assert {(t["msub"], t["pipe"]) for t in ts} == {(False, False), (False, True), (True, False), (True, True)}
    # more than one query block for every QT, ragged in each (group A), and under the XCD mapping (group C)
    for d in range(8, 161, 8):
        for qt in (2, 3, 4) if d <= 80 else (2,):
            assert any(t["qt"] == qt and t["query_blocks"] >= 2 and c.n_q % (64 * qt) and c.n_q % 16 and not t["xcd"]
                       for c in A.by_group("flash", "A") if c.dt == dt and c.d == d for t in [A.traits(c)]), (d, qt)
    assert any(A.traits(c)["xcd"] and A.traits(c)["query_blocks"] >= 2 and c.mod and c.div > 1 for c in A.by_group("flash", "C") if c.dt == dt)
    assert all(c.B * c.H <= 32 and c.n_q <= 270 and c.n_k <= 330 for c in A.FLASH_CASES)
    assert {c.n_k for c in A.by_group("flash", "B")} == set(A.TAIL_NK) and all(A.traits(c)["xcd"] for c in A.by_group("flash", "B"))


@pytest.mark.parametrize("kind,names", [("flash", FLASH_DEFECTS), ("temporal", TEMPORAL_DEFECTS)])
def test_every_defect_is_declared_by_a_case_of_each_type(kind, names):
    for dt in ("bf16", "f16") + (("f32",) if kind == "temporal" else ()):
        declared = {x for c in A.CASES if c.kind == kind and c.dt == dt for x in c.defects}
        assert declared == set(names), (dt, set(names) ^ declared)
    for c in A.CASES:
        assert not set(c.defects) & {n for n, _ in c.unchanged} and all(reason for _, reason in c.unchanged), c.name
    assert all("drop_last_key" in c.defects for c in A.by_group("flash", "B"))


# ---- the bound admits the design, and rejects the defects ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", BOUNDED, ids=A.case_ids(BOUNDED))
def test_model_of_the_rounding_points_stays_within_the_bound(case):
    ops, ref, bound, _ = problem(case.problem)
    for pl in PLACEMENTS if case.kind == "flash" else (0.0,):
        fig = judge(case, ops, A.model(case, ops, pl), ref, bound)
        assert fig["elem_ratio"] <= 1.0


@pytest.mark.parametrize("case", BOUNDED, ids=A.case_ids(BOUNDED))
def test_declared_defects_leave_the_bound(case):
    ops, ref, bound, _ = problem(case.problem)
    clean = A.model(case, ops)
    for name in case.defects:
        bad = A.model(case, ops, defect=name)
        assert not torch.equal(bad.view(torch.int16 if case.dt != "f32" else torch.int32), clean.view(torch.int16 if case.dt != "f32" else torch.int32)), name
        with pytest.raises(AssertionError):
            judge(case, ops, bad, ref, bound)
    for name, _ in case.unchanged:      # the claim "cannot change this case" is checked, not believed
        judge(case, ops, A.model(case, ops, defect=name), ref, bound)


def test_a_write_outside_the_output_is_caught():
    for case in (A.by_group("flash", "A")[0], A.by_group("temporal", "F")[0]):
        ops, ref, bound, _ = problem(case.problem)
        good = A.model(case, ops)
        for where in (A.FRONT - 1, ops.buf.numel() - 1) + ((A.FRONT + case.cols,) if case.kind == "flash" else ()):      # in front, behind, a pad column
            buf = ops.buf.clone()
            A.window(case, buf).copy_(good)
            buf[where] = 1.0
            with pytest.raises(AssertionError, match="outside the output"):
                compare(A.window(case, buf), A.window(case, ref), dtype=case.dt, bound=bound, rtol=case.rtol, labels=A.labels(case), guard=Guard(ops.buf, buf, ops.mask), tag=case.name)


TAILS = _problems(A.by_group("flash", "B"))


@pytest.mark.parametrize("case", TAILS, ids=A.case_ids(TAILS))
def test_designated_queries_weigh_the_keys_a_tail_mask_can_lose(case):
    ops, _, _, w = problem(case.problem)
    if case.n_k < 3:
        assert not ops.designated      # a single key: its weight is 1, and losing it leaves nothing finite
        return
    keys = {j for _, j in ops.designated}
    assert keys == {case.n_k - 1, case.n_k - 2, (case.n_k - 1) // 32 * 32, (case.n_k - 1) // 64 * 64}
    for r, j in ops.designated:
        assert ((w[0, :, r, j] >= 0.2) & (w[0, :, r, j] <= 0.5)).all(), (r, j, w[0, :, r, j])


# ---- selection ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SELECT, ids=A.case_ids(SELECT))
def test_selection_preconditions(case):
    """on the rounded operands, in f64: every query's weight on every key but pi(query) is below 2^-64, pi is a permutation that differs per (batch, head) and
    reaches every tile, both 32-key blocks, all four lane quads and the ragged tail; 0.5 <= |v| < 2; and the model of the rounding points selects bit for bit"""
    ops = A.operands(case)
    if case.kind == "flash":
        q = torch.stack([ops.q_full[A.q_of(case, b)] for b in range(case.B)]).double()
        k = torch.stack([ops.k[A.kv_of(case, b)] for b in range(case.B)]).double()
        v, n = ops.vt[..., : case.n_k], case.n_k
    else:
        q, k, v = (t.double() for t in A._split(case, ops))
        n = case.F
    w = torch.softmax(q @ k.transpose(-1, -2) * case.scale, dim=-1)
    pi = ops.pi
    assert torch.equal(torch.sort(pi, dim=-1).values, torch.arange(n).expand_as(pi)), "pi is not a permutation"
    flat = pi.reshape(-1, n)
    assert len({tuple(r.tolist()) for r in flat}) == flat.shape[0], "the same permutation twice"
    if n >= 16:
        assert (flat != torch.arange(n)).any(dim=-1).all()
    assert torch.gather(w, -1, pi[..., None]).min().item() > 0.5
    others = w.scatter(-1, pi[..., None], 0.0)
    assert others.max().item() < 2.0 ** -64, others.max().item()
    assert (v.abs() >= 0.5).all() and (v.abs() < 2).all()
    want = A.selected(case, ops)
    bits = torch.int32 if case.dt == "f32" else torch.int16
    if case.dt != "f32":
        for pl in PLACEMENTS if case.kind == "flash" else (0.0,):
            assert torch.equal(A.model(case, ops, pl).view(bits), want.view(bits))
    else:
        ref, bound, _ = A.reference(case, ops)
        judge(case, ops, A.model(case, ops), ref, bound)
        assert torch.equal(A.window(case, ref).view(bits), want.contiguous().view(bits))
