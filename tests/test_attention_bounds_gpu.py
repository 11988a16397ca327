"""fyc_attention and fyc_temporal_attention on the cases of tests/attention_cases.py (what each case launches and that the list reaches every built
instantiation is proven on the CPU by tests/test_attention_cases.py).  Every case is one launch into an output that lies inside a larger, prefilled
buffer - 64 elements in front; two rows and the pad columns [H d, ldo) behind for the flash kernel, one row block for the temporal one - compared
with the plain f64 reference (no rounding of P) by kernel_compare.compare: finite, global relative L2 at the tolerance of the existing test of the
same op, EVERY element within the bound derived from the kernel's rounding points (tests/kernel_compare.py), nothing outside the output touched.  The
selection cases must return v[pi(query)] bit for bit.

FYC_ATTENTION_FIGURES=<file>: append the figures of every comparison to that file (profiles/attention_bound_coverage.txt was made from it)."""
import os

import pytest
import torch

import attention_cases as A
from kernel_compare import Guard, compare
from test_kernels_gpu import hip  # noqa: F401  (the module-scoped library fixture)

pytestmark = pytest.mark.gpu

FIGURES = os.environ.get("FYC_ATTENTION_FIGURES")
_ref_cache = {}


def reference(c):
    """operands, reference buffer and bound of a case's PROBLEM: computed once and shared by its cases (the QT variants), never modified"""
    if c.problem not in _ref_cache:
        ops = A.operands(c)
        _ref_cache[c.problem] = (ops,) + (tuple(A.reference(c, ops)[:2]) if c.recipe != "select" or c.dt == "f32" else (None, None))
    return _ref_cache[c.problem]


def launch(hip, c, ops):  # noqa: F811
    """one launch of the case into a fresh copy of its guarded buffer; returns that buffer (CPU)"""
    buf = ops.buf.cuda()
    o = A.out_view(c, buf)
    if c.kind == "temporal":
        extra = dict(rope=tuple(t.cuda() for t in ops.tables)) if c.rope else {}
        hip.temporal_attention(ops.qkv.cuda(), o, clips=c.clips, frames=c.F, pixels=c.P, heads=c.H, d=c.d, scale=c.scale, **extra)
        torch.cuda.synchronize()
        return buf.cpu()
    hip.set_tuning(A.TUNE_ATTN_VARIANT, c.qt)
    try:
        hip.attention(ops.q.cuda(), ops.k.cuda(), ops.vt.cuda(), o, batch=c.B, heads=c.H, n_q=c.n_q, n_k=c.n_k, d=c.d, ldo=c.ldo, ldvt=c.ldvt, scale=c.scale,
                      kv_batch_div=c.div, q_batch_mod=c.mod, accumulate=c.accumulate, o_scale=c.o_scale)
        torch.cuda.synchronize()
    finally:
        hip.set_tuning(A.TUNE_ATTN_VARIANT, 0)
    return buf.cpu()


def record(c, fig, note=""):
    if FIGURES:
        with open(FIGURES, "a") as f:
            f.write(f"{c.kind} {c.group} {c.dt} {c.name} {fig['global_rel']:.3e} {fig['elem_ratio']:.4f}{note}\n")


def _run(hip, c):  # noqa: F811
    ops, ref, bound = reference(c)
    got = launch(hip, c, ops)
    fig = compare(A.window(c, got), A.window(c, ref), dtype=c.dt, bound=bound, rtol=c.rtol, labels=A.labels(c), guard=Guard(ops.buf, got, ops.mask), tag=c.name)
    print(f"{c.name}: global rel-L2 {fig['global_rel']:.3e} (tolerance {c.rtol:.1e}), worst element at {fig['elem_ratio']:.3f} of its bound")
    record(c, fig)


def _run_selection(hip, c):  # noqa: F811
    ops, ref, bound = reference(c)
    got = launch(hip, c, ops)
    want = A.selected(c, ops).contiguous()
    if c.dt == "f32":      # the f32 kernel's weights on the other frames are below 2^-64, not zero: the element bound instead of the bits
        assert torch.equal(A.window(c, ref), want)
        fig = compare(A.window(c, got), A.window(c, ref), dtype=c.dt, bound=bound, rtol=c.rtol, labels=A.labels(c), guard=Guard(ops.buf, got, ops.mask), tag=c.name)
        record(c, fig)
        return
    out = A.window(c, got).contiguous()
    wrong = (out.view(torch.int16) != want.view(torch.int16)).nonzero()
    if wrong.numel():
        i, j = wrong[0].tolist()
        lab = A.labels(c)
        raise AssertionError(f"{c.name}: {wrong.shape[0]} of {out.numel()} elements are not the selected value bit for bit; first: got {out[i, j].item()!r}, "
                             f"want {want[i, j].item()!r} at row {i} ({lab.row(i)}), column {j} ({lab.col(j)})")
    fig = compare(out, want, dtype=c.dt, bound=torch.full(out.shape, 2.0 ** -200, dtype=torch.float64), rtol=0.0, labels=A.labels(c),
                  guard=Guard(ops.buf, got, ops.mask), tag=c.name)      # equal: what is left to check is the guard
    record(c, fig, " exact")


HEAD_DIMS, TAILS, BATCH, SCORES = (A.by_group("flash", g) for g in "ABCD")
SELECT = A.by_group("flash", "E") + A.by_group("temporal", "E")
TEMPORAL = A.by_group("temporal", "F")


@pytest.mark.parametrize("case", HEAD_DIMS, ids=A.case_ids(HEAD_DIMS))
def test_every_head_dim_and_query_tiling(hip, case):  # noqa: F811
    """A: d = 8 .. 160, QT = 2, 3, 4 where the dispatch honours it; B H = 6 (no XCD mapping), 150 / 270 queries (ragged query blocks), 97 keys (one full tile,
    then a tail whose second block holds one key), ldo = H d + 8, ldvt = 104 with pad keys of the largest finite magnitude"""
    _run(hip, case)


@pytest.mark.parametrize("case", TAILS, ids=A.case_ids(TAILS))
def test_key_tails_at_the_block_edges(hip, case):  # noqa: F811
    """B: n_k at and around every 32-key block edge, with queries that put a weight of 0.2 .. 0.5 on the keys a tail mask one key off would lose"""
    _run(hip, case)


@pytest.mark.parametrize("case", BATCH, ids=A.case_ids(BATCH))
def test_batch_indexing_and_accumulation(hip, case):  # noqa: F811
    """C: kv_batch_div that does not divide the batch, q_batch_mod with kv_batch_div under the XCD mapping, o_accumulate with o_scale 0.7 and -1.5"""
    _run(hip, case)


@pytest.mark.parametrize("case", SCORES, ids=A.case_ids(SCORES))
def test_score_offsets_spikes_and_creeping_maximum(hip, case):  # noqa: F811
    """D: scores +-(90 .. 120) log2 units from 0, a late and an early spike per lane quad, a slowly creeping maximum: every row judged on its own"""
    _run(hip, case)


@pytest.mark.parametrize("case", SELECT, ids=A.case_ids(SELECT))
def test_selection_is_exact(hip, case):  # noqa: F811
    """E: every query's weight on all keys but one is below 2^-64: the output is that key's value row, bit for bit"""
    _run_selection(hip, case)


@pytest.mark.parametrize("case", TEMPORAL, ids=A.case_ids(TEMPORAL))
def test_temporal_attention_every_family(hip, case):  # noqa: F811
    """F: every (DP, DVT) family of launch_d and its padded members, NFT = 1 .. 4, LAZY or not, RoPE off and on, task counts that do not fill the last block"""
    _run(hip, case)
