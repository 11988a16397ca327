"""fyc_temporal_attention's split-bf16 product rule for f32 tensors (include/fyc.h: fyc_tattn_args.f32_products = FYC_PRODUCTS_SPLIT_BF16;
HipOps.temporal_attention(products="split")) on the GPU: the cases, their f64 references and the bound are tests/tattn_split_spec.py's, the guarded
buffers tests/attention_cases.py's.  Every case is one launch into an output inside a larger prefilled buffer, judged by kernel_compare.compare: finite, global
relative L2 at the exact f32 kernel's tolerance, EVERY element within the derived bound, nothing outside the output touched.

Every test asks for the rule per call, or sets the mode of the shared HipOps and puts it back in a `finally`: the session's engines must not see it.

FYC_TATTN_SPLIT_FIGURES=<file>: append the figures of every comparison to that file (profiles/f32x3_tattn_bound_coverage.txt was made from it)."""
import os
from dataclasses import replace

import pytest
import torch

import attention_cases as A
import tattn_split_spec as S
from kernel_compare import Guard, compare
from test_kernels_gpu import hip  # noqa: F401  (the module-scoped library fixture)

pytestmark = pytest.mark.gpu

FIGURES = os.environ.get("FYC_TATTN_SPLIT_FIGURES")


def launch(hip, c, ops, qkv=None, **kw):  # noqa: F811
    """one launch of the case into a fresh copy of its guarded buffer; returns that buffer (CPU).  kw: products=, or nothing for the instance's default"""
    buf = ops.buf.cuda()
    extra = dict(rope=tuple(t.cuda() for t in ops.tables)) if c.rope else {}
    hip.temporal_attention((ops.qkv if qkv is None else qkv).cuda(), A.out_view(c, buf), clips=c.clips, frames=c.F, pixels=c.P, heads=c.H, d=c.d, scale=c.scale, **extra, **kw)
    torch.cuda.synchronize()
    return buf.cpu()


def bits(c, buf):
    return A.window(c, buf).contiguous().view(torch.int16 if buf.element_size() == 2 else torch.int32)


def judge(c, got):
    ops, ref, bound = S.reference(c)
    fig = compare(A.window(c, got), A.window(c, ref), dtype="f32", bound=bound, rtol=c.rtol, labels=A.labels(c), guard=Guard(ops.buf, got, ops.mask), tag=c.name)
    print(f"{c.name}: global rel-L2 {fig['global_rel']:.3e} (tolerance {c.rtol:.1e}), worst element at {fig['elem_ratio']:.3f} of its bound")
    if FIGURES:
        with open(FIGURES, "a") as f:
            f.write(f"temporal {c.group} f32split {c.name} {fig['global_rel']:.3e} {fig['elem_ratio']:.4f}\n")


FAMILY = S.FAMILY_CASES + S.TWO_TASK_CASES


@pytest.mark.parametrize("case", FAMILY, ids=A.case_ids(FAMILY))
def test_every_family_inside_the_bound(hip, case):  # noqa: F811
    """1: every (DP, DVT) family and its padded members, NFT = 1 .. 4, RoPE off and on, task counts that do not fill the last block (of four tasks, and of two
    for DP 160 / NFT 4)"""
    judge(case, launch(hip, case, S.reference(case)[0], products="split"))


def _one_frame_cases():
    """the single-frame cases of the list, and one more per (DP, DVT) family"""
    out = [c for c in S.FAMILY_CASES if c.F == 1]
    for (_, dp, dvt), d in zip(A.FAMILIES, (24, 40, 64, 72, 96, 128, 160)):
        c = next(c for c in S.FAMILY_CASES if c.d == d and c.F > 1 and not c.rope)
        assert A.ttraits(replace(c, dt="bf16"))["family"] == (dp, dvt)
        out.append(replace(c, F=1, name=f"one-frame-d{d}-P{c.P}-H{c.H}-c{c.clips}"))
    return out


ONE_FRAME = _one_frame_cases()


@pytest.mark.parametrize("case", ONE_FRAME, ids=A.case_ids(ONE_FRAME))
def test_split_is_taken_and_is_the_specified_one(hip, case):  # noqa: F811
    """2: with one frame p = 1 = hi(p) and the accumulator receives lo(v) 1 + hi(v) 0 + hi(v) 1: the split rule returns hi(v) + lo(v) BIT FOR BIT, which is not v for
    values with more than 16 significant bits; the exact kernel returns v.  The bound cannot tell the rules apart (exact products pass it too); this does"""
    c = case
    ops = A.operands(c)
    want, v = S.hi_plus_lo_of_v(c, ops)
    got = A.window(c, launch(hip, c, ops, products="split"))
    assert torch.equal(got.contiguous().view(torch.int32), want.view(torch.int32)), f"{(got != want).sum().item()} of {got.numel()} elements are not hi(v) + lo(v)"
    assert (got != v).float().mean().item() >= 0.5, "the output is v itself: the products were exact"
    exact = A.window(c, launch(hip, c, ops, products="exact"))
    assert torch.equal(exact.contiguous().view(torch.int32), v.contiguous().view(torch.int32))


@pytest.mark.parametrize("case", S.SELECT_CASES, ids=A.case_ids(S.SELECT_CASES))
def test_selection_inside_the_bound(hip, case):  # noqa: F811
    """3: every query frame's weight on all frames but one is below 2^-64, scores 80 log2 units apart: the selected row comes out as hi(v) + lo(v), inside the bound"""
    c = case
    ops, ref, _ = S.reference(c)
    assert torch.equal(A.window(c, ref), A.selected(c, ops).contiguous())
    judge(c, launch(hip, c, ops, products="split"))


OFF_CASES = [A.Temporal("off-d40-F16", "O", "f32", 2, 16, 5, 3, 40, False, 2e-5), A.Temporal("off-d80-F17-rope", "O", "f32", 2, 17, 5, 3, 80, True, 2e-5),
             A.Temporal("off-d160-F33", "O", "f32", 1, 33, 3, 3, 160, False, 2e-5)]


@pytest.mark.parametrize("case", OFF_CASES, ids=A.case_ids(OFF_CASES))
def test_off_is_off(hip, case):  # noqa: F811
    """4: the default call, products="exact", and an instance whose mode is "split" called with products="exact" launch the same kernel: the same bits"""
    c = case
    ops = A.operands(c)
    before = hip.f32_products
    hip.set_f32_products("exact")
    try:
        default = launch(hip, c, ops)
        explicit = launch(hip, c, ops, products="exact")
        hip.set_f32_products("split")
        overridden = launch(hip, c, ops, products="exact")
        split = launch(hip, c, ops, products="split")
    finally:
        hip.set_f32_products(before)
    assert torch.equal(bits(c, default), bits(c, explicit)) and torch.equal(bits(c, default), bits(c, overridden))
    assert not torch.equal(bits(c, default), bits(c, split)), "the split rule gave the exact rule's bits"


def test_instance_default(hip):  # noqa: F811
    """5: after set_f32_products("split") a call without the keyword is the explicit "split" call; with bf16 tensors the same instance launches what the default
    instance launches"""
    c = OFF_CASES[1]
    ops = A.operands(c)
    c16 = replace(c, dt="bf16")
    ops16 = A.operands(c16)
    before = hip.f32_products
    hip.set_f32_products("exact")
    try:
        explicit = launch(hip, c, ops, products="split")
        plain16 = launch(hip, c16, ops16)
        hip.set_f32_products("split")
        default = launch(hip, c, ops)
        split16 = launch(hip, c16, ops16)
        with pytest.raises(TypeError, match="split"):
            launch(hip, c16, ops16, products="split")
    finally:
        hip.set_f32_products(before)
    assert torch.equal(bits(c, default), bits(c, explicit))
    assert torch.equal(bits(c16, plain16), bits(c16, split16))
    judge(c, default)


NONFINITE = [A.Temporal("nonfinite-d40-F17", "N", "f32", 2, 17, 3, 3, 40, False, 2e-5), A.Temporal("nonfinite-d160-F64", "N", "f32", 1, 64, 3, 3, 160, False, 2e-5)]


@pytest.mark.parametrize("case", NONFINITE, ids=A.case_ids(NONFINITE))
def test_non_finite_input_stays_in_its_task(hip, case):  # noqa: F811
    """6: an Inf in q, a NaN in k or an Inf in v of one (clip, pixel, head) task: every row and head column of every other task keeps the bits of the run without it"""
    c = case
    ops = A.operands(c)
    clean = launch(hip, c, ops, products="split")
    b, pix, h = c.clips - 1, 1, 1
    other = torch.ones(c.clips, c.F, c.P, c.H, c.d, dtype=torch.bool)
    other[b, :, pix, h] = False
    other = other.reshape(c.rows, c.cols)
    for which, value in ((0, float("inf")), (1, float("nan")), (2, float("-inf"))):
        qkv = ops.qkv.clone()
        qkv.view(c.clips, c.F, c.P, 3, c.H, c.d)[b, c.F - 2, pix, which, h, c.d - 3] = value
        got = launch(hip, c, ops, qkv=qkv, products="split")
        same = bits(c, got) == bits(c, clean)
        assert bool(same[other].all()), f"{c.name}: {int((~same & other).sum())} elements of other tasks changed with a non-finite value in {'qkv'[which]}"
        assert not bool(torch.isfinite(A.window(c, got)[~other]).all()), f"{c.name}: the task of the non-finite {'qkv'[which]} value came out finite"
        assert torch.equal(got.view(torch.int32)[~ops.mask], ops.buf.view(torch.int32)[~ops.mask])


def test_two_launches_give_the_same_bits(hip):  # noqa: F811
    """7"""
    c = next(c for c in S.FAMILY_CASES if c.d == 160 and c.F > 48 and c.rope)
    ops = S.reference(c)[0]
    assert torch.equal(bits(c, launch(hip, c, ops, products="split")), bits(c, launch(hip, c, ops, products="split")))
