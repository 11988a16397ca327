"""fyc_attention's split-bf16 product rule for f32 tensors (include/fyc.h: fyc_attn_args.f32_products = FYC_PRODUCTS_SPLIT_BF16; HipOps.attention(products="split"))
on the GPU: the cases, their f64 references and the bound are tests/attn_split_spec.py's, the guarded buffers tests/attention_cases.py's.  Every case is one launch
into an output inside a larger prefilled buffer, judged by kernel_compare.compare: finite, global relative L2 at the case's tolerance, EVERY element within the derived
bound, nothing outside the output touched.

Every test asks for the rule per call, or sets the mode of the shared HipOps and puts it back in a `finally`: the session's engines must not see it.

FYC_ATTN_SPLIT_FIGURES=<file>: append the figures of every comparison to that file (profiles/f32x3_attention_bound_coverage.txt was made from it)."""
import ctypes
import os
from dataclasses import replace

import pytest
import torch

import attention_cases as A
import attn_split_spec as S
from kernel_compare import Guard, compare
from test_kernels_gpu import hip  # noqa: F401  (the module-scoped library fixture)

pytestmark = pytest.mark.gpu

FIGURES = os.environ.get("FYC_ATTN_SPLIT_FIGURES")


def launch(hip, c, ops, q=None, **kw):  # noqa: F811
    """one launch of the case into a fresh copy of its guarded buffer; returns that buffer (CPU).  kw: products=, or nothing for the instance's default"""
    buf = ops.buf.cuda()
    hip.set_tuning(A.TUNE_ATTN_VARIANT, c.qt)
    try:
        hip.attention((ops.q if q is None else q).cuda(), ops.k.cuda(), ops.vt.cuda(), A.out_view(c, buf), batch=c.B, heads=c.H, n_q=c.n_q, n_k=c.n_k, d=c.d, ldo=c.ldo,
                      ldvt=c.ldvt, scale=c.scale, kv_batch_div=c.div, q_batch_mod=c.mod, accumulate=c.accumulate, o_scale=c.o_scale, **kw)
        torch.cuda.synchronize()
    finally:
        hip.set_tuning(A.TUNE_ATTN_VARIANT, 0)
    return buf.cpu()


def bits(c, buf):
    return A.window(c, buf).contiguous().view(torch.int16 if buf.element_size() == 2 else torch.int32)


def judge(c, got, note=""):
    ops, ref, bound = S.reference(c)
    print(f"{c.name}{note}: global rel-L2 {S.rel_l2(c, got, ref):.3e} (tolerance {c.rtol:.1e})")      # before anything is asserted
    fig = compare(A.window(c, got), A.window(c, ref), dtype="f32", bound=bound, rtol=c.rtol, labels=S.labels(c), guard=Guard(ops.buf, got, ops.mask), tag=c.name)
    print(f"{c.name}{note}: worst element at {fig['elem_ratio']:.3f} of its bound")
    if FIGURES:
        with open(FIGURES, "a") as f:
            f.write(f"flash {c.group} f32split {c.name}{note} {fig['global_rel']:.3e} {fig['elem_ratio']:.4f}\n")
    return fig


@pytest.mark.parametrize("case", S.CASES, ids=A.case_ids(S.CASES))
def test_every_case_inside_the_bound(hip, case):  # noqa: F811
    """1: groups A - E: every head dim at QT = 2 and (d <= 80) 4 with one ragged and two query blocks, key counts on both sides of every 32-key tile edge, batch
    indexing and accumulate, score offsets and spikes, selection"""
    c = case
    ops = S.reference(c)[0]
    judge(c, launch(hip, c, ops, products="split"))


ONE_KEY = [c for c in S.CASES if c.n_k == 1] + [replace(c, n_k=1, name=c.name + "-nk1", defects=()) for c in S.by_group("A")
                                                 if c.qt == (4 if c.d <= 80 else 2) and c.n_q == 150 and c.d in (8, 24, 72, 96, 104, 136)]


@pytest.mark.parametrize("case", ONE_KEY, ids=A.case_ids(ONE_KEY))
def test_one_key_returns_hi_plus_lo(hip, case):  # noqa: F811
    """2: with one key p = l = 1 and the accumulator receives lo(v) 1 + hi(v) 0 + hi(v) 1: the split rule returns hi(v) + lo(v) BIT FOR BIT, which is not v for values
    with more than 16 significant bits.  The bound cannot tell the rules apart (exact products pass it too); this does"""
    c = case
    ops = S.operands(c)
    want, v = S.hi_plus_lo_of_v(c, ops)
    got = A.window(c, launch(hip, c, ops, products="split"))
    assert torch.equal(got.contiguous().view(torch.int32), want.view(torch.int32)), f"{(got != want).sum().item()} of {got.numel()} elements are not hi(v) + lo(v)"
    assert (got != v).float().mean().item() >= 0.5, "the output is v itself: the products were exact"


def _raw_args(hip, c, ops, buf, dtype, products):  # noqa: F811
    from followyourclick_amd import _lib
    a = _lib.AttnArgs()
    a.q, a.k, a.vt, a.o = ops["q"].data_ptr(), ops["k"].data_ptr(), ops["vt"].data_ptr(), A.out_view(c, buf).data_ptr()
    a.batch, a.heads, a.n_q, a.n_k, a.d, a.ldo, a.ldvt = c.B, c.H, c.n_q, c.n_k, c.d, c.ldo, c.ldvt
    a.kv_batch_div, a.o_accumulate, a.scale, a.o_scale, a.dtype = 1, 0, c.scale, 1.0, dtype
    if products is not None:
        a.f32_products = products
    return a


REFUSED = S.by_group("C")[0]


def test_bad_combinations_are_refused_and_write_nothing(hip):  # noqa: F811
    """3: f32 + exact and bf16 + split: by the Python entry point before anything is launched, and by the library itself; the output buffer keeps its prefill"""
    from followyourclick_amd import _lib
    c = REFUSED
    ops = S.operands(c)
    c16 = replace(c, dt="bf16")
    ops16 = A.operands(c16)
    before = hip.f32_products
    hip.set_f32_products("exact")
    try:
        with pytest.raises(_lib.FycError, match="materialised"):
            launch(hip, c, ops)
        with pytest.raises(_lib.FycError, match="materialised"):
            launch(hip, c, ops, products="exact")
        with pytest.raises(TypeError, match="split"):
            launch(hip, c16, ops16, products="split")
    finally:
        hip.set_f32_products(before)
    for cc, oo, dtype, products in ((c, ops, _lib.FYC_F32, 0), (c16, ops16, _lib.FYC_BF16, 1), (c, ops, _lib.FYC_F32, 2)):
        buf = oo.buf.cuda()
        dev = dict(q=oo.q.cuda(), k=oo.k.cuda(), vt=oo.vt.cuda())
        a = _raw_args(hip, cc, dev, buf, dtype, products)
        assert hip.lib.fyc_attention(ctypes.byref(a), hip._stream()) != 0
        assert b"f32_products" in hip.lib.fyc_last_error()
        torch.cuda.synchronize()
        assert torch.equal(buf.cpu().view(torch.int16 if dtype else torch.int32), oo.buf.view(torch.int16 if dtype else torch.int32))


def test_bf16_call_with_the_field_never_written(hip):  # noqa: F811
    """4: a 16-bit call through a struct whose new field was never written (what a caller of the previous binding's fields passes, zero-initialised) gives the bits of
    products=None"""
    from followyourclick_amd import _lib
    c = replace(REFUSED, dt="bf16")
    ops = A.operands(c)
    want = launch(hip, c, ops)
    buf = ops.buf.cuda()
    dev = dict(q=ops.q.cuda(), k=ops.k.cuda(), vt=ops.vt.cuda())
    a = _raw_args(hip, c, dev, buf, _lib.FYC_BF16, None)
    assert a.f32_products == 0
    assert hip.lib.fyc_attention(ctypes.byref(a), hip._stream()) == 0, hip.lib.fyc_last_error()
    torch.cuda.synchronize()
    assert torch.equal(bits(c, buf.cpu()), bits(c, want))


def test_instance_default(hip):  # noqa: F811
    """5: after set_f32_products("split") a call without the keyword is the explicit "split" call; with bf16 tensors the same instance launches what the default
    instance launches"""
    c = REFUSED
    ops = S.reference(c)[0]
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
    finally:
        hip.set_f32_products(before)
    assert torch.equal(bits(c, default), bits(c, explicit))
    assert torch.equal(bits(c16, plain16), bits(c16, split16))
    judge(c, default, " (instance default)")


NONFINITE = [A.Flash("nonfinite-d40", "N", "f32", 2, 3, 150, 97, 40, 2e-5, ldvt=104), A.Flash("nonfinite-d160", "N", "f32", 2, 3, 70, 77, 160, 2e-5, ldvt=80)]


@pytest.mark.parametrize("case", NONFINITE, ids=A.case_ids(NONFINITE))
def test_non_finite_input_stays_in_its_head(hip, case):  # noqa: F811
    """6: an Inf in the q of one (batch, head): every row and head column of every other (batch, head) keeps the bits of the run without it"""
    c = case
    ops = S.operands(c)
    clean = launch(hip, c, ops, products="split")
    b, h = c.B - 1, 1
    other = torch.ones(c.B, c.n_q, c.H, c.d, dtype=torch.bool)
    other[b, :, h] = False
    other = other.reshape(c.rows, c.cols)
    q = ops.q.clone()
    q[b, h, c.n_q - 2, c.d - 3] = float("inf")
    got = launch(hip, c, ops, q=q, products="split")
    same = bits(c, got) == bits(c, clean)
    assert bool(same[other].all()), f"{c.name}: {int((~same & other).sum())} elements of other (batch, head)s changed with an Inf in q"
    assert not bool(torch.isfinite(A.window(c, got)[~other]).all()), f"{c.name}: the head of the Inf came out finite"
    assert torch.equal(got.view(torch.int32)[~ops.mask], ops.buf.view(torch.int32)[~ops.mask])


def test_two_launches_give_the_same_bits(hip):  # noqa: F811
    """7: no atomics, a fixed summation order"""
    c = next(c for c in S.by_group("A") if c.d == 80 and c.qt == 4 and c.n_q == 270)
    ops = S.reference(c)[0]
    assert torch.equal(bits(c, launch(hip, c, ops, products="split")), bits(c, launch(hip, c, ops, products="split")))


def _materialised(hip, c, ops):  # noqa: F811
    """engine/unet3d.py::_attend's materialised sequence on the case's operands with split products: zeros + score GEMM + row softmax + P V GEMM (+ axpy on the host)"""
    buf = ops.buf.cuda()
    out = A.out_view(c, buf)
    q, k, vt = ops.q.cuda(), ops.k.cuda(), ops.vt.cuda()
    H, n_q, n_k, d, C, ldvt = c.H, c.n_q, c.n_k, c.d, c.cols, c.ldvt
    ldS = (n_k + 7) // 8 * 8
    for b in range(c.B):
        kb = b // c.div
        Sm = torch.zeros(H, n_q, ldS, dtype=torch.float32, device="cuda")
        hip.gemm(q[b % c.mod if c.mod else b], k[kb], Sm, M=n_q, N=n_k, K=d, lda=d, ldw=d, ldo=ldS, batch=H, stride_a=n_q * d, stride_w=n_k * d, stride_o=n_q * ldS,
                 out_scale=c.scale, products="split")
        hip.softmax_rows(Sm, rows=H * n_q, cols=n_k, ld=ldS)
        tmp = torch.empty(n_q, C, dtype=torch.float32, device="cuda")
        hip.gemm(Sm, vt[kb], tmp, M=n_q, N=d, K=ldS, lda=ldS, ldw=ldvt, ldo=C, batch=H, stride_a=n_q * ldS, stride_w=d * ldvt, stride_o=d, products="split")
        dst = torch.as_strided(out, (n_q, C), (c.ldo, 1), out.storage_offset() + b * n_q * c.ldo)
        dst.copy_(dst + torch.tensor(c.o_scale, dtype=torch.float32) * tmp if c.accumulate else tmp)
    torch.cuda.synchronize()
    return buf.cpu()


VERSUS = [A.Flash(f"versus-d{d}", "V", "f32", 2, 3, 150, 97, d, S.RTOL, ldvt=104) for d in (40, 64, 80, 160)] + \
         [A.Flash("versus-d40-nk77-acc", "V", "f32", 2, 3, 150, 77, 40, S.RTOL, ldvt=80, accumulate=True, o_scale=0.7)]


@pytest.mark.parametrize("case", VERSUS, ids=A.case_ids(VERSUS))
def test_fused_and_materialised_are_both_inside_their_bounds(hip, case):  # noqa: F811
    """8: one case per head dim of the UNet, and a 77-key accumulate: the fused kernel inside this file's bound; the materialised sequence with split products inside
    its own (attn_split_spec.materialised_bound), with zero pad keys as the engine writes them (its P V GEMM runs over the pad columns of the score tensor).  Their
    mutual rel-L2 is printed for the profile, not asserted"""
    c = case
    ops, ref, _ = S.reference(c)
    fused = launch(hip, c, ops, products="split")
    judge(c, fused, " fused")
    zc = replace(c, name=c.name + "-zero-pad")
    zops = S.operands(zc)
    zops.vt[..., c.n_k:] = 0.0
    mat = _materialised(hip, zc, zops)
    bound = S.materialised_bound(c)
    fig = compare(A.window(c, mat), A.window(c, ref), dtype="f32", bound=bound, rtol=c.rtol, labels=S.labels(c), guard=Guard(zops.buf, mat, zops.mask), tag=c.name + " materialised")
    g, m = A.window(c, fused).double(), A.window(c, mat).double()
    print(f"{c.name}: materialised at {fig['elem_ratio']:.3f} of the bound, rel-L2 {fig['global_rel']:.3e}; fused vs materialised rel-L2 {((g - m).norm() / m.norm()).item():.3e}")
    if FIGURES:
        with open(FIGURES, "a") as f:
            f.write(f"flash V f32split {c.name} materialised {fig['global_rel']:.3e} {fig['elem_ratio']:.4f} mutual {((g - m).norm() / m.norm()).item():.3e}\n")
