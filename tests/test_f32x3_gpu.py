"""fyc_gemm's split-bf16 product rule for f32 operands (include/fyc.h: f32_products = FYC_PRODUCTS_SPLIT_BF16; HipOps.gemm(products="split")) on the GPU, on
everything the f32 mode dispatches: the cases, their f64 references and the bound are tests/f32x3_spec.py's, the guarded buffers tests/gemm_cases.py's.

Every test asks for the rule per call, or sets the mode of the shared HipOps and puts "exact" back in a `finally`: the session's engines must not see it.

Tile: the plan of an f32 problem reads neither `tile` nor fyc_set_tuning key 1 - N picks between the two f32 tile configs (f32x3_spec.GEMM_CASES has both) - so
"tile 1 forced" changes nothing for it; the cases still run with key 1 = 0 and = 1, and both are judged.
Split-K: the plan splits 16-bit problems only.  M 288, N 328, K 520 with key 10 = 2 runs unsplit in f32 in either rule (test_f32_problems_do_not_split_k asserts the
query's answer), so there is no split-K case here.

FYC_F32X3_FIGURES=<file>: append the figures of every comparison to that file (profiles/f32x3_bound_coverage.txt was made from it)."""
import ctypes as C
import os
from dataclasses import replace

import pytest
import torch

import f32x3_spec as X
import gemm_cases as G
from kernel_compare import Guard, compare
from test_engine_gpu import _load, _nhwc, rel, report
from test_gemm_epilogues_gpu import launch, reference
from test_kernels_gpu import hip  # noqa: F401  (the module-scoped library fixture)

pytestmark = pytest.mark.gpu

FIGURES = os.environ.get("FYC_F32X3_FIGURES")


def judge(c, got, ref, S, K, *, group, guard=None, tag=None):
    fig = compare(got, ref, dtype="f32", bound_terms=X.bound_for(S, K, G.tile_shape(c.want_cfg) if c is not None else (128, 64)), guard=guard, tag=tag or c.name)
    if FIGURES:
        with open(FIGURES, "a") as f:
            f.write(f"{group} {tag or c.name} {fig['global_rel']:.3e} {fig['row_rel']:.3e} {fig['column_rel']:.3e} {fig['elem_ratio']:.4f}\n")
    return fig


def run_case(hip, c, *, products="split", ops=None):  # noqa: F811
    """one launch of a gemm_cases.Case in the split rule, judged against the shared f64 reference of its problem; returns the guarded buffer (CPU)"""
    ops0, ref_buf, S = reference(c)
    got_buf = launch(hip, c, ops0 if ops is None else ops, products=products).cpu()
    judge(c, G.logical(c, got_buf), G.logical(c, ref_buf), S, c.K, group=c.group, guard=Guard(ops0.buf, got_buf, ops0.mask), tag=f"{c.name}-key1={c.tile}")
    return got_buf


@pytest.mark.parametrize("key1", [0, 1])
@pytest.mark.parametrize("case", X.GEMM_CASES, ids=G.case_ids(X.GEMM_CASES))
def test_bound_and_guards(hip, case, key1):  # noqa: F811
    """1: PLAIN with residual, out_scale and both row-bias layouts at M 300, N 328 / 384, K 136 (a K tail of 8), the convolution geometries, the one-pixel
    case, the frame-axis convolution and the batched P V stripes: every element inside the bound, nothing outside the output written"""
    run_case(hip, replace(case, tile=key1))


@pytest.mark.parametrize("key1", [0, 1])
@pytest.mark.parametrize("name", sorted(X.epilogue_cases()))
def test_bound_epilogues(hip, name, key1):  # noqa: F811
    """1: GEGLU, HEADS, LINEAR + GELU, the LayerNorm fold, chan_parts and the dual-source A, at the smallest f32 shapes of tests/test_kernels_gpu.py"""
    case = X.epilogue_cases()[name]
    extra = {}
    if name == "chan":
        kw = case["kw"]
        nt, tile_rows, slots = hip.gemm_stat_layout(torch.float32, M=kw["M"], N=kw["N"], K=kw["K"], cs_rows=case["cs_rows"])
        assert tile_rows == 128 and 1 <= slots <= 4, (nt, tile_rows, slots)
        parts = torch.full((nt * slots * kw["N"] * 2,), float("nan"), device="cuda")
        extra = dict(chan_parts=parts, cs_rows=case["cs_rows"])
    hip.set_tuning(G.TUNE_TILE, key1)
    try:
        got = X.run_epilogue_case(hip, case, to=lambda t: t.cuda(), products="split", **extra)
        torch.cuda.synchronize()
    finally:
        hip.set_tuning(G.TUNE_TILE, 0)
    ref = X.run_epilogue_case(G.emulator(torch.float64), case)
    judge(None, got, ref, X.epilogue_bound_terms(case), case["K"], group=name, tag=f"{name}-key1={key1}")
    if name == "chan":      # the statistics are those of the values as stored, whatever rule produced them
        kw = case["kw"]
        cs = torch.zeros(kw["M"] // case["cs_rows"], kw["N"], 2, dtype=torch.float64, device="cuda")
        hip.chan_stats_reduce(parts, cs, rows=kw["M"], N=kw["N"], cs_rows=case["cs_rows"], tile_rows=tile_rows, slots=slots)
        v = got.double().reshape(kw["M"] // case["cs_rows"], case["cs_rows"], kw["N"])
        want = torch.stack([v.sum(dim=1), (v * v).sum(dim=1)], dim=-1)
        assert ((cs.cpu() - want).norm() / want.norm()).item() <= 2e-6


def test_f32_problems_do_not_split_k(hip):  # noqa: F811
    hip.set_tuning(G.TUNE_SPLITK_MIN_KT, 2)
    try:
        assert hip.gemm_split_bytes(torch.float32, M=288, N=328, K=520) == 0
        assert hip.gemm_split_bytes(torch.bfloat16, M=288, N=328, K=520) > 0      # (the 16-bit problem of the same shape does)
    finally:
        hip.set_tuning(G.TUNE_SPLITK_MIN_KT, 0)


def _identity_case():
    """the identity_w layout of the `alias` cases in f32, without bias or residual: out = a I"""
    return replace(G.BY_NAME["alias-bf16-t0"], name="identity-f32", group="identity", dt="f32", residual=0, ldr=0, want_cfg=2, want_ring=-1, want_wide=0)


def test_split_is_taken_and_is_the_specified_one(hip):  # noqa: F811
    """2: with W = I the split rule returns hi(a) + lo(a) BIT FOR BIT - the accumulator receives hi(a) 0 + lo(a) 1 + hi(a) 1 and zeros - which is not a for values
    with more than 16 significant bits; the exact rule returns a.  The bound cannot tell the rules apart (exact products pass it too); this does"""
    c = _identity_case()
    ops = G.operands(c)
    ops.a = ops.a * torch.tensor(1 + 2.0 ** -10 + 2.0 ** -20, dtype=torch.float64).float()
    a = ops.a[:, :c.K]
    hi, lo = X.split_bf16(a)
    got = G.logical(c, launch(hip, c, ops, products="split").cpu())
    assert torch.equal(got.view(torch.int32), (hi + lo).view(torch.int32)), f"{(got != hi + lo).sum().item()} of {got.numel()} elements are not hi(a) + lo(a)"
    assert (got != a).float().mean().item() >= 0.5, "the output is a itself: the products were exact"
    exact = G.logical(c, launch(hip, c, ops, products="exact").cpu())
    assert torch.equal(exact.view(torch.int32), a.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", ["plain-f32-t0r0-rb96", "conv-s1p1-c64-f32-t0r0"])
def test_off_is_off(hip, name):  # noqa: F811
    """3: the instance's default, products="exact" and an argument struct whose new field was never touched launch the same kernel: the same bits"""
    c = G.BY_NAME[name]
    ops, _, _ = reference(c)
    before = hip.f32_products
    hip.set_f32_products("exact")
    try:
        default = launch(hip, c, ops).cpu()
        explicit = launch(hip, c, ops, products="exact").cpu()
        buf = ops.buf.cuda()
        a, w, out, kw = G.gemm_kwargs(c, ops, buf, to=lambda t: t.cuda())
        full = dict(ldo=0, bias=None, rowbias=None, rows_per_batch=1, residual=None, ldr=0, ldrb=0, out_scale=1.0, epilogue=0, mode=0, conv=None, batch=1, stride_a=0,
                    stride_w=0, stride_o=0, heads=None, tile=0, a2=None, k_split=0, lda2=0, act=0, ln_stats=None, ln_colsum=None, ln_nparts=0, ln_eps=1e-5,
                    chan_parts=None, cs_rows=0, row_parts=None, row_nparts=0)
        full.update(kw)
        g = hip._gemm_args(a, w, out, **full)
        assert g.f32_products == 0
        hip._call("fyc_gemm", g)
        torch.cuda.synchronize()
        raw = buf.cpu()
        split = launch(hip, c, ops, products="split").cpu()
    finally:
        hip.set_f32_products(before)
    assert torch.equal(default.view(torch.int32), explicit.view(torch.int32)) and torch.equal(default.view(torch.int32), raw.view(torch.int32))
    assert not torch.equal(default.view(torch.int32), split.view(torch.int32)), "the split rule gave the exact rule's bits"


def test_split_with_16_bit_tensors_raises(hip):  # noqa: F811
    a = torch.zeros(128, 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(TypeError, match="split"):
        hip.gemm(a, a, torch.zeros(128, 128, dtype=torch.bfloat16, device="cuda"), M=128, N=128, K=64, lda=64, ldw=64, ldo=128, products="split")
    with pytest.raises(ValueError):
        hip.gemm(a, a, a, M=128, N=128, K=64, lda=64, ldw=64, ldo=128, products="f16")


def test_non_finite_input_stays_in_its_row(hip):  # noqa: F811
    """4: one Inf in row 7 of A: row 7 of the output is non-finite (NaN rather than Inf: lo = Inf - Inf), every other row is inside the bound"""
    c = G.BY_NAME["plain-f32-t0r0-norb"]
    ops0, ref_buf, S = reference(c)
    ops = replace(ops0, a=ops0.a.clone())
    ops.a[7, 5] = float("inf")
    got_buf = launch(hip, c, ops, products="split").cpu()
    got, ref = G.logical(c, got_buf), G.logical(c, ref_buf)
    assert not bool(torch.isfinite(got[7]).any()), f"{int(torch.isfinite(got[7]).sum())} finite values in the row of the Inf"
    keep = [i for i in range(c.M) if i != 7]
    judge(c, got[keep], ref[keep], S[keep], c.K, group="nonfinite", guard=Guard(ops0.buf, got_buf, ops0.mask), tag="plain-inf-row7")


# ---- the UNet in split mode ------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def split_mode(hip):  # noqa: F811
    """run(fn, mode): fn() with the shared HipOps in `mode`; "exact" is back when the test ends, whatever happened"""
    def run(fn, mode):
        hip.set_f32_products(mode)
        try:
            return fn()
        finally:
            hip.set_f32_products("exact")
    yield run
    hip.set_f32_products("exact")


def test_forward_vs_reference(golden_dir, fullwidth, split_mode):
    """5: one full-width forward (F = 4, 16x16) of the session's f32 engine in split mode: < 1e-3 from the reference's f32 output - the project's figure for the
    f32 tier (tests/test_fullwidth_gpu.py) - and two runs give the same bits"""
    from oracle import functional as Fn
    from oracle import weights as W
    from followyourclick_amd.engine import UNet3DConfig
    g = _load(golden_dir, "unet_full_small_fwd.npz")
    cfg = Fn.UNetConfig()
    F, H, Wd = int(g["frames"]), int(g["h"]), int(g["w"])
    inp = W.seeded_inputs(cfg, 1, F, H, Wd, seed=int(g["input_seed"]))
    x9 = torch.cat([Fn.build_model_input(inp["latents"], inp["first_image_latents"], inp["first_images_mask"])] * 2)
    eng = fullwidth.engine(cfg, UNet3DConfig(), torch.float32, seed=0)
    assert eng.ops.name == "hip"

    def fwd():
        eng.prepare_context(inp["text"])
        _, temb = eng.prepare_time_embeddings([int(g["timestep"])], g["fps"].tolist(), g["flow"].tolist(), 2)
        return eng.forward(_nhwc(x9, torch.float32), temb, 2, F, H, Wd).float().cpu().reshape(2, F, H, Wd, 4).permute(0, 4, 1, 2, 3)
    exact, split, again = split_mode(fwd, "exact"), split_mode(fwd, "split"), split_mode(fwd, "split")
    assert torch.isfinite(split).all()
    r_split, r_exact = rel(split, g["out_f32"]), rel(exact, g["out_f32"])
    report(f"full-width fwd (F=4, 16x16) f32 split-bf16 products: vs ref-f32 {r_split:.3e} (exact products {r_exact:.3e}; split vs exact {rel(split, exact):.3e})")
    assert r_split < 1e-3, r_split
    assert torch.equal(split, again), "two split-mode forwards differ"
    assert not torch.equal(split, exact), "the split-mode forward has the exact mode's bits"


def test_cfg1_trajectory_vs_reference(golden_dir, fullwidth, split_mode):
    """5: BASELINE configs[0] (8 frames 256x256, 5 DDIM steps) in split mode: every step's latents < 1e-3 from the reference pipeline's f32 run"""
    from oracle import functional as Fn
    from followyourclick_amd.engine import UNet3DConfig
    from test_fullwidth_gpu import _trajectory

    def engines(dtype):
        return fullwidth.engine(Fn.UNetConfig(), UNet3DConfig(), dtype, seed=0)
    g, got = split_mode(lambda: _trajectory(golden_dir, engines, "cfg1_trajectory.npz", torch.float32, 5), "split")
    _, exact = split_mode(lambda: _trajectory(golden_dir, engines, "cfg1_trajectory.npz", torch.float32, 5), "exact")
    assert sorted(got) == list(range(5))
    for i in sorted(got):
        r_split, r_exact = rel(got[i], g[f"step{i}_f32"]), rel(exact[i], g[f"step{i}_f32"])
        report(f"cfg1 step {i} f32 split-bf16 products: vs ref-f32 {r_split:.3e} (exact products {r_exact:.3e})")
        assert torch.isfinite(got[i]).all()
        assert r_split < 1e-3, (i, r_split)
