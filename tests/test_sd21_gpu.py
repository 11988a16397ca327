"""The SD-2.1 UNet family on the GPU, all through the C ABI: the head-split GEMM epilogue and fyc_attention at this family's head layout (5 / 10 / 20
heads of 64, and the tiny model's 1 / 2 / 4), an f16 case whose raw scores exceed the f16 range (why upcast_attention is a no-op), engine and drop-in
forwards against goldens of the real reference (tools/make_golden_sd21.py), the 2-D UNet, the gelu CLIP text encoder, repeatability."""
import functools
import math
import os
import sys

import pytest
import torch

import attention_cases as A
import sd21_spec as S
import test_attention_bounds_gpu as TB
from emu_ops import EmuOps
from kernel_compare import Guard, compare
from sd21_spec import engine_forward, golden_name, load_golden, rel, sd21_cfg, sd21_weights
from test_kernels_gpu import DT, RTOL, close, rnd

pytestmark = pytest.mark.gpu

EMU = EmuOps(acc=torch.float64)
LAYOUTS = [(5, 64, 320), (10, 64, 640), (20, 64, 1280), (1, 64, 64), (2, 64, 128), (4, 64, 256)]        # (heads, d, seg_cols)
LAYOUT_IDS = [f"h{h}-c{c}" for h, _, c in LAYOUTS]
GUARD = 96              # NaN elements in front of and behind every output


@pytest.fixture(scope="module")
def hip():
    from followyourclick_amd import ops
    h = ops.get()
    h.ensure_init(torch.device("cuda:0"))
    assert h.name == "hip"
    return h


# ---- fyc_gemm, HEADS epilogue ------------------------------------------------------------------------------------------------------------
def _head_outs(Bn, heads, d, tokens, segs, T, guarded):
    """the outputs of a head-split GEMM, one per segment: q / k as [Bn][H][tokens][d], V^T as [Bn][H][d][ld], ld = tokens rounded up to 8 with zero pad
    columns (as the engine allocates it).  guarded: each inside its own NaN-filled device buffer, every element the kernel must write NaN as well"""
    ld = (tokens + 7) // 8 * 8
    bufs, outs = [], []
    for tr in segs:
        shape = (Bn, heads, d, ld) if tr else (Bn, heads, tokens, d)
        n = math.prod(shape)
        if not guarded:
            outs.append(torch.zeros(shape, dtype=T))
            continue
        buf = torch.full((GUARD + n + GUARD,), float("nan"), dtype=T, device="cuda")
        o = buf[GUARD:GUARD + n].view(shape)
        if tr:
            o[..., tokens:] = 0
        bufs.append(buf)
        outs.append(o)
    return bufs, outs, ld


@functools.lru_cache(maxsize=None)
def _heads_problem(dt, layout, tokens, Bn, K, fold, segs):
    """operands and the emulator's (f64-accumulated) result, computed once per problem and shared by the tile cases"""
    heads, d, C = layout
    T, M, N = DT[dt], Bn * tokens, len(segs) * C
    a, w, bias = rnd((M, K), T, 1), rnd((N, K), T, 2, 1 / math.sqrt(K)), rnd((N,), torch.float32, 3)
    ln = {}
    if fold:            # a folded LayerNorm: per-row {mean, rstd} and the column sums of the weight
        ln = dict(ln_stats=torch.stack([0.1 * rnd((M,), torch.float32, 4), 1 + 0.1 * rnd((M,), torch.float32, 5).abs()], dim=1).contiguous(),
                  ln_colsum=rnd((N,), torch.float32, 6))
    _, outs, ld = _head_outs(Bn, heads, d, tokens, segs, T, guarded=False)
    kw = dict(M=M, N=N, K=K, lda=K, ldw=K, epilogue=2)
    EMU.gemm(a, w, None, bias=bias, heads=dict(seg_cols=C, heads=heads, tokens=tokens, outs=outs, transposed=list(segs), ld=[ld * s for s in segs]), **kw, **ln)
    return a, w, bias, ln, outs, kw


def _run_heads(hip, dt, layout, tokens, Bn, K, fold, segs=(0, 0, 1), tile=0):
    heads, d, C = layout
    a, w, bias, ln, ref, kw = _heads_problem(dt, layout, tokens, Bn, K, fold, segs)
    bufs, outs, ld = _head_outs(Bn, heads, d, tokens, segs, DT[dt], guarded=True)
    hip.gemm(a.cuda(), w.cuda(), None, bias=bias.cuda(), tile=tile, **{k: v.cuda() for k, v in ln.items()},
             heads=dict(seg_cols=C, heads=heads, tokens=tokens, outs=outs, transposed=list(segs), ld=[ld * s for s in segs]), **kw)
    torch.cuda.synchronize()
    for i, (o, r, buf) in enumerate(zip(outs, ref, bufs)):
        close(o, r, f"heads {dt} {layout} tokens {tokens} K {K} fold {fold} tile {tile} seg {i}", RTOL[dt])
        assert torch.isnan(buf[:GUARD].float()).all() and torch.isnan(buf[-GUARD:].float()).all(), f"segment {i}: written outside its output"
        if segs[i]:
            assert not o[..., tokens:].any(), "the pad columns of V^T were written"


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("fold", [False, True], ids=["k64", "kC-ln"])
@pytest.mark.parametrize("tokens", [64, 77])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_gemm_heads_at_the_family_layouts(hip, layout, tokens, fold, dt):
    """q | k | v of the fused QKV projection, batch 3: 64 tokens (the wide epilogue in bf16 / f16), 77 (no multiple of 16: the narrow one); K = 64, and
    K = seg_cols with a folded LayerNorm as the engine issues it"""
    _run_heads(hip, dt, layout, tokens, 3, layout[2] if fold else 64, fold)


@pytest.mark.parametrize("tile", [1, 5, 6, 11])          # the tile configs of test_kernels_gpu.py::test_gemm_heads_every_wide_tile
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_gemm_heads_wide_epilogue_on_every_tile(hip, layout, dt, tile):
    """the wide head-split epilogue (its divisions by seg_cols and by the head dim) at d = 64 with a folded LayerNorm, 5 x 64 tokens"""
    _run_heads(hip, dt, layout, 64, 5, layout[2], True, tile=tile)


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("layout", [LAYOUTS[0], LAYOUTS[2]], ids=[LAYOUT_IDS[0], LAYOUT_IDS[2]])
def test_gemm_heads_text_keys_from_context_1024(hip, layout, dt):
    """K | V^T of the cross-attention cache: 2 prompts x 77 tokens of a 1024-wide context"""
    _run_heads(hip, dt, layout, 77, 2, 1024, False, segs=(0, 1))


# ---- fyc_attention ------------------------------------------------------------------------------------------------------------------------
def _attention_cases():
    out = []
    for dt in ("bf16", "f16"):
        for H in (5, 20):
            for qt in (2, 3, 4):
                for n in (64, 100):     # 100: a ragged last key block (one full 64-key tile, then 36), ragged query blocks
                    out.append(A.Flash(f"sd21-{dt}-h{H}-qt{qt}-self{n}", "A", dt, 2, H, n, n, 64, A.RTOL_FLASH[dt], qt=qt, ldvt=(n + 7) // 8 * 8))
                # cross-attention on the text cache: 4 frames share 2 prompts of 77 keys
                out.append(A.Flash(f"sd21-{dt}-h{H}-qt{qt}-cross77", "C", dt, 4, H, 64, 77, 64, A.RTOL_FLASH[dt], qt=qt, ldvt=80, div=2))
        # the dispatch's own choice (tuning key 3 at 0) at the smallest problem where it is QT = 3 for d = 64: n_q = 1024 and
        # batch * heads * ceil(n_q / 192) = 600 >= 512; 40 keys keep the f64 reference of the 100 (batch, head) pairs short
        out.append(A.Flash(f"sd21-{dt}-h20-auto-nq1024-nk40", "C", dt, 5, 20, 1024, 40, 64, A.RTOL_FLASH[dt], qt=0, ldvt=40, div=5))
    return out


ATTENTION = _attention_cases()


@pytest.mark.parametrize("case", ATTENTION, ids=A.case_ids(ATTENTION))
def test_attention_d64_at_5_and_20_heads(hip, case):
    """every element within the bound of tests/kernel_compare.py against the plain f64 reference, nothing outside the output written; the query tile
    asked for is the one that runs (d = 64 <= 80)"""
    if case.qt:
        assert A.effective_qt(case) == case.qt and A.traits(case)["xcd"] == (case.H == 20)
    else:
        assert case.n_q >= 1024 and case.B * case.H * ((case.n_q + 191) // 192) >= 512
    TB._run(hip, case)


def test_attention_f16_scores_beyond_the_f16_range(hip):
    """q and k entries of magnitude 100 at d = 64: the raw dot products reach 6.4e5, ten times the largest f16 number - the situation upcast_attention
    exists for in the reference.  The kernel forms the scores in f32 from a pre-scaled q and soft-maxes them in f32: the output is finite and inside the
    same per-element bound.  Every query's own key leads the others by thousands of log2 units, so the expected output is one value row."""
    c = A.Flash("sd21-f16-overflow", "D", "f16", 2, 5, 64, 64, 64, A.RTOL_FLASH["f16"], ldvt=64)
    ops = A.operands(c)
    g = torch.Generator().manual_seed(5)
    code = A._codes(c.n_k, c.d).float()
    sigma = torch.stack([torch.stack([torch.randperm(c.n_k, generator=g) for _ in range(c.H)]) for _ in range(c.B)])
    tau = torch.randint(0, c.n_k, (c.B, c.H, c.n_q), generator=g)
    jit = lambda: 1 + 0.02 * torch.randn(c.B, c.H, c.n_q, c.d, generator=g)          # noqa: E731
    ops.k = (100.0 * code[sigma] * jit()).to(torch.float16)
    ops.q = ops.q_full = (100.0 * code[tau] * jit()).to(torch.float16)
    raw = torch.matmul(ops.q.double(), ops.k.double().transpose(-1, -2))
    assert raw.max().item() > 5 * 65504 and ops.q.abs().max().item() < 120
    top = torch.topk(raw * c.scale * 1.4426950408889634, 2, dim=-1).values
    assert (top[..., 0] - top[..., 1]).min().item() > 1000                         # log2 units between a query's key and the runner-up
    ref, bound, w = A.reference(c, ops)
    assert w.max(dim=-1).values.min().item() == 1.0
    got = TB.launch(hip, c, ops)
    fig = compare(A.window(c, got), A.window(c, ref), dtype=c.dt, bound=bound, rtol=c.rtol, labels=A.labels(c), guard=Guard(ops.buf, got, ops.mask), tag=c.name)
    print(f"{c.name}: largest raw score {raw.max().item():.3e}; global rel-L2 {fig['global_rel']:.3e}, worst element at {fig['elem_ratio']:.3f} of its bound")


# ---- engine and drop-in against the real reference ---------------------------------------------------------------------------------------
TOL = {torch.float32: S.TOL_F32, torch.bfloat16: S.TOL_16, torch.float16: S.TOL_16}
GOLDENS = [(5, False), (16, False), (5, True)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _engine(g, tconv, dtype):
    from followyourclick_amd.engine.unet3d import UNet3DEngine
    from followyourclick_amd.engine.weights import pack_unet
    cfg = sd21_cfg(use_temporal_conv=tconv)
    eng = UNet3DEngine(pack_unet(sd21_weights(cfg, int(g["weight_seed"])), cfg, dtype, "cuda:0"))
    assert eng.ops.name == "hip"
    return eng


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F,tconv", GOLDENS)
def test_engine_forward_vs_reference_golden(golden_dir, F, tconv, dtype):
    g = load_golden(golden_dir, golden_name(F, tconv))
    out = engine_forward(_engine(g, tconv, dtype), g, dtype, "cuda:0")
    assert torch.isfinite(out).all()
    r = rel(out, g["out"])
    print(f"sd21 engine forward F={F} tconv={tconv} {dtype}: rel-L2 {r:.3e} (bound {TOL[dtype]:.0e})")
    assert r < TOL[dtype], r


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_engine_forward_is_repeatable(golden_dir, dtype):
    g = load_golden(golden_dir, golden_name(5))
    eng = _engine(g, False, dtype)
    a, b = engine_forward(eng, g, dtype, "cuda:0"), engine_forward(eng, g, dtype, "cuda:0")
    assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.fixture(scope="module")
def dropin():
    import followyourclick_amd
    old = os.environ.get("FYC_UNET_VARIANTS")
    os.environ["FYC_UNET_VARIANTS"] = "1"                 # the drop-in builds these model families on request only
    followyourclick_amd.install_dropin(force=True)
    yield
    if old is None:
        del os.environ["FYC_UNET_VARIANTS"]
    else:
        os.environ["FYC_UNET_VARIANTS"] = old
    for name in [k for k in sys.modules if k.split(".")[0] in ("animatediff", "diffusers", "ip_adapter")]:
        del sys.modules[name]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F,tconv", GOLDENS)
def test_dropin_forward_vs_reference_golden(dropin, golden_dir, F, tconv, dtype):
    from animatediff.models.unet import UNet3DConditionModel
    g = load_golden(golden_dir, golden_name(F, tconv))
    unet = UNet3DConditionModel(**S.TINY, use_temporal_conv=tconv, compute_dtype=dtype).to("cuda")
    unet.load_state_dict(sd21_weights(sd21_cfg(use_temporal_conv=tconv), int(g["weight_seed"])), strict=True)
    out = unet(g["sample"].cuda(), torch.tensor(int(g["timestep"])), g["text"].cuda(), use_fps_condition=True,
               fps_tensor=g["fps"].cuda(), flow_control=g["flow"].cuda()).sample.float().cpu()
    assert torch.isfinite(out).all()
    r = rel(out, g["out"])
    print(f"sd21 drop-in forward F={F} tconv={tconv} {dtype}: rel-L2 {r:.3e} (bound {TOL[dtype]:.0e})")
    assert r < TOL[dtype], r


@pytest.mark.parametrize("dtype", DTYPES)
def test_unet2d_forward_vs_reference_golden(dropin, golden_dir, dtype):
    from diffusers import UNet2DConditionModel
    g = load_golden(golden_dir, "sd2d_unet_sd21_fwd.npz")
    unet = UNet2DConditionModel(**S.TINY_2D, compute_dtype=dtype).to("cuda")
    unet.load_state_dict(sd21_weights(S.sd21_cfg_2d(), int(g["weight_seed"])), strict=True)
    out = unet(g["sample"].cuda(), torch.tensor(int(g["timestep"])), g["text"].cuda()).sample.float().cpu()
    assert out.shape == g["out"].shape and torch.isfinite(out).all()
    r = rel(out, g["out"])
    print(f"sd21 2-D forward {dtype}: rel-L2 {r:.3e} (bound {TOL[dtype]:.0e})")
    assert r < TOL[dtype], r


# ---- text encoder ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 3e-2)])      # the bounds of tests/test_encoders_gpu.py
def test_clip_text_gelu(dtype, tol):
    """2 layers, hidden 128, 2 heads of 64, hidden_act "gelu" through ClipTextHip against transformers.CLIPTextModel"""
    from followyourclick_amd.encoders import ClipTextHip
    sd, ids, ref = S.clip_gelu_case()
    enc = ClipTextHip(sd, dict(S.CLIP_GELU, eos_token_id=2), compute_dtype=dtype).to("cuda")
    assert enc.engine_config.hidden_act == "gelu"
    out = enc(ids.cuda()).last_hidden_state.float().cpu()
    r = rel(out, ref)
    print(f"CLIP text gelu {dtype}: rel-L2 {r:.3e}")
    assert out.shape == ref.shape and r < tol, r
