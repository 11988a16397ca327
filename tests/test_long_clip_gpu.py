"""Temporal attention over clips of 65 .. 256 frames on a real MI355X: the long-clip kernel (csrc/temporal_attn_long.hip) and the exact f32
kernel against the f64 specification (tests/rope_spec.py with tables, the op emulator without), the long kernel against the register-resident
one where both run (kernel="long" below 65 frames), and the engine / the drop-in module against goldens of the real reference
(tools/make_golden_long.py).

Bounds: rel-L2 6e-3 for the 16-bit types and 2e-5 for f32 (tests/test_rope_gpu.py); the tiny UNet forward by tests/long_clip_spec.py::TOL."""
import functools
import math
import sys

import pytest
import torch

import long_clip_spec as S
import rope_spec
from emu_ops import EmuOps
from rope_spec import TINY, engine_forward, rel, rope_weights

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
RTOL = {"bf16": 6e-3, "f16": 6e-3, "f32": 2e-5}

# (clips, F, P, heads, d)
SHAPES = [(1, 65, 3, 8, 40),        # one frame into the fifth query tile and the second key block
          (1, 80, 2, 8, 160),       # widest head
          (2, 96, 5, 2, 16),
          (1, 128, 3, 8, 80),
          (1, 200, 2, 8, 40),       # F no multiple of 16 or 64
          (1, 256, 2, 8, 160)]      # the limit: 16 waves, four key blocks
AB_SHAPES = [(1, 48, 4, 8, 40), (2, 64, 3, 8, 160)]
AB_TOL = 1.2e-2                     # two results inside 6e-3 of the specification are within 1.2e-2 of each other (triangle inequality)


@pytest.fixture(scope="module")
def hip():
    from followyourclick_amd import ops
    h = ops.get()
    h.ensure_init(torch.device("cuda:0"))
    return h


def _scale(F, d):
    """as tests/test_rope_gpu.py::_scale: the query factor of a model trained on 16 frames rides on the softmax scale"""
    return d ** -0.5 * (math.log(16) / math.log(F) if F > 16 else 1.0)


@functools.lru_cache(maxsize=None)
def _case(dt, shape, rope):
    """(qkv, tables or None, specification output - f64 accumulation, rounded to the storage type as the kernel's - as f64, keywords) of one
    case, computed once"""
    clips, F, P, H, d = shape
    g = torch.Generator().manual_seed(1000 * F + d)
    qkv = torch.randn(clips * F * P, 3 * H * d, generator=g).to(DT[dt])
    kw = dict(clips=clips, frames=F, pixels=P, heads=H, d=d, scale=_scale(F, d))
    ref = torch.zeros(clips * F * P, H * d, dtype=DT[dt])
    tables = rope_spec.rope_tables(d, F) if rope else None
    if rope:
        rope_spec.temporal_attention(qkv, ref, rope=tables, acc=torch.float64, **kw)
    else:
        EmuOps(acc=torch.float64).temporal_attention(qkv, ref, **kw)
    return qkv, tables, ref.double(), kw


def _launch(hip, dt, shape, rope, **extra):
    """the kernel's output rows as f64, after the checks every launch gets: the NaN-filled buffer is written everywhere inside the problem
    with finite values and nowhere behind it"""
    qkv, tables, ref, kw = _case(dt, shape, rope)
    clips, F, P, H, d = shape
    rows, C = clips * F * P, H * d
    o = torch.full((rows + P, C), float("nan"), dtype=DT[dt], device="cuda")      # one sentinel row block behind the output
    if rope:
        extra = dict(extra, rope=tuple(t.cuda() for t in tables))
    hip.temporal_attention(qkv.cuda(), o, **kw, **extra)
    torch.cuda.synchronize()
    o = o.cpu()
    assert torch.isnan(o[rows:]).all(), "the rows behind the output were written"
    got = o[:rows].double()
    assert torch.isfinite(got).all(), f"{(~torch.isfinite(got)).sum().item()} of {got.numel()} outputs not written or not finite"
    return got


def _err(got, ref):
    return ((got - ref).norm() / ref.norm()).item()


def _run(hip, dt, shape, rope, **extra):
    got, ref = _launch(hip, dt, shape, rope, **extra), _case(dt, shape, rope)[2]
    err = _err(got, ref)
    print(f"tattn long {'rope ' if rope else ''}{dt} {shape} {extra or ''}: rel-L2 {err:.3e} (bound {RTOL[dt]:.0e}), max abs {(got - ref).abs().max().item():.3e}")
    assert err <= RTOL[dt], err


@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_temporal_attention_long_clip(hip, dt, shape, rope):
    _run(hip, dt, shape, rope)


@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
def test_split_products_above_64_frames_run_the_exact_kernel(hip, rope):
    _run(hip, "f32", (2, 96, 5, 2, 16), rope, products="split")


@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("shape", AB_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_long_kernel_against_the_register_resident_kernel(hip, dt, shape, rope):
    ref = _case(dt, shape, rope)[2]
    short, long_ = _launch(hip, dt, shape, rope), _launch(hip, dt, shape, rope, kernel="long")
    es, el, ab = _err(short, ref), _err(long_, ref), _err(long_, short)
    print(f"tattn A/B {'rope ' if rope else ''}{dt} {shape}: short {es:.3e}, long {el:.3e} of the specification (bound {RTOL[dt]:.0e}); long vs short {ab:.3e} (bound {AB_TOL:.1e})")
    assert es <= RTOL[dt] and el <= RTOL[dt], (es, el)
    assert ab <= AB_TOL, ab


def test_identity_tables_give_the_bits_of_no_tables(hip):
    """cos = 1, sin = 0: x * 1 + (+/- partner) * 0 is x exactly, and one rounding of a 16-bit value to its own type returns it"""
    clips, F, P, H, d = 1, 96, 6, 8, 40
    qkv = torch.randn(clips * F * P, 3 * H * d, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).cuda()
    kw = dict(clips=clips, frames=F, pixels=P, heads=H, d=d, scale=_scale(F, d))
    a = torch.full((clips * F * P, H * d), float("nan"), dtype=torch.bfloat16, device="cuda")
    b = a.clone()
    hip.temporal_attention(qkv, a, **kw)
    hip.temporal_attention(qkv, b, rope=(torch.ones(F, d // 2, device="cuda"), torch.zeros(F, d // 2, device="cuda")), **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(a.float()).all()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_limits_are_checked(hip):
    from followyourclick_amd._lib import FycError

    def tensors(F, dtype):
        return torch.zeros(F * 2, 3 * 64, dtype=dtype, device="cuda"), torch.zeros(F * 2, 64, dtype=dtype, device="cuda")
    kw = dict(clips=1, pixels=2, heads=8, d=8, scale=1.0)
    assert hip.temporal_attention_max_frames == 256      # what UNet3DEngine._rope asks the backend
    for dtype in (torch.bfloat16, torch.float32):
        with pytest.raises(FycError, match="256"):
            hip.temporal_attention(*tensors(257, dtype), frames=257, **kw)
    with pytest.raises(FycError, match="256"):
        hip.temporal_attention(*tensors(257, torch.bfloat16), frames=257, kernel="long", **kw)
    with pytest.raises(FycError, match="FYC_BF16 / FYC_F16"):
        hip.temporal_attention(*tensors(96, torch.float32), frames=96, kernel="long", **kw)
    with pytest.raises(FycError, match="17 frames"):
        hip.temporal_attention(*tensors(16, torch.bfloat16), frames=16, kernel="long", **kw)
    with pytest.raises(ValueError, match="kernel"):
        hip.temporal_attention(*tensors(96, torch.bfloat16), frames=96, kernel="short", **kw)


def test_no_fused_temporal_block_for_long_clips(hip):
    """the fused C = 320 sub-block is a 16-frame kernel: the library answers no for the shape it is built for at any other clip length"""
    shape = dict(clips=2, pixels=64, heads=8, d=40)
    assert hip.temporal_block_supported(torch.bfloat16, frames=16, **shape)
    for F in (65, 96, 128, 256):
        assert not hip.temporal_block_supported(torch.bfloat16, frames=F, **shape)


# ---- engine and drop-in against the real reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("which", ["rope96", "pe128"])
def test_engine_forward_vs_reference_golden(golden_dir, which, dtype):
    from followyourclick_amd.engine.unet3d import UNet3DEngine
    from followyourclick_amd.engine.weights import pack_unet
    g = S.load(golden_dir, which)
    eng = UNet3DEngine(pack_unet(rope_weights(int(g["weight_seed"])), S.cfg_of(which), dtype, "cuda:0"))
    assert eng.ops.name == "hip"
    out = engine_forward(eng, g, dtype, "cuda:0")
    assert torch.isfinite(out).all()
    r = rel(out, g["out"])
    print(f"long-clip engine forward {which} {dtype}: rel-L2 {r:.3e} (bound {S.TOL[dtype]:.0e})")
    assert r < S.TOL[dtype], r


@pytest.fixture(scope="module")
def dropin():
    import followyourclick_amd
    followyourclick_amd.install_dropin(force=True)
    yield
    for name in [k for k in sys.modules if k.split(".")[0] in ("animatediff", "diffusers", "ip_adapter")]:
        del sys.modules[name]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("which", ["rope96", "pe128"])
def test_dropin_forward_vs_reference_golden(dropin, golden_dir, which, dtype):
    from animatediff.models.unet import UNet3DConditionModel
    g = S.load(golden_dir, which)
    unet = UNet3DConditionModel(**TINY, motion_module_kwargs=S.motion_kwargs(which), compute_dtype=dtype).to("cuda")
    missing, unexpected = unet.load_state_dict(rope_weights(int(g["weight_seed"])), strict=False)
    kept = "rope.em.inv_freq" if which == "rope96" else "pos_encoder.pe"      # formula-valued buffers the seeded weights leave out
    assert not unexpected and all(k.endswith(kept) for k in missing)
    out = unet(g["sample"].cuda(), torch.tensor(int(g["timestep"])), g["text"].cuda(), use_fps_condition=True,
               fps_tensor=g["fps"].cuda(), flow_control=g["flow"].cuda()).sample.float().cpu()
    assert torch.isfinite(out).all()
    r = rel(out, g["out"])
    print(f"long-clip drop-in forward {which} {dtype}: rel-L2 {r:.3e} (bound {S.TOL[dtype]:.0e})")
    assert r < S.TOL[dtype], r


def test_animation_pipeline_96_frames(dropin):
    """AnimationPipeline.__call__(video_length=96) with a rotary UNet built for 96 frames: sampling and the per-frame VAE decode run end to end
    (no golden: the reference pipeline at this length is not recorded; the UNet forward it repeats is judged above), and every temporal
    attention of the run is a 96-frame launch"""
    from animatediff.models.unet import UNet3DConditionModel
    from animatediff.pipelines.pipeline_animation import AnimationPipeline
    from diffusers import AutoencoderKL, DDIMScheduler
    from followyourclick_amd import ops
    from oracle import functional as Fn
    from oracle import stubs
    from oracle import weights as W
    dtype, F = torch.bfloat16, 96
    kw = dict(TINY, use_fps_condition=False, use_first_frame_mask_condition_concat=False)
    unet = UNet3DConditionModel(**kw, motion_module_kwargs=S.motion_kwargs("rope96"), compute_dtype=dtype)
    ocfg = Fn.tiny_unet_config(use_fps_condition=False, use_first_frame_mask_condition_concat=False)
    sd = {k: v for k, v in W.make_weights(W.unet_state_shapes(ocfg), 0).items() if not k.endswith("pos_encoder.pe")}
    missing, unexpected = unet.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("rope.em.inv_freq") for k in missing)
    vae = AutoencoderKL(block_out_channels=(64, 128, 128, 128), layers_per_block=2, latent_channels=4, compute_dtype=dtype)
    vae.load_state_dict(W.make_weights(W.vae_decoder_state_shapes(Fn.VAEConfig(block_out_channels=(64, 128, 128, 128))), 1), strict=False)
    sched = DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
    pipe = AnimationPipeline(vae=vae, text_encoder=stubs.StubTextEncoder(64), tokenizer=stubs.FakeTokenizer(), unet=unet, scheduler=sched).to("cuda")
    h, frames = ops.get(), []
    launch = h.temporal_attention

    def spy(qkv, o, **k):
        frames.append((k["frames"], k.get("rope") is not None))
        return launch(qkv, o, **k)
    h.temporal_attention = spy
    try:
        out = pipe("a corgi waving its tail", video_length=F, height=64, width=64, num_inference_steps=2, guidance_scale=7.5, negative_prompt="blurry",
                   latents=torch.randn(1, 4, F, 8, 8, generator=torch.Generator().manual_seed(3)))
    finally:
        del h.temporal_attention
    assert frames and set(frames) == {(F, True)}, set(frames)
    assert out.videos.shape == (1, 3, F, 64, 64) and torch.isfinite(out.videos).all()
    assert out.videos.std().item() > 1e-3
