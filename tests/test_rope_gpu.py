"""RoPE temporal attention and clips of up to 64 frames on a real MI355X: fyc_temporal_attention with rope_cos / rope_sin against the torch
specification (tests/rope_spec.py, which rounds where the kernel does), the F > 32 instantiations without RoPE against the op emulator,
and the engine / the drop-in module against goldens of the real reference (tools/make_golden_rope.py).

Bounds are those of tests/test_kernels_gpu.py::test_temporal_attention (rel-L2 6e-3 for the 16-bit types, 2e-5 for f32) and of the tiny
UNet forward (f32 1e-3, 16-bit 5e-2: tests/test_engine_gpu.py)."""
import functools
import math
import sys

import pytest
import torch

import rope_spec
from emu_ops import EmuOps
from rope_spec import MM, TINY, engine_forward, load_golden, rel, rope_cfg, rope_weights

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
RTOL = {"bf16": 6e-3, "f16": 6e-3, "f32": 2e-5}
# (clips, F, P, heads, d)
ROPE_SHAPES = [(1, 8, 3, 8, 8),          # partner inside the lane's own fragment
               (1, 16, 5, 8, 40),        # h = 20 straddles fragments; P not a multiple of the 4 tasks per block
               (2, 24, 9, 8, 80),        # two frame tiles, padded frames
               (1, 32, 4, 8, 160),
               (1, 40, 3, 8, 40),        # three frame tiles
               (2, 48, 7, 2, 16),
               (1, 64, 2, 8, 160)]       # four frame tiles at the widest head
LONG_SHAPES = [(1, 33, 5, 8, 80), (1, 40, 3, 8, 40), (1, 64, 2, 8, 160)]


@pytest.fixture(scope="module")
def hip():
    from followyourclick_amd import ops
    h = ops.get()
    h.ensure_init(torch.device("cuda:0"))
    return h


def _scale(F, d):
    return d ** -0.5 * (math.log(16) / math.log(F) if F > 16 else 1.0)


@functools.lru_cache(maxsize=None)
def _case(dt, shape, rope):
    """(qkv, tables or None, specification output) of one case, computed once"""
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
    return qkv, tables, ref, kw


def _run(hip, dt, shape, rope):
    qkv, tables, ref, kw = _case(dt, shape, rope)
    clips, F, P, H, d = shape
    rows, C = clips * F * P, H * d
    o = torch.full((rows + P, C), float("nan"), dtype=DT[dt], device="cuda")      # one sentinel row block behind the output
    extra = dict(rope=tuple(t.cuda() for t in tables)) if rope else {}
    hip.temporal_attention(qkv.cuda(), o, **kw, **extra)
    torch.cuda.synchronize()
    o = o.cpu()
    assert torch.isnan(o[rows:]).all(), "the rows behind the output were written"
    got = o[:rows].double()
    assert torch.isfinite(got).all(), f"{(~torch.isfinite(got)).sum().item()} of {got.numel()} outputs not written or not finite"
    err = ((got - ref.double()).norm() / ref.double().norm()).item()
    print(f"tattn {'rope ' if rope else ''}{dt} {shape}: rel-L2 {err:.3e} (bound {RTOL[dt]:.0e}), max abs {(got - ref.double()).abs().max().item():.3e}")
    assert err <= RTOL[dt], err


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape", ROPE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_temporal_attention_rope(hip, dt, shape):
    _run(hip, dt, shape, True)


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape", LONG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_temporal_attention_more_than_32_frames(hip, dt, shape):
    _run(hip, dt, shape, False)


def test_identity_tables_give_the_bits_of_no_tables(hip):
    """cos = 1, sin = 0: x * 1 + (+/- partner) * 0 is x exactly, and one rounding of a 16-bit value to its own type returns it"""
    clips, F, P, H, d = 2, 16, 64, 8, 40
    qkv = torch.randn(clips * F * P, 3 * H * d, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).cuda()
    kw = dict(clips=clips, frames=F, pixels=P, heads=H, d=d, scale=d ** -0.5)
    a = torch.full((clips * F * P, H * d), float("nan"), dtype=torch.bfloat16, device="cuda")
    b = a.clone()
    hip.temporal_attention(qkv, a, **kw)
    hip.temporal_attention(qkv, b, rope=(torch.ones(F, d // 2, device="cuda"), torch.zeros(F, d // 2, device="cuda")), **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(a.float()).all()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_rope_arguments_are_checked(hip):
    qkv = torch.zeros(16 * 2, 3 * 64, dtype=torch.bfloat16, device="cuda")
    o = torch.zeros(16 * 2, 64, dtype=torch.bfloat16, device="cuda")
    kw = dict(clips=1, frames=16, pixels=2, heads=8, d=8, scale=1.0)
    with pytest.raises(ValueError, match="rope tables"):
        hip.temporal_attention(qkv, o, rope=(torch.ones(16, 8, device="cuda"), torch.zeros(16, 8, device="cuda")), **kw)      # [F][d], not [F][d/2]
    with pytest.raises(ValueError, match="rope tables"):
        hip.temporal_attention(qkv, o, rope=(torch.ones(16, 4, device="cuda", dtype=torch.bfloat16),) * 2, **kw)


# ---- engine and drop-in against the real reference -----------------------------------------------------------------------------------
TOL = {torch.float32: 1e-3, torch.bfloat16: 5e-2, torch.float16: 5e-2}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("F", [16, 40])
def test_engine_forward_vs_reference_golden(golden_dir, F, dtype):
    from followyourclick_amd.engine.unet3d import UNet3DEngine
    from followyourclick_amd.engine.weights import pack_unet
    g = load_golden(golden_dir, F)
    eng = UNet3DEngine(pack_unet(rope_weights(int(g["weight_seed"])), rope_cfg(F), dtype, "cuda:0"))
    assert eng.ops.name == "hip"
    out = engine_forward(eng, g, dtype, "cuda:0")
    assert torch.isfinite(out).all()
    r = rel(out, g["out"])
    print(f"RoPE engine forward F={F} {dtype}: rel-L2 {r:.3e} (bound {TOL[dtype]:.0e})")
    assert r < TOL[dtype], r


@pytest.fixture(scope="module")
def dropin():
    import followyourclick_amd
    followyourclick_amd.install_dropin(force=True)
    yield
    for name in [k for k in sys.modules if k.split(".")[0] in ("animatediff", "diffusers", "ip_adapter")]:
        del sys.modules[name]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("F", [16, 40])
def test_dropin_forward_vs_reference_golden(dropin, golden_dir, F, dtype):
    from animatediff.models.unet import UNet3DConditionModel
    g = load_golden(golden_dir, F)
    unet = UNet3DConditionModel(**TINY, motion_module_kwargs=dict(MM, video_length=F, train_video_length=16), compute_dtype=dtype).to("cuda")
    missing, unexpected = unet.load_state_dict(rope_weights(int(g["weight_seed"])), strict=False)
    assert not unexpected and all(k.endswith("rope.em.inv_freq") for k in missing)
    out = unet(g["sample"].cuda(), torch.tensor(int(g["timestep"])), g["text"].cuda(), use_fps_condition=True,
               fps_tensor=g["fps"].cuda(), flow_control=g["flow"].cuda()).sample.float().cpu()
    assert torch.isfinite(out).all()
    r = rel(out, g["out"])
    print(f"RoPE drop-in forward F={F} {dtype}: rel-L2 {r:.3e} (bound {TOL[dtype]:.0e})")
    assert r < TOL[dtype], r
