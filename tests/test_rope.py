"""RoPE motion module (motion_module_kwargs.use_rope_postion_encoding) without a GPU: the specification of the rotated temporal attention
(tests/rope_spec.py) against the reference's VersatileAttention, the engine on the op emulator against goldens of the real reference
(tools/make_golden_rope.py), the state-dict schema, the drop-in constructor, and the schedule (never the fused temporal block)."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import rope_spec
from rope_spec import MM, TINY, TRAIN, engine_forward, load_golden, rel, rope_cfg, rope_weights
from followyourclick_amd.engine import unet3d
from followyourclick_amd.engine.schema import unet_schema
from followyourclick_amd.engine.unet3d import UNet3DEngine
from followyourclick_amd.engine.weights import pack_unet, rope_tables
from oracle import refshim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the specification against the reference module ------------------------------------------------------------------------------
SPEC_VS_REFERENCE = r"""
import math, sys, torch
sys.path.insert(0, sys.argv[1])
from oracle import refshim
refshim.install()
import rope_spec
from rope_spec import MM, TINY, TRAIN, engine_forward, load_golden, rel, rope_cfg, rope_weights
from animatediff.models.motion_module import VersatileAttention
for C, H, F, train in ((64, 8, 16, 16), (320, 8, 48, 16), (80, 2, 40, 16)):
    torch.manual_seed(C + F)
    d, B, P = C // H, 2, 3
    att = VersatileAttention(attention_mode="Temporal", use_rope_postion_encoding=True, temporal_position_encoding_max_len=32,
                             video_length=F, train_video_length=train, query_dim=C, heads=H, dim_head=d, cross_attention_dim=None).eval()
    hs = torch.randn(B * F, P, C)
    with torch.no_grad():
        ref = att(hs, video_length=F)
        qkv = torch.cat([att.to_q(hs), att.to_k(hs), att.to_v(hs)], dim=-1).reshape(B * F * P, 3 * C)
        o = torch.zeros(B * F * P, C)
        scale = d ** -0.5 * (math.log(train) / math.log(F) if F > train else 1.0)
        rope_spec.temporal_attention(qkv, o, clips=B, frames=F, pixels=P, heads=H, d=d, scale=scale, rope=rope_spec.rope_tables(d, F), acc=torch.float32)
        got = att.to_out[0](o).reshape(B * F, P, C)
    print("MAXABS", C, H, F, float((got - ref).abs().max()), float(ref.abs().max()))
"""


@pytest.mark.skipif(not refshim.available(), reason="the reference tree is not present")
def test_spec_matches_reference_versatile_attention():
    """f32, (C, heads, F, train) = (64, 8, 16, 16), (320, 8, 48, 16), (80, 2, 40, 16): max abs <= 1e-6.  In a subprocess: the reference's
    `animatediff` package and the drop-in's cannot share an interpreter."""
    r = subprocess.run([sys.executable, "-c", SPEC_VS_REFERENCE, os.path.join(ROOT, "tests")], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith("MAXABS")]
    assert len(lines) == 3, r.stdout
    for _, C, H, F, err, mag in lines:
        print(f"spec vs VersatileAttention C={C} heads={H} F={F}: max abs {float(err):.3e} (|ref| max {float(mag):.3f})")
        assert float(err) <= 1e-6, (C, H, F, err)


def test_engine_tables_follow_the_formula():
    """engine/weights.py::rope_tables against the specification's, and against the reference's table layout cat((freqs, freqs))"""
    for d, F in ((8, 16), (40, 40), (160, 64)):
        cos, sin = rope_tables(d, F)
        cs, ss = rope_spec.rope_tables(d, F)
        assert cos.dtype == torch.float32 and cos.shape == (F, d // 2) and cos.is_contiguous()
        assert torch.equal(cos, cs) and torch.equal(sin, ss)


# ---- the engine on the emulator against the real reference -------------------------------------------------------------------------
@pytest.mark.parametrize("F", [16, 40])
def test_engine_on_emulator_matches_reference_golden(golden_dir, F, monkeypatch):
    g = load_golden(golden_dir, F)
    assert int(g["F"]) == F and g["sample"].shape[2] == F
    eng = UNet3DEngine(pack_unet(rope_weights(int(g["weight_seed"])), rope_cfg(F), torch.float32, "cpu"), ops=rope_spec.RopeEmuOps())
    r = rel(engine_forward(eng, g), g["out"])
    print(f"RoPE engine on the emulator, F={F}: rel-L2 {r:.3e}")
    assert r < 1e-3, r
    # control: the fixture sees the rotation (identity tables: cos = 1, sin = 0)
    eng._rope_tables = {k: (torch.ones_like(c), torch.zeros_like(s)) for k, (c, s) in eng._rope_tables.items()}
    assert len(eng._rope_tables) == 3                              # d = 8, 16, 32 at this clip length
    r0 = rel(engine_forward(eng, g), g["out"])
    print(f"  without the rotation: rel-L2 {r0:.3e}")
    assert r0 > 0.1, r0
    if F > TRAIN:                                                  # control: the fixture sees the ln(train) / ln(video) query factor
        eng = UNet3DEngine(pack_unet(rope_weights(int(g["weight_seed"])), rope_cfg(TRAIN), torch.float32, "cpu"), ops=rope_spec.RopeEmuOps())
        r1 = rel(engine_forward(eng, g), g["out"])
        print(f"  without the ln({TRAIN})/ln({F}) factor: rel-L2 {r1:.3e}")
        assert r1 > 5e-2, r1


def test_query_factor_uses_the_constructor_length(golden_dir):
    """a model built for 40 frames scales its queries by ln 16 / ln 40 at ANY clip length (reference rope.py:169-172)"""
    scales = []

    class Spy(rope_spec.RopeEmuOps):
        def temporal_attention(self, qkv, o, **kw):
            scales.append((kw["d"], kw["scale"], kw.get("rope") is not None))
            return super().temporal_attention(qkv, o, **kw)
    g = load_golden(golden_dir, 16)
    eng = UNet3DEngine(pack_unet(rope_weights(0), rope_cfg(40), torch.float32, "cpu"), ops=Spy())
    engine_forward(eng, g)
    assert scales and all(r for _, _, r in scales)
    for d, s, _ in scales:
        assert s == pytest.approx(d ** -0.5 * math.log(16) / math.log(40), rel=1e-12)


def test_more_than_64_frames_is_refused():
    eng = UNet3DEngine(pack_unet(rope_weights(0), rope_cfg(16), torch.float32, "cpu"), ops=rope_spec.RopeEmuOps())
    with pytest.raises(ValueError, match="64 frames"):
        eng._rope(8, 65)


def test_no_fused_temporal_block_under_rope(golden_dir, monkeypatch):
    """an ops object that offers the fused temporal sub-block for every shape: a RoPE engine still never takes it"""
    monkeypatch.setattr(unet3d, "FUSE_TEMPORAL", True)
    calls = []

    class Eager(rope_spec.RopeEmuOps):
        def temporal_block_supported(self, dtype, **kw):
            return True

        def temporal_block(self, *a, **kw):
            calls.append("temporal_block")
            raise AssertionError("fyc_temporal_block has no rotation")

        def temporal_attention(self, qkv, o, **kw):
            calls.append("temporal_attention" if kw.get("rope") is not None else "temporal_attention without rope")
            return super().temporal_attention(qkv, o, **kw)
    g = load_golden(golden_dir, 16)
    eng = UNet3DEngine(pack_unet(rope_weights(0), rope_cfg(16), torch.bfloat16, "cpu"), ops=Eager())
    engine_forward(eng, g, torch.bfloat16)
    assert set(calls) == {"temporal_attention"} and len(calls) == 40, calls[:5]


# ---- schema and drop-in ------------------------------------------------------------------------------------------------------------
def test_schema_matches_reference(golden_dir):
    with open(os.path.join(golden_dir, "schema_unet_tiny_rope.json")) as f:
        ref = json.load(f)
    mine = unet_schema(rope_cfg(16))
    assert {k: list(v) for k, v in mine.items()} == ref          # same names and shapes (load_state_dict is order-independent)
    assert not any(k.endswith("pos_encoder.pe") for k in mine)
    assert sum(k.endswith("rope.em.inv_freq") for k in mine) == 40


@pytest.fixture()
def dropin():
    import followyourclick_amd
    followyourclick_amd.install_dropin(force=True)
    yield
    for name in [k for k in sys.modules if k.split(".")[0] in ("animatediff", "diffusers", "ip_adapter")]:
        del sys.modules[name]


def test_dropin_accepts_rope_options(dropin, golden_dir):
    from animatediff.models.unet import UNet3DConditionModel
    unet = UNet3DConditionModel(**TINY, motion_module_kwargs=dict(MM, video_length=40, train_video_length=16), compute_dtype=torch.float32)
    cfg = unet.engine_config
    assert cfg.use_rope_position_encoding and cfg.rope_video_length == 40 and cfg.rope_train_video_length == 16
    d16 = UNet3DConditionModel(**TINY, motion_module_kwargs=MM, compute_dtype=torch.float32).engine_config       # both lengths default to 16
    assert (d16.rope_video_length, d16.rope_train_video_length) == (16, 16)
    with open(os.path.join(golden_dir, "schema_unet_tiny_rope.json")) as f:
        ref = json.load(f)
    sd = unet.state_dict()
    assert {k: list(v.shape) for k, v in sd.items()} == ref
    # the buffers carry the formula's values, like the reference's constructor
    k = "down_blocks.1.motion_modules.0.temporal_transformer.transformer_blocks.0.attention_blocks.1.rope.em.inv_freq"
    assert torch.equal(sd[k], 1.0 / (10000.0 ** (torch.arange(0, 16, 2).float() / 16)))
    # a reference-style state dict (every key of the reference module, inv_freq included) loads strictly
    full = dict(rope_weights(0))
    full.update({k: torch.full(tuple(s), 0.5) for k, s in ref.items() if k.endswith("rope.em.inv_freq")})
    unet.load_state_dict({k: full[k] for k in ref}, strict=True)


def test_dropin_still_refuses_temporal_lora(dropin):
    from animatediff.models.unet import UNet3DConditionModel
    with pytest.raises(NotImplementedError, match="add_temporal_lora"):
        UNet3DConditionModel(**TINY, motion_module_kwargs=dict(MM, add_temporal_lora=True))
