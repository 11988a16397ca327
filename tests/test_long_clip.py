"""Clips of more than 64 frames without a GPU: the engine on the op emulator against goldens of the real reference (tools/make_golden_long.py;
the models: tests/long_clip_spec.py) in f32 and in the emulated 16-bit types, and the two refusals - more than 256 frames under RoPE, and a
sinusoidal clip longer than its positional table."""
import pytest
import torch

import long_clip_spec as S
import rope_spec
from rope_spec import engine_forward, rel, rope_cfg, rope_weights
from followyourclick_amd.engine.unet3d import UNet3DEngine
from followyourclick_amd.engine.weights import pack_unet


def _engine(which, g, dtype):
    return UNet3DEngine(pack_unet(rope_weights(int(g["weight_seed"])), S.cfg_of(which), dtype, "cpu"), ops=S.emu_of(which))


@pytest.mark.parametrize("which", ["rope96", "pe128"])
def test_engine_on_emulator_matches_reference_golden(golden_dir, which):
    """f32, bound 1e-3 as tests/test_rope.py.  Measured: rope96 2.0e-6, pe128 1.6e-6."""
    g = S.load(golden_dir, which)
    r = rel(engine_forward(_engine(which, g, torch.float32), g), g["out"])
    print(f"long-clip engine on the emulator, {which}: rel-L2 {r:.3e}")
    assert r < S.TOL[torch.float32], r


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("which", ["rope96", "pe128"])
def test_engine_on_emulator_16bit(golden_dir, which, dtype):
    """The engine on the emulator with 16-bit storage against the f32 golden.  Measured rel-L2: rope96 bf16 1.81e-2, f16 2.3e-3; pe128 bf16
    1.44e-2, f16 1.7e-3.  All are at most half of the project's 5e-2, so that bound stands for the GPU runs (long_clip_spec.TOL); this test
    holds the precondition."""
    g = S.load(golden_dir, which)
    r = rel(engine_forward(_engine(which, g, dtype), g, dtype), g["out"])
    print(f"long-clip engine on the emulator, {which} {dtype}: rel-L2 {r:.3e}")
    assert r <= S.TOL[dtype] / 2, r


def test_more_than_256_frames_is_refused():
    """the limit is the backend's: 256 frames where it has the long-clip kernel, 64 where it does not say (tests/test_rope.py holds that case)"""
    eng = UNet3DEngine(pack_unet(rope_weights(0), rope_cfg(16), torch.float32, "cpu"), ops=S.LongRopeEmuOps())
    with pytest.raises(ValueError, match="256 frames"):
        eng._rope(8, 257)
    cos, sin = eng._rope(8, 256)
    assert cos.shape == (256, 4) and sin.shape == (256, 4)


def test_sinusoidal_clip_longer_than_its_table_is_refused(golden_dir):
    """temporal_position_encoding_max_len = 128: 80 frames run (the golden above), 129 do not"""
    g = dict(S.load(golden_dir, "pe128"))
    eng = _engine("pe128", g, torch.float32)
    g["sample"] = torch.zeros(1, 9, S.PE_MAX_LEN + 1, 8, 8)
    with pytest.raises(ValueError, match=r"video_length 129 exceeds the positional table \(128\)"):
        engine_forward(eng, g)
