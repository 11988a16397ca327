"""What tests/test_long_clip.py and tests/test_long_clip_gpu.py share: the two models behind the long-clip goldens of the real reference
(tools/make_golden_long.py) and the bounds both files judge the tiny UNet forward by.  A helper, not a test module.

  "rope96"   unet_tiny_rope_f96.npz: tests/rope_spec.py's rotary model built for video_length 96 against train_video_length 16, 96 frames
  "pe128"    unet_tiny_pe128_f80.npz: the same tiny model with the sinusoidal table, temporal_position_encoding_max_len = 128, 80 frames

TOL: f32 1e-3 as tests/test_rope.py.  16-bit: the project's 5e-2 (tests/test_engine_gpu.py) stands when the engine on the op emulator in that
type is at most half of it from the golden; tests/test_long_clip.py::test_engine_on_emulator_16bit measures that (its docstring has the values)
and asserts the precondition."""
import os

import numpy as np
import torch

import rope_spec
from emu_ops import EmuOps
from followyourclick_amd.engine import UNet3DConfig
from rope_spec import MM, rope_cfg

GOLDENS = {"rope96": ("unet_tiny_rope_f96.npz", 96), "pe128": ("unet_tiny_pe128_f80.npz", 80)}
TOL = {torch.float32: 1e-3, torch.bfloat16: 5e-2, torch.float16: 5e-2}
PE_MAX_LEN = 128


def cfg_of(which, **kw):
    if which == "rope96":
        return rope_cfg(96, **kw)
    return UNet3DConfig(block_out_channels=(64, 128, 256, 256), cross_attention_dim=64, sample_size=8, temporal_position_encoding_max_len=PE_MAX_LEN, **kw)


class LongRopeEmuOps(rope_spec.RopeEmuOps):
    """RopeEmuOps as the specification of a backend with the long-clip kernel: the engine asks its backend for the longest clip of the rotary
    temporal attention (HipOps.temporal_attention_max_frames) and takes 64 frames where the backend does not say"""
    temporal_attention_max_frames = 256


def emu_of(which):
    return LongRopeEmuOps() if which == "rope96" else EmuOps()


def motion_kwargs(which):
    """motion_module_kwargs of the drop-in UNet3DConditionModel"""
    if which == "rope96":
        return dict(MM, video_length=96, train_video_length=16)
    return dict(MM, use_rope_postion_encoding=False, temporal_position_encoding_max_len=PE_MAX_LEN)


def load(golden_dir, which):
    name, F = GOLDENS[which]
    g = {k: torch.from_numpy(v) if v.shape else v for k, v in np.load(os.path.join(golden_dir, name)).items()}
    assert int(g["F"]) == F and g["sample"].shape == (1, 9, F, 8, 8)
    return g
