"""Without the two native additions (fyc_repeat, q_batch_mod) the engine keeps the plain schedule: the op emulator (tests/emu_ops.py)
has neither, nor the direct statistics fold, and would raise a TypeError on any keyword it does not know."""
import os

import numpy as np
import pytest
import torch

from emu_ops import EmuOps
from followyourclick_amd.engine import DDIMConfig, UNet3DConfig
from followyourclick_amd.engine.sampler import DDIMSampler
from followyourclick_amd.engine.unet3d import UNet3DEngine
from followyourclick_amd.engine.weights import pack_unet
from oracle import functional as Fn
from oracle import weights as W


def tiny_cfg(**kw):
    return UNet3DConfig(block_out_channels=(64, 128, 256, 256), cross_attention_dim=64, sample_size=8, **kw)


def _load(golden_dir, name):
    return {k: torch.from_numpy(v) if v.shape else v for k, v in np.load(os.path.join(golden_dir, name)).items()}


class Counting(EmuOps):
    def __init__(self):
        super().__init__()
        self.seen = []

    def __getattribute__(self, name):
        v = object.__getattribute__(self, name)
        if callable(v) and not name.startswith("_") and name != "seen":
            object.__getattribute__(self, "seen").append(name)
        return v


def test_emulator_lacks_the_new_ops_and_forward_takes_the_plain_schedule(golden_dir):
    g = _load(golden_dir, "unet_tiny_fwd.npz")
    ops = Counting()
    assert not hasattr(EmuOps, "repeat") and not hasattr(EmuOps, "attention_q_batch_mod_supported") and not hasattr(EmuOps, "direct_stats_supported")
    sd = W.make_weights(W.unet_state_shapes(Fn.tiny_unet_config()), int(g["weight_seed"]))
    eng = UNet3DEngine(pack_unet(sd, tiny_cfg(), torch.float32, "cpu"), ops=ops)
    assert not eng.direct_stats
    x9 = g["sample"]
    B, C9, F, H, Wd = x9.shape
    assert B == 2 and torch.equal(x9[0], x9[1])
    x = torch.zeros(B * F * H * Wd, 64)
    x[:, :C9] = x9.permute(0, 2, 3, 4, 1).reshape(-1, C9)
    eng.prepare_context(g["text"])
    _, temb = eng.prepare_time_embeddings([int(g["timestep"])], g["fps"].tolist(), g["flow"].tolist(), B)
    assert not eng.shares_prefix(B)
    ops.seen.clear()
    plain = eng.forward(x, temb, B, F, H, Wd)
    seen_plain = [n for n in ops.seen if n != "ensure_init"]
    ops.seen.clear()
    half = eng.forward(x[: x.shape[0] // 2], temb, B, F, H, Wd, shared_prefix=2)       # the distinct half only: duplicated by the fall-back
    assert eng.last_schedule == "plain"
    assert [n for n in ops.seen if n != "ensure_init"] == seen_plain                   # op for op the plain schedule
    assert torch.equal(half, plain)
    out = plain.reshape(B, F, H, Wd, 4).permute(0, 4, 1, 2, 3)
    assert ((out - g["out"]).norm() / g["out"].norm()).item() < 2e-4


def test_sampler_on_the_emulator_duplicates_the_input(golden_dir):
    """DDIMSampler.step asks the engine before it leaves out the CFG duplicate: on the emulator the input is built twice, as before"""
    g = _load(golden_dir, "pipeline_tiny.npz")
    sd = W.make_weights(W.unet_state_shapes(Fn.tiny_unet_config()), int(g["unet_weight_seed"]))
    seen = []

    class Spy(EmuOps):
        def unet_input(self, *a, **kw):
            seen.append(kw["cfg_dup"])
            return super().unet_input(*a, **kw)
    eng = UNet3DEngine(pack_unet(sd, tiny_cfg(), torch.float32, "cpu"), ops=Spy())
    traj = []
    DDIMSampler(eng, DDIMConfig()).sample(g["latents"], g["text_embeddings"], 2, 8.0, g["first_image_latents"], g["first_images_mask"], fps=[2], flow=[4],
                                          callback=lambda i, t, l: traj.append(l.clone()))
    assert seen == [2, 2] and eng.last_schedule == "plain" and len(traj) == 2


class SharingEmu(EmuOps):
    """the emulator plus a specification of the two native additions: the shared schedule itself can then run on the CPU"""

    def attention_q_batch_mod_supported(self):
        return True

    def repeat(self, src, dst, *, times):
        assert src.dtype == dst.dtype and dst.numel() == times * src.numel()
        dst.reshape(times, -1).copy_(src.reshape(1, -1).expand(times, -1))

    def attention(self, q, k, vt, o, *, q_batch_mod=0, **kw):
        if q_batch_mod:
            q = q.reshape(q_batch_mod, -1)[torch.arange(kw["batch"]) % q_batch_mod].reshape(kw["batch"], *q.shape[1:])
        return super().attention(q, k, vt, o, **kw)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-4), (torch.bfloat16, 6e-2)])
def test_shared_schedule_on_the_emulator_matches_golden(golden_dir, monkeypatch, dtype, tol):
    """the engine-side wiring of the shared prefix (which tensors are broadcast, which time-embedding rows the prefix reads, where the
    batch doubles) against the reference golden of the duplicated batch; FYC_CFG_SHARE=0 turns it off"""
    from followyourclick_amd.engine import unet3d
    g = _load(golden_dir, "unet_tiny_fwd.npz")
    sd = W.make_weights(W.unet_state_shapes(Fn.tiny_unet_config()), int(g["weight_seed"]))
    eng = UNet3DEngine(pack_unet(sd, tiny_cfg(), dtype, "cpu"), ops=SharingEmu())
    x9 = g["sample"][:1]
    _, C9, F, H, Wd = x9.shape
    x = torch.zeros(F * H * Wd, 64)
    x[:, :C9] = x9.permute(0, 2, 3, 4, 1).reshape(-1, C9)
    eng.prepare_context(g["text"])
    _, temb = eng.prepare_time_embeddings([int(g["timestep"])], g["fps"].tolist(), g["flow"].tolist(), 2)
    assert eng.shares_prefix(2) and not eng.shares_prefix(3) and not eng.shares_prefix(2, temb[:1])
    out = eng.forward(x.to(dtype), temb, 2, F, H, Wd, shared_prefix=2)
    assert eng.last_schedule == "shared"
    out = out.float().reshape(2, F, H, Wd, 4).permute(0, 4, 1, 2, 3)
    rel = ((out - g["out"]).norm() / g["out"].norm()).item()
    assert rel < tol, rel
    monkeypatch.setattr(unet3d, "CFG_SHARE", False)
    assert not eng.shares_prefix(2)
