"""Golden vectors of clips of more than 64 frames, from the REAL reference (build container only; needs the reference tree that
oracle/refshim.py resolves).

Run:  python tools/make_golden_long.py

Writes to tests/golden/:
  unet_tiny_rope_f96.npz    one UNet3DConditionModel.forward of tools/make_golden_rope.py's model (use_rope_postion_encoding) built for
                            video_length 96 against train_video_length 16 (queries scaled by ln 16 / ln 96), 96 frames
  unet_tiny_pe128_f80.npz   the same tiny model with the sinusoidal table, temporal_position_encoding_max_len = 128, 80 frames

Weights are not stored: both models take W.make_weights(W.unet_state_shapes(tiny), 0) without the pos_encoder.pe keys (those draw nothing
from the generator), as tools/make_golden_rope.py's do.  The rotary model's inv_freq buffers and the sinusoidal model's pe buffers keep the
constructor's values (load_state_dict(strict=False)).  One clip per file (sample 1 x 9 x F x 8 x 8) keeps the files small."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import functional as Fn      # noqa: E402
from oracle import refshim               # noqa: E402
from oracle import weights as W          # noqa: E402
from oracle.make_golden import MM_KW     # noqa: E402
from make_golden_rope import INPUT_SEED, TRAIN_LENGTH, WEIGHT_SEED, ref_unet_rope      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
PE_MAX_LEN = 128


def ref_unet_pe(cfg: Fn.UNetConfig, max_len: int):
    from animatediff.models.unet import UNet3DConditionModel
    return UNet3DConditionModel(
        sample_size=cfg.sample_size, in_channels=cfg.in_channels, out_channels=cfg.out_channels,
        block_out_channels=cfg.block_out_channels, layers_per_block=cfg.layers_per_block,
        cross_attention_dim=cfg.cross_attention_dim, attention_head_dim=cfg.attention_head_dim,
        norm_num_groups=cfg.norm_num_groups, norm_eps=cfg.norm_eps, act_fn="silu", use_linear_projection=False,
        use_motion_module=True, motion_module_resolutions=(1, 2, 4, 8), unet_use_cross_frame_attention=False,
        unet_use_temporal_attention=False, use_fps_condition=True,
        use_first_frame_mask_condition_concat=cfg.use_first_frame_mask_condition_concat,
        motion_module_type="Vanilla", motion_module_kwargs=dict(MM_KW, temporal_position_encoding_max_len=max_len))


def main():
    refshim.install()
    cfg = Fn.tiny_unet_config()
    sd = {k: v for k, v in W.make_weights(W.unet_state_shapes(cfg), WEIGHT_SEED).items() if not k.endswith("pos_encoder.pe")}
    fps, flow = torch.tensor([2]), torch.tensor([4])
    for name, F, unet, kept, extra in (
            ("unet_tiny_rope_f96.npz", 96, ref_unet_rope(cfg, 96), "rope.em.inv_freq", dict(train_video_length=np.int64(TRAIN_LENGTH))),
            ("unet_tiny_pe128_f80.npz", 80, ref_unet_pe(cfg, PE_MAX_LEN), "pos_encoder.pe", dict(max_len=np.int64(PE_MAX_LEN)))):
        unet = unet.eval()
        missing, unexpected = unet.load_state_dict(sd, strict=False)
        assert not unexpected and missing and all(k.endswith(kept) for k in missing), (missing, unexpected)
        g = torch.Generator().manual_seed(INPUT_SEED)
        sample = torch.randn(1, 9, F, 8, 8, generator=g)
        text = torch.randn(1, 77, cfg.cross_attention_dim, generator=g)
        with torch.no_grad():
            out = unet(sample, torch.tensor(481), text, use_fps_condition=True, fps_tensor=fps, flow_control=flow).sample
        assert torch.isfinite(out).all()
        path = os.path.join(OUT, name)
        np.savez_compressed(path, sample=sample.numpy(), timestep=np.int64(481), text=text.numpy(), fps=fps.numpy(), flow=flow.numpy(),
                            out=out.numpy(), weight_seed=np.int64(WEIGHT_SEED), input_seed=np.int64(INPUT_SEED), F=np.int64(F), **extra)
        print(f"wrote {path} ({os.path.getsize(path) >> 10} KiB), |out| max {float(out.abs().max()):.3f}")


if __name__ == "__main__":
    main()
