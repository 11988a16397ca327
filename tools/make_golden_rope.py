"""Golden vectors of the RoPE motion module, from the REAL reference (build container only; needs the reference tree that
oracle/refshim.py resolves).

Run:  python tools/make_golden_rope.py

Writes to tests/golden/:
  unet_tiny_rope_f16.npz   one UNet3DConditionModel.forward of the tiny config built with use_rope_postion_encoding, 16 frames
  unet_tiny_rope_f40.npz   the same model built for video_length 40 against train_video_length 16 (queries scaled by ln 16 / ln 40), 40 frames
  schema_unet_tiny_rope.json   state-dict names -> shapes of that model (no pos_encoder.pe, 40 rope.em.inv_freq buffers)

The model is oracle/make_golden.py::ref_unet's for tiny_unet_config() with other motion_module_kwargs.  Weights are not stored: they are
W.make_weights(W.unet_state_shapes(tiny), 0) without the pos_encoder.pe keys (those draw nothing from the generator, so every other tensor
equals the one behind unet_tiny_fwd.npz).  The inv_freq buffers keep the constructor's values (load_state_dict(strict=False))."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import functional as Fn      # noqa: E402
from oracle import refshim               # noqa: E402
from oracle import weights as W          # noqa: E402
from oracle.make_golden import MM_KW     # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
TRAIN_LENGTH, MAX_LEN, WEIGHT_SEED, INPUT_SEED = 16, 32, 0, 9


def ref_unet_rope(cfg: Fn.UNetConfig, video_length: int):
    from animatediff.models.unet import UNet3DConditionModel
    mm = dict(MM_KW, use_rope_postion_encoding=True, temporal_position_encoding_max_len=MAX_LEN, video_length=video_length,
              train_video_length=TRAIN_LENGTH)
    return UNet3DConditionModel(
        sample_size=cfg.sample_size, in_channels=cfg.in_channels, out_channels=cfg.out_channels,
        block_out_channels=cfg.block_out_channels, layers_per_block=cfg.layers_per_block,
        cross_attention_dim=cfg.cross_attention_dim, attention_head_dim=cfg.attention_head_dim,
        norm_num_groups=cfg.norm_num_groups, norm_eps=cfg.norm_eps, act_fn="silu", use_linear_projection=False,
        use_motion_module=True, motion_module_resolutions=(1, 2, 4, 8), unet_use_cross_frame_attention=False,
        unet_use_temporal_attention=False, use_fps_condition=True,
        use_first_frame_mask_condition_concat=cfg.use_first_frame_mask_condition_concat,
        motion_module_type="Vanilla", motion_module_kwargs=mm)


def main():
    refshim.install()
    cfg = Fn.tiny_unet_config()
    sd = {k: v for k, v in W.make_weights(W.unet_state_shapes(cfg), WEIGHT_SEED).items() if not k.endswith("pos_encoder.pe")}
    fps, flow = torch.tensor([2, 2]), torch.tensor([4, 4])
    for F in (16, 40):
        unet = ref_unet_rope(cfg, F).eval()
        missing, unexpected = unet.load_state_dict(sd, strict=False)
        assert not unexpected and missing and all(k.endswith("rope.em.inv_freq") for k in missing), (missing, unexpected)
        if F == 16:
            with open(os.path.join(OUT, "schema_unet_tiny_rope.json"), "w") as f:
                json.dump({k: list(v.shape) for k, v in unet.state_dict().items()}, f, indent=0)
        g = torch.Generator().manual_seed(INPUT_SEED)
        sample = torch.randn(2, 9, F, 8, 8, generator=g)
        text = torch.randn(2, 77, cfg.cross_attention_dim, generator=g)
        with torch.no_grad():
            out = unet(sample, torch.tensor(481), text, use_fps_condition=True, fps_tensor=fps, flow_control=flow).sample
        assert torch.isfinite(out).all()
        path = os.path.join(OUT, f"unet_tiny_rope_f{F}.npz")
        np.savez_compressed(path, sample=sample.numpy(), timestep=np.int64(481), text=text.numpy(), fps=fps.numpy(), flow=flow.numpy(),
                            out=out.numpy(), weight_seed=np.int64(WEIGHT_SEED), input_seed=np.int64(INPUT_SEED), F=np.int64(F),
                            train_video_length=np.int64(TRAIN_LENGTH), max_len=np.int64(MAX_LEN))
        print(f"wrote {path} ({os.path.getsize(path) >> 10} KiB), |out| max {float(out.abs().max()):.3f}")


if __name__ == "__main__":
    main()
