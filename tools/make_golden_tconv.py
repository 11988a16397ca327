"""Golden vectors of the per-frame GroupNorm / temporal-conv UNet variant, from the REAL reference (build container only; needs the
reference tree that oracle/refshim.py resolves).

Run:  python tools/make_golden_tconv.py

Writes to tests/golden/:
  unet_tiny_tconv_f5.npz    one UNet3DConditionModel.forward of the tiny config built with use_inflated_groupnorm and use_temporal_conv, 5 frames
                            (odd: a row tile straddles frames at 8x8 and below)
  unet_tiny_tconv_f16.npz   the same model, 16 frames
  schema_unet_tiny_tconv.json   state-dict names -> shapes of that model (352 temporal_conv entries)

The model is oracle/make_golden.py::ref_unet's for tiny_unet_config() with the two options.  Weights are not stored: they are
W.make_weights(W.unet_state_shapes(tiny), weight_seed) plus the 352 temporal_conv tensors of tests/tconv_spec.py::tconv_extra_weights(extra_seed)
(conv4 NOT zero, or the block would be invisible).  Two control numbers are stored with each output: the rel-L2 distance of the same
reference model WITHOUT the temporal blocks (`ctl_no_tconv`) and with cross-frame instead of per-frame ResNet norms (`ctl_cross_frame`)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import functional as Fn      # noqa: E402
from oracle import refshim               # noqa: E402
from oracle.make_golden import MM_KW     # noqa: E402
import tconv_spec                        # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
WEIGHT_SEED, EXTRA_SEED, INPUT_SEED = 0, 11, 13


def ref_unet_tconv(cfg: Fn.UNetConfig, inflated: bool = True, tconv: bool = True):
    from animatediff.models.unet import UNet3DConditionModel
    return UNet3DConditionModel(
        sample_size=cfg.sample_size, in_channels=cfg.in_channels, out_channels=cfg.out_channels,
        block_out_channels=cfg.block_out_channels, layers_per_block=cfg.layers_per_block,
        cross_attention_dim=cfg.cross_attention_dim, attention_head_dim=cfg.attention_head_dim,
        norm_num_groups=cfg.norm_num_groups, norm_eps=cfg.norm_eps, act_fn="silu", use_linear_projection=False,
        use_motion_module=True, motion_module_resolutions=(1, 2, 4, 8), unet_use_cross_frame_attention=False,
        unet_use_temporal_attention=False, use_fps_condition=True,
        use_first_frame_mask_condition_concat=cfg.use_first_frame_mask_condition_concat,
        motion_module_type="Vanilla", motion_module_kwargs=dict(MM_KW),
        use_inflated_groupnorm=inflated, use_temporal_conv=tconv)


def rel(a, b):
    return float((a - b).norm() / b.norm())


def main():
    refshim.install()
    cfg = Fn.tiny_unet_config()
    sd = tconv_spec.tconv_weights(WEIGHT_SEED, EXTRA_SEED)
    extra = [k for k in sd if ".temporal_conv." in k]
    assert len(extra) == 352, len(extra)
    assert all(float(sd[k].abs().max()) > 0 for k in extra if ".conv4.3." in k)
    unet = ref_unet_tconv(cfg).eval()
    unet.load_state_dict(sd, strict=True)                      # no missing and no unexpected keys
    no_tconv = ref_unet_tconv(cfg, tconv=False).eval()
    no_tconv.load_state_dict({k: v for k, v in sd.items() if ".temporal_conv." not in k}, strict=True)
    cross = ref_unet_tconv(cfg, inflated=False).eval()
    cross.load_state_dict(sd, strict=True)
    with open(os.path.join(OUT, "schema_unet_tiny_tconv.json"), "w") as f:
        json.dump({k: list(v.shape) for k, v in unet.state_dict().items()}, f, indent=0)
    fps, flow = torch.tensor([2, 2]), torch.tensor([4, 4])
    for F in (5, 16):
        g = torch.Generator().manual_seed(INPUT_SEED)
        sample = torch.randn(2, 9, F, 8, 8, generator=g)
        text = torch.randn(2, 77, cfg.cross_attention_dim, generator=g)

        def run(m):
            with torch.no_grad():
                return m(sample, torch.tensor(481), text, use_fps_condition=True, fps_tensor=fps, flow_control=flow).sample
        out = run(unet)
        assert torch.isfinite(out).all()
        ctl_a, ctl_b = rel(run(no_tconv), out), rel(run(cross), out)
        path = os.path.join(OUT, f"unet_tiny_tconv_f{F}.npz")
        np.savez_compressed(path, sample=sample.numpy(), timestep=np.int64(481), text=text.numpy(), fps=fps.numpy(), flow=flow.numpy(),
                            out=out.numpy(), weight_seed=np.int64(WEIGHT_SEED), extra_seed=np.int64(EXTRA_SEED), input_seed=np.int64(INPUT_SEED),
                            F=np.int64(F), ctl_no_tconv=np.float64(ctl_a), ctl_cross_frame=np.float64(ctl_b))
        print(f"wrote {path} ({os.path.getsize(path) >> 10} KiB), |out| max {float(out.abs().max()):.3f}, "
              f"without the temporal blocks rel-L2 {ctl_a:.3f}, cross-frame norms rel-L2 {ctl_b:.3f}")


if __name__ == "__main__":
    main()
