"""The models behind the SD-2.1 family goldens (tools/make_golden_sd21.py): Linear proj_in / proj_out in the spatial transformers and one head
count per level, head dim 64 everywhere.  A helper, not a test module.

Weights are not stored: `sd21_weights(cfg, seed)` draws them in the order of the engine schema from ONE seeded generator - norm gains 1 + 0.1 N,
biases 0.05 N, matrices and kernels N(0, 1 / fan_in); tensors the reference's constructor zero-initialises (motion-module proj_out, the fps / motion
embeddings' linear_2, conv4 of the temporal blocks) are drawn like every other, or they would hide what sits behind them.  The positional tables
are analytic and draw nothing.  The generator loads exactly this dict into the reference with strict=True."""
import functools
import math
import os
from collections import OrderedDict

import numpy as np
import torch

from followyourclick_amd.engine import UNet3DConfig
from followyourclick_amd.engine.schema import unet_schema
from rope_spec import engine_forward, rel  # noqa: F401  (one forward helper for every tiny model)

WIDTHS, HEADS, CTX = (64, 128, 256, 256), (1, 2, 4, 4), 96
FULL_WIDTHS, FULL_HEADS, FULL_CTX = (320, 640, 1280, 1280), (5, 10, 20, 20), 1024
WEIGHT_SEED, INPUT_SEED, WEIGHT_SEED_2D, INPUT_SEED_2D = 21, 23, 25, 27
TOL_F32, TOL_16 = 1e-3, 5e-2      # the project's bounds for tiny-model forwards against reference goldens (tests/test_tconv.py, test_tconv_gpu.py)


def sd21_cfg(**kw) -> UNet3DConfig:
    base = dict(block_out_channels=WIDTHS, attention_head_dim=HEADS, cross_attention_dim=CTX, sample_size=8, use_linear_projection=True,
                use_inflated_groupnorm=True, motion_module_mid_block=True)
    base.update(kw)
    return UNet3DConfig(**base)


def sd21_cfg_2d(**kw) -> UNet3DConfig:
    """the 2-D UNet: the spatial half run as a one-frame clip - no motion modules, no fps / flow embeddings, 4 input channels"""
    return sd21_cfg(use_inflated_groupnorm=False, motion_module_mid_block=False, use_motion_module=False, use_fps_condition=False,
                    use_first_frame_mask_condition_concat=False, **kw)


def full_cfg() -> UNet3DConfig:
    return UNet3DConfig(block_out_channels=FULL_WIDTHS, attention_head_dim=FULL_HEADS, cross_attention_dim=FULL_CTX, sample_size=96,
                        use_linear_projection=True, use_inflated_groupnorm=True, motion_module_mid_block=True)


def pe_table(channels, length):
    """pe[p, 2i] = sin(p * exp(-2i ln(1e4) / C)), pe[p, 2i + 1] = cos(...) (reference motion_module.py:295-301)"""
    pos = torch.arange(length, dtype=torch.float32)[:, None]
    div = torch.exp(torch.arange(0, channels, 2, dtype=torch.float32) * (-math.log(10000.0) / channels))
    pe = torch.zeros(1, length, channels)
    pe[0, :, 0::2] = torch.sin(pos * div)
    pe[0, :, 1::2] = torch.cos(pos * div)
    return pe


def sd21_weights(cfg: UNet3DConfig, seed: int):
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for name, shape in unet_schema(cfg).items():
        if name.endswith("pos_encoder.pe"):
            sd[name] = pe_table(shape[2], shape[1])
            continue
        r = torch.randn(shape, generator=g, dtype=torch.float32)
        if name.endswith(".bias"):
            sd[name] = 0.05 * r
        elif len(shape) == 1:
            sd[name] = 1.0 + 0.1 * r
        else:
            sd[name] = r / math.sqrt(math.prod(shape[1:]))
    return sd


def is_spatial_proj(name: str) -> bool:
    return ".attentions." in name and name.endswith((".proj_in.weight", ".proj_out.weight"))


def conv_twin(sd):
    """the same numbers with proj_in / proj_out of the spatial transformers as (C, C, 1, 1) convolutions: the model without use_linear_projection"""
    return OrderedDict((k, v[:, :, None, None].clone() if is_spatial_proj(k) else v) for k, v in sd.items())


def load_golden(golden_dir, name):
    return {k: torch.from_numpy(v) if v.shape else v for k, v in np.load(os.path.join(golden_dir, name)).items()}


def load_json(golden_dir, name):
    """a fixture of tools/make_golden_sd21.py; the large ones are gzip-compressed"""
    import gzip
    import json
    path = os.path.join(golden_dir, name)
    with (gzip.open(path, "rt") if name.endswith(".gz") else open(path)) as f:
        return json.load(f)


def golden_name(F, tconv=False):
    return f"unet_tiny_sd21{'_tconv' if tconv else ''}_f{F}.npz"


MM = dict(num_attention_heads=8, num_transformer_block=1, attention_block_types=["Temporal_Self", "Temporal_Self"],
          temporal_position_encoding=True, temporal_position_encoding_max_len=24, temporal_attention_dim_div=1, zero_initialize=True)
# constructor arguments of the drop-in / the reference UNet3DConditionModel for the tiny model
TINY = dict(sample_size=8, in_channels=4, out_channels=4, block_out_channels=WIDTHS, layers_per_block=2, cross_attention_dim=CTX,
            attention_head_dim=list(HEADS), use_linear_projection=True, upcast_attention=True, use_inflated_groupnorm=True,
            use_motion_module=True, motion_module_resolutions=(1, 2, 4, 8), motion_module_mid_block=True,
            unet_use_cross_frame_attention=False, unet_use_temporal_attention=False, use_fps_condition=True,
            use_first_frame_mask_condition_concat=True, motion_module_type="Vanilla", motion_module_kwargs=MM)
TINY_2D = dict(sample_size=8, in_channels=4, out_channels=4, block_out_channels=WIDTHS, layers_per_block=2, cross_attention_dim=CTX,
               attention_head_dim=list(HEADS), use_linear_projection=True, upcast_attention=True)


def sd21_config_json(widths=FULL_WIDTHS, heads=FULL_HEADS, ctx=FULL_CTX, sample_size=96):
    """the fields of stable-diffusion-2-1's unet/config.json (written from its published model card), at the given widths"""
    return {"_class_name": "UNet2DConditionModel", "_diffusers_version": "0.10.0.dev0", "act_fn": "silu", "attention_head_dim": list(heads),
            "block_out_channels": list(widths), "center_input_sample": False, "cross_attention_dim": ctx,
            "down_block_types": ["CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"],
            "downsample_padding": 1, "dual_cross_attention": False, "flip_sin_to_cos": True, "freq_shift": 0, "in_channels": 4,
            "layers_per_block": 2, "mid_block_scale_factor": 1, "norm_eps": 1e-05, "norm_num_groups": 32, "num_class_embeds": None,
            "only_cross_attention": False, "out_channels": 4, "sample_size": sample_size,
            "up_block_types": ["UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"], "upcast_attention": True,
            "use_linear_projection": True}


# ---- the text encoder of the family: CLIP with hidden_act "gelu" (SD-2.1's OpenCLIP ViT-H text tower), at 2 layers, hidden 128, 2 heads of 64 ----
CLIP_GELU = dict(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=77,
                 hidden_act="gelu", layer_norm_eps=1e-5)


@functools.lru_cache(maxsize=None)
def clip_gelu_case():
    """(state dict, input ids [2][77], last_hidden_state of transformers.CLIPTextModel in f32): computed once, shared, never modified.  The weights
    follow the rule of sd21_weights (transformers' own initialisation has std 0.02: LayerNorm would carry the whole output)."""
    from transformers import CLIPTextConfig, CLIPTextModel
    model = CLIPTextModel(CLIPTextConfig(**CLIP_GELU, projection_dim=128, pad_token_id=1, bos_token_id=0, eos_token_id=2)).eval()
    g = torch.Generator().manual_seed(29)
    sd = OrderedDict()
    for name, p in model.state_dict().items():
        if not p.is_floating_point():
            sd[name] = p.clone()
            continue
        r = torch.randn(p.shape, generator=g)
        if "embedding" in name:
            sd[name] = 0.5 * r
        elif name.endswith(".bias"):
            sd[name] = 0.05 * r
        elif p.dim() == 1:
            sd[name] = 1.0 + 0.1 * r
        else:
            sd[name] = r / math.sqrt(p.shape[1])
    model.load_state_dict(sd, strict=True)
    ids = torch.randint(3, CLIP_GELU["vocab_size"], (2, 77), generator=g)
    ids[:, 0], ids[0, 30:], ids[1, 76] = 0, 2, 2          # bos; an early and a late eos
    with torch.no_grad():
        ref = model(input_ids=ids).last_hidden_state.float()
    assert torch.isfinite(ref).all()
    return sd, ids, ref
