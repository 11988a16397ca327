"""Golden vectors of the SD-2.1 UNet family (Linear proj_in / proj_out, one head count per level), from the REAL reference (build container only;
needs the reference tree that oracle/refshim.py resolves).

Run:  python tools/make_golden_sd21.py

Writes to tests/golden/:
  unet_tiny_sd21_f5.npz, _f16.npz   one UNet3DConditionModel.forward of the tiny model of tests/sd21_spec.py: widths (64,128,256,256), heads (1,2,4,4)
                                    = head dim 64 at every level, context 96, use_linear_projection, upcast_attention, use_inflated_groupnorm,
                                    a mid-block motion module, fps conditioning, 9-channel input
  unet_tiny_sd21_tconv_f5.npz       the same with use_temporal_conv
  schema_unet_tiny_sd21.json.gz      state-dict names -> shapes of the tiny model
  schema_unet_sd21_full.json.gz      ... of the reference at (320,640,1280,1280), heads (5,10,20,20), context 1024 (built on the meta device)
  sd2d_unet_sd21_fwd.npz            one UNet2DConditionModel.forward of the tiny configuration
  convert_keymap_sd21.json.gz        [ldm_key, diffusers_key, shape_after] of the reference's convert_ldm_unet_checkpoint for a synthetic SD-2.x LDM
                                    state dict (2-D proj_in / proj_out weights) and a config with use_linear_projection
  sd21_yaml_unet_kwargs.json        the distinct `unet_additional_kwargs` of the reference's YAMLs that set use_linear_projection, each with the
                                    names of the YAMLs that carry it (settings only)

The three large JSON fixtures are written gzip-compressed (compact separators, mtime 0: the bytes depend on the content alone); tests/sd21_spec.py::
load_json reads them.

Weights are not stored: tests/sd21_spec.py::sd21_weights draws them from the engine schema and they load into the reference with strict=True.
Each forward golden stores four control numbers, asserted here: the rel-L2 distance of the same reference with attention_head_dim[0] at every
level (`ctl_heads0`) and with 8 heads at every level (`ctl_heads8`), both >= 50x the f32 test bound; without upcast_attention (`ctl_no_upcast`,
exactly 0 in f32); and of the conv-projection twin (`ctl_conv_twin`, < 1e-5)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import refshim                                   # noqa: E402
from oracle.make_golden_convert import ldm_unet_keys        # noqa: E402
import sd21_spec as S                                        # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def dump_json_gz(name, obj):
    import gzip
    path = os.path.join(OUT, name)
    with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
        f.write(json.dumps(obj, separators=(",", ":")).encode())
    return path


def ref_unet(**over):
    from animatediff.models.unet import UNet3DConditionModel
    kw = dict(S.TINY, act_fn="silu", norm_num_groups=32, norm_eps=1e-5)
    kw.update(over)
    return UNet3DConditionModel(**kw)


def rel(a, b):
    return float((a - b).norm() / b.norm())


def forward_goldens(tconv: bool, frames):
    cfg = S.sd21_cfg(use_temporal_conv=tconv)
    sd = S.sd21_weights(cfg, S.WEIGHT_SEED)
    assert all(float(v.abs().max()) > 0 for v in sd.values())
    twin = S.conv_twin(sd)

    def model(weights=sd, **over):
        m = ref_unet(use_temporal_conv=tconv, **over).eval()
        m.load_state_dict(weights, strict=True)                # no missing and no unexpected keys
        return m
    unet = model()
    assert {k: tuple(v.shape) for k, v in unet.state_dict().items()} == {k: tuple(v) for k, v in S.unet_schema(cfg).items()}
    if not tconv:
        dump_json_gz("schema_unet_tiny_sd21.json.gz", {k: list(v.shape) for k, v in unet.state_dict().items()})
    controls = dict(ctl_heads0=model(attention_head_dim=S.HEADS[0]), ctl_heads8=model(attention_head_dim=8),
                    ctl_no_upcast=model(upcast_attention=False), ctl_conv_twin=model(twin, use_linear_projection=False))
    fps, flow = torch.tensor([2, 2]), torch.tensor([4, 4])
    for F in frames:
        g = torch.Generator().manual_seed(S.INPUT_SEED)
        sample = torch.randn(2, 9, F, 8, 8, generator=g)
        text = torch.randn(2, 77, S.CTX, generator=g)

        def run(m):
            with torch.no_grad():
                return m(sample, torch.tensor(481), text, use_fps_condition=True, fps_tensor=fps, flow_control=flow).sample
        out = run(unet)
        assert torch.isfinite(out).all()
        ctl = {k: rel(run(m), out) for k, m in controls.items()}
        assert ctl["ctl_heads0"] >= 50 * S.TOL_F32 and ctl["ctl_heads8"] >= 50 * S.TOL_F32, ctl
        assert ctl["ctl_no_upcast"] == 0.0 and ctl["ctl_conv_twin"] < 1e-5, ctl
        path = os.path.join(OUT, S.golden_name(F, tconv))
        np.savez_compressed(path, sample=sample.numpy(), timestep=np.int64(481), text=text.numpy(), fps=fps.numpy(), flow=flow.numpy(),
                            out=out.numpy(), weight_seed=np.int64(S.WEIGHT_SEED), input_seed=np.int64(S.INPUT_SEED), F=np.int64(F),
                            **{k: np.float64(v) for k, v in ctl.items()})
        print(f"wrote {path} ({os.path.getsize(path) >> 10} KiB), |out| max {float(out.abs().max()):.3f}, " +
              ", ".join(f"{k} {v:.3e}" for k, v in ctl.items()))


def full_schema():
    from animatediff.models.unet import UNet3DConditionModel
    kw = dict(S.TINY, block_out_channels=S.FULL_WIDTHS, attention_head_dim=list(S.FULL_HEADS), cross_attention_dim=S.FULL_CTX, sample_size=96)
    with torch.device("meta"):
        unet = UNet3DConditionModel(**kw)
    shapes = {k: list(v.shape) for k, v in unet.state_dict().items()}
    path = dump_json_gz("schema_unet_sd21_full.json.gz", shapes)
    print(f"wrote {path}: {len(shapes)} entries, {os.path.getsize(path) >> 10} KiB")


def forward_2d():
    from diffusers.models.unet_2d_condition import UNet2DConditionModel
    cfg = S.sd21_cfg_2d()
    sd = S.sd21_weights(cfg, S.WEIGHT_SEED_2D)
    unet = UNet2DConditionModel(**S.TINY_2D).eval()
    unet.load_state_dict(sd, strict=True)
    g = torch.Generator().manual_seed(S.INPUT_SEED_2D)
    x = torch.randn(2, 4, 8, 8, generator=g)
    text = torch.randn(2, 77, S.CTX, generator=g)
    with torch.no_grad():
        y = unet(x, torch.tensor(481), text).sample
        uni = UNet2DConditionModel(**dict(S.TINY_2D, attention_head_dim=S.HEADS[0])).eval()
        uni.load_state_dict(sd, strict=True)
        ctl = rel(uni(x, torch.tensor(481), text).sample, y)
    assert torch.isfinite(y).all() and ctl >= 50 * S.TOL_F32, ctl
    path = os.path.join(OUT, "sd2d_unet_sd21_fwd.npz")
    np.savez_compressed(path, sample=x.numpy(), text=text.numpy(), timestep=np.int64(481), out=y.numpy(), weight_seed=np.int64(S.WEIGHT_SEED_2D),
                        ctl_heads0=np.float64(ctl))
    print(f"wrote {path} ({os.path.getsize(path) >> 10} KiB), ctl_heads0 {ctl:.3e}")


def convert_keymap():
    from animatediff.utils import convert_from_ckpt as C
    src = {}
    for i, k in enumerate(ldm_unet_keys()):
        lin = k.endswith((".1.proj_in.weight", ".1.proj_out.weight"))        # SD-2.x: Linear projections, 2-D in the LDM file as well
        src[k] = torch.full((2, 2) if lin else (2,), float(i))
    src["cond_stage_model.model.ln_final.weight"] = torch.full((2,), -1.0)    # foreign keys are ignored
    cfg = {"layers_per_block": 2, "class_embed_type": None, "use_linear_projection": True}
    out = C.convert_ldm_unet_checkpoint(dict(src), cfg)
    by_tag = {float(v.flatten()[0]): k for k, v in src.items()}
    triples = sorted([by_tag[float(v.flatten()[0])], k, list(v.shape)] for k, v in out.items())
    path = dump_json_gz("convert_keymap_sd21.json.gz", {"unet": triples, "src_shapes": {k: list(v.shape) for k, v in src.items()}})
    print(f"wrote {path}: {len(triples)} keys, {os.path.getsize(path) >> 10} KiB")


def yaml_kwargs():
    import glob
    import yaml
    seen = {}
    for f in sorted(glob.glob(os.path.join(refshim.REFERENCE_ROOT, "configs", "**", "*.yaml"), recursive=True)):
        y = yaml.safe_load(open(f))
        kw = y.get("unet_additional_kwargs") if isinstance(y, dict) else None
        if isinstance(kw, dict) and kw.get("use_linear_projection"):
            assert "stable-diffusion-2-1" in str(y.get("pretrained_model_path")), f
            seen.setdefault(json.dumps(kw, sort_keys=True), []).append(os.path.basename(f))
    out = [{"yamls": names, "unet_additional_kwargs": json.loads(k)} for k, names in seen.items()]
    assert sum(len(e["yamls"]) for e in out) == 15
    path = os.path.join(OUT, "sd21_yaml_unet_kwargs.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e, sort_keys=True) for e in out) + "\n]\n")
    print(f"wrote {path}: {len(out)} distinct settings of 15 YAMLs")


def main():
    refshim.install()
    yaml_kwargs()
    forward_goldens(False, (5, 16))
    forward_goldens(True, (5,))
    full_schema()
    forward_2d()
    convert_keymap()


if __name__ == "__main__":
    main()
