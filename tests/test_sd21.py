"""The SD-2.1 UNet family (use_linear_projection, one head count per level, upcast_attention) without a GPU: the engine on the op emulator against
goldens of the real reference (tools/make_golden_sd21.py), the state-dict schema at the tiny and at the full width, the conv-projection twin, the
drop-in's constructors and loaders, the checkpoint converter, the gelu CLIP text encoder and the shared CFG prefix."""
import json
import os
import sys

import pytest
import torch

import sd21_spec as S
import trace_ops
from emu_ops import EmuOps
from sd21_spec import conv_twin, engine_forward, golden_name, load_golden, rel, sd21_cfg, sd21_weights
from tconv_spec import TconvEmuOps
from followyourclick_amd.engine import UNet3DConfig
from followyourclick_amd.engine import encoders as EN
from followyourclick_amd.engine.schema import unet_schema
from followyourclick_amd.engine.unet3d import UNet3DEngine
from followyourclick_amd.engine.weights import pack_unet

GOLDENS = [(5, False), (16, False), (5, True)]


def _engine(g, cfg, sd=None, ops=None, dtype=torch.float32):
    sd = sd if sd is not None else sd21_weights(cfg, int(g["weight_seed"]))
    return UNet3DEngine(pack_unet(sd, cfg, dtype, "cpu"), ops=ops or TconvEmuOps())


# ---- configuration -----------------------------------------------------------------------------------------------------------------------
def test_config_head_counts_per_level():
    cfg = S.full_cfg()
    assert [cfg.down_heads(i) for i in range(4)] == [5, 10, 20, 20] and cfg.mid_heads() == 20
    assert [cfg.up_heads(i) for i in range(4)] == [20, 20, 10, 5]
    cfg.validate()                                                   # head dim 64 at every level
    one = UNet3DConfig()                                             # an int keeps its meaning: that many heads everywhere
    assert [one.down_heads(i) for i in range(4)] == [8] * 4 and one.mid_heads() == 8 and [one.up_heads(i) for i in range(4)] == [8] * 4
    one.validate()
    with pytest.raises(ValueError, match="multiple of 8"):
        UNet3DConfig(attention_head_dim=(5, 10, 20, 3)).validate()   # 1280 / 3
    with pytest.raises(ValueError, match="160"):
        UNet3DConfig(attention_head_dim=(1, 10, 20, 20)).validate()  # head dim 320 where attention runs
    with pytest.raises(ValueError, match="160"):
        UNet3DConfig(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 1)).validate()   # the last entry is the mid block's: 256 / 1
    with pytest.raises(ValueError, match="entries"):
        UNet3DConfig(attention_head_dim=(5, 10, 20)).validate()


# ---- the engine on the emulator against the real reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("F,tconv", GOLDENS)
def test_engine_on_emulator_matches_reference_golden(golden_dir, F, tconv):
    g = load_golden(golden_dir, golden_name(F, tconv))
    assert int(g["F"]) == F and g["sample"].shape[2] == F
    cfg = sd21_cfg(use_temporal_conv=tconv)
    r = rel(engine_forward(_engine(g, cfg), g), g["out"])
    print(f"sd21 engine on the emulator, F={F} tconv={tconv}: rel-L2 {r:.3e}")
    assert r < S.TOL_F32, r
    # the controls stored with the fixture (the reference's own distances): the fixture sees the head layout, not upcast_attention, and the twin
    assert float(g["ctl_heads0"]) >= 50 * S.TOL_F32 and float(g["ctl_heads8"]) >= 50 * S.TOL_F32
    assert float(g["ctl_no_upcast"]) == 0.0 and float(g["ctl_conv_twin"]) < 1e-5
    if F == 5:      # and so does the engine: 8 heads everywhere is as far from the golden as the reference says
        r8 = rel(engine_forward(_engine(g, sd21_cfg(use_temporal_conv=tconv, attention_head_dim=8)), g), g["out"])
        print(f"  8 heads at every level: rel-L2 {r8:.3e} (reference {float(g['ctl_heads8']):.3e})")
        assert r8 > 0.5 * float(g["ctl_heads8"]), r8


def test_schema_matches_reference(golden_dir):
    ref = S.load_json(golden_dir, "schema_unet_tiny_sd21.json.gz")
    mine = unet_schema(sd21_cfg())
    assert {k: list(v) for k, v in mine.items()} == ref
    lin = [k for k in mine if S.is_spatial_proj(k)]
    assert len(lin) == 2 * 16 and all(len(mine[k]) == 2 for k in lin)
    conv = unet_schema(sd21_cfg(use_linear_projection=False))
    assert list(conv) == list(mine) and all(tuple(conv[k]) == tuple(mine[k]) + ((1, 1) if k in lin else ()) for k in mine)
    assert all(len(v) == 2 for k, v in mine.items() if ".temporal_transformer.proj_" in k and k.endswith(".weight"))      # motion modules: Linear as before


def test_full_width_schema_matches_reference(golden_dir):
    """(320, 640, 1280, 1280), heads (5, 10, 20, 20), context 1024: names and shapes only, no weights"""
    ref = S.load_json(golden_dir, "schema_unet_sd21_full.json.gz")
    cfg = S.full_cfg()
    cfg.validate()
    mine = unet_schema(cfg)
    assert {k: list(v) for k, v in mine.items()} == ref
    assert mine["down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_k.weight"] == (320, 1024)
    assert mine["mid_block.attentions.0.proj_in.weight"] == (1280, 1280)


def _trace(cfg, sd, share=1, B=2, F=4, H=32, Wd=32):
    ops = trace_ops.TraceOps(fused=True)
    eng = UNet3DEngine(pack_unet(sd, cfg, torch.bfloat16, "cpu"), ops=ops)
    eng.prepare_context(torch.zeros(B, 77, cfg.cross_attention_dim))
    _, temb = eng.prepare_time_embeddings([500], [2] * B, [4] * B, B)
    pre = ops.lines()
    ops.reset()
    eng.forward(torch.zeros(B // share * F * H * Wd, 64, dtype=torch.bfloat16), temb, B, F, H, Wd, shared_prefix=share)
    return pre, ops.lines(), ops.log


def test_conv_projection_twin_same_schedule_and_bits(golden_dir):
    """the same numbers as (C, C, 1, 1) convolutions and use_linear_projection off: one launch list, one output, bit for bit"""
    g = load_golden(golden_dir, golden_name(5))
    sd = sd21_weights(sd21_cfg(), int(g["weight_seed"]))
    twin = conv_twin(sd)
    assert sum(v.dim() == 4 and v.shape[2:] == (1, 1) for k, v in twin.items() if S.is_spatial_proj(k)) == 32
    a = engine_forward(_engine(g, sd21_cfg(), sd), g)
    b = engine_forward(_engine(g, sd21_cfg(use_linear_projection=False), twin), g)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    for share in (1, 2):
        la, lb = _trace(sd21_cfg(), sd, share), _trace(sd21_cfg(use_linear_projection=False), twin, share)
        assert la[0] == lb[0] and la[1] == lb[1] and len(la[1]) > 300


def test_schedule_uses_each_transformers_own_head_count():
    """every HEADS epilogue and every attention launch of transformer i carries heads = C / 64; the temporal attention keeps its 8 heads"""
    cfg = sd21_cfg()
    _, _, log = _trace(cfg, sd21_weights(cfg, 0))
    hd = [l.args["heads"] for l in log if l.op == "gemm" and l.args.get("heads") is not None]
    assert len(hd) == 2 * 16 and all(h["seg_cols"] == 64 * h["heads"] for h in hd)
    order = [1, 1, 2, 2, 4, 4, 4, 4, 4, 4, 2, 2, 2, 1, 1, 1]         # down 0 .. 2, mid, up 1 .. 3 (reversed list)
    assert [h["heads"] for h in hd[0::2]] == order and [h["heads"] for h in hd[1::2]] == order
    att = [l.args for l in log if l.op == "attention"]
    assert len(att) == 2 * 16 and all(a["d"] == 64 and a["ldo"] == 64 * a["heads"] for a in att)
    assert [a["heads"] for a in att[0::2]] == order
    tmp = [l.args for l in log if l.op in ("temporal_attention", "temporal_block")]
    assert tmp and all(a["heads"] == 8 for a in tmp)


# ---- shared CFG prefix -------------------------------------------------------------------------------------------------------------------
class SharingEmu(TconvEmuOps):
    """the emulator plus a specification of fyc_repeat and q_batch_mod (as tests/test_tconv.py): the shared schedule on the CPU"""

    def attention_q_batch_mod_supported(self):
        return True

    def repeat(self, src, dst, *, times):
        assert src.dtype == dst.dtype and dst.numel() == times * src.numel()
        dst.reshape(times, -1).copy_(src.reshape(1, -1).expand(times, -1))

    def attention(self, q, k, vt, o, *, q_batch_mod=0, **kw):
        if q_batch_mod:
            q = q.reshape(q_batch_mod, -1)[torch.arange(kw["batch"]) % q_batch_mod].reshape(kw["batch"], *q.shape[1:])
        return super().attention(q, k, vt, o, **kw)


def test_shared_prefix_equals_the_unshared_schedule(golden_dir):
    """the CFG pair with the prefix run once agrees with the duplicated batch (f32: 2e-4, the bound of tests/test_shared_prefix_emulated.py)"""
    g = load_golden(golden_dir, golden_name(5))
    eng = _engine(g, sd21_cfg(), ops=SharingEmu())
    x9 = g["sample"][:1]
    _, C9, F, H, Wd = x9.shape
    x = torch.zeros(F * H * Wd, 64)
    x[:, :C9] = x9.permute(0, 2, 3, 4, 1).reshape(-1, C9)
    eng.prepare_context(g["text"])
    _, temb = eng.prepare_time_embeddings([int(g["timestep"])], g["fps"].tolist(), g["flow"].tolist(), 2)
    assert eng.shares_prefix(2)
    shared = eng.forward(x, temb, 2, F, H, Wd, shared_prefix=2)
    assert eng.last_schedule == "shared"
    plain = eng.forward(torch.cat([x, x]), temb, 2, F, H, Wd)
    assert eng.last_schedule == "plain"
    r = rel(shared, plain)
    print(f"shared prefix vs duplicated batch: rel-L2 {r:.3e}")
    assert r < 2e-4, r
    assert not torch.equal(plain[: plain.shape[0] // 2], plain[plain.shape[0] // 2:])       # the halves differ (text states)


# ---- drop-in -----------------------------------------------------------------------------------------------------------------------------
def _purge():
    for name in [k for k in sys.modules if k.split(".")[0] in ("animatediff", "diffusers", "ip_adapter")]:
        del sys.modules[name]


@pytest.fixture()
def dropin(monkeypatch):
    import followyourclick_amd
    monkeypatch.setenv("FYC_UNET_VARIANTS", "1")          # the drop-in builds these model families on request only
    followyourclick_amd.install_dropin(force=True)
    yield
    _purge()


def test_dropin_builds_the_family_under_the_switch(dropin, golden_dir):
    from animatediff.models.unet import UNet3DConditionModel
    unet = UNet3DConditionModel(**S.TINY, compute_dtype=torch.float32)
    cfg = unet.engine_config
    assert cfg.use_linear_projection and cfg.attention_head_dim == S.HEADS and cfg.use_inflated_groupnorm and cfg.motion_module_mid_block
    # `.config` round-trips the constructor arguments as they were given
    assert unet.config.attention_head_dim == list(S.HEADS) and unet.config.use_linear_projection is True and unet.config.upcast_attention is True
    again = UNet3DConditionModel.from_config(vars(unet.config), compute_dtype=torch.float32)
    assert again.engine_config == cfg
    ref = S.load_json(golden_dir, "schema_unet_tiny_sd21.json.gz")
    assert {k: list(v.shape) for k, v in unet.state_dict().items()} == ref
    full = sd21_weights(sd21_cfg(), S.WEIGHT_SEED)
    unet.load_state_dict(full, strict=True)
    back = unet.state_dict()
    assert all(torch.equal(back[k], full[k]) for k in ref)
    # upcast_attention changes nothing: same engine configuration, same schema
    off = UNet3DConditionModel(**dict(S.TINY, upcast_attention=False), compute_dtype=torch.float32)
    assert off.engine_config == cfg and off.config.upcast_attention is False
    # the module's weights through the engine on the emulator == the golden
    g = load_golden(golden_dir, golden_name(5))
    eng = UNet3DEngine(pack_unet(unet.state_dict(), unet.engine_config, torch.float32, "cpu"), ops=TconvEmuOps())
    assert rel(engine_forward(eng, g), g["out"]) < S.TOL_F32


def test_dropin_refuses_the_family_without_the_switch(dropin, monkeypatch):
    from animatediff.models.unet import UNet3DConditionModel
    monkeypatch.delenv("FYC_UNET_VARIANTS")
    base = {k: v for k, v in S.TINY.items() if k not in ("use_linear_projection", "attention_head_dim", "use_inflated_groupnorm")}
    for opts, named in ((dict(use_linear_projection=True, attention_head_dim=8), "use_linear_projection"),
                        (dict(attention_head_dim=list(S.HEADS)), "attention_head_dim"),
                        (dict(attention_head_dim=tuple(S.HEADS)), "attention_head_dim"),
                        (dict(use_linear_projection=True, attention_head_dim=list(S.HEADS)), "use_linear_projection")):
        with pytest.raises(NotImplementedError, match="FYC_UNET_VARIANTS=1") as e:
            UNet3DConditionModel(**base, **opts)
        assert named in str(e.value)
    # a list of equal entries is an int: no switch, the int's configuration; upcast_attention alone needs none either
    same = UNet3DConditionModel(**dict(base, attention_head_dim=[8, 8, 8, 8], upcast_attention=True), compute_dtype=torch.float32)
    assert same.engine_config == UNet3DConditionModel(**dict(base, attention_head_dim=8, upcast_attention=False), compute_dtype=torch.float32).engine_config
    assert same.engine_config.attention_head_dim == 8 and same.config.attention_head_dim == [8, 8, 8, 8]


def test_dropin_head_list_must_have_one_entry_per_block(dropin):
    from animatediff.models.unet import UNet3DConditionModel
    with pytest.raises(ValueError, match="entries"):
        UNet3DConditionModel(**dict(S.TINY, attention_head_dim=[1, 2, 4]))


def _tiny_sd21_dir(tmp_path):
    """a checkpoint directory shaped like stable-diffusion-2-1/unet: every field of its config.json (context 1024, sample_size 96, head list, the
    null / false options), at the tiny widths so that the weights stay small"""
    cfg_json = S.sd21_config_json(widths=S.WIDTHS, heads=S.HEADS)
    assert cfg_json["cross_attention_dim"] == 1024 and cfg_json["sample_size"] == 96 and cfg_json["num_class_embeds"] is None
    sd = sd21_weights(S.sd21_cfg_2d(cross_attention_dim=1024), 3)
    d = tmp_path / "stable-diffusion-2-1" / "unet"
    d.mkdir(parents=True)
    (d / "config.json").write_text(json.dumps(cfg_json, indent=2))
    torch.save(dict(sd), str(d / "diffusion_pytorch_model.bin"))
    return str(tmp_path / "stable-diffusion-2-1"), sd


def test_from_pretrained_2d_takes_an_sd21_config(dropin, golden_dir, tmp_path, capsys):
    """an unmodified SD-2.1 config.json with the unet_additional_kwargs of each of the 15 YAMLs that name that checkpoint"""
    from animatediff.models.unet import UNet3DConditionModel
    root, sd2d = _tiny_sd21_dir(tmp_path)
    settings = S.load_json(golden_dir, "sd21_yaml_unet_kwargs.json")
    assert sum(len(s["yamls"]) for s in settings) == 15
    for s in settings:
        kw = s["unet_additional_kwargs"]
        unet = UNet3DConditionModel.from_pretrained_2d(root, subfolder="unet", unet_additional_kwargs=kw)
        cfg = unet.engine_config
        assert cfg.attention_head_dim == S.HEADS and cfg.use_linear_projection and cfg.cross_attention_dim == 1024 and cfg.sample_size == 96
        assert cfg.use_inflated_groupnorm == bool(kw.get("use_inflated_groupnorm")) and cfg.use_temporal_conv == bool(kw.get("use_temporal_conv"))
        assert cfg.use_fps_condition == bool(kw.get("use_fps_condition")) and cfg.motion_module_mid_block and cfg.temporal_position_encoding_max_len == 32
        assert unet.config.upcast_attention is True and unet.config.attention_head_dim == list(S.HEADS)
        assert "unexpected keys: 0" in capsys.readouterr().out
        mine = unet.state_dict()
        assert all(torch.equal(mine[k], v) for k, v in sd2d.items())          # every 2-D tensor arrived, Linear projections included
        assert mine["down_blocks.0.attentions.0.proj_in.weight"].dim() == 2


def test_unet2d_from_pretrained_takes_an_sd21_config(dropin, golden_dir, tmp_path):
    from diffusers import UNet2DConditionModel
    root, sd2d = _tiny_sd21_dir(tmp_path)
    unet = UNet2DConditionModel.from_pretrained(root, subfolder="unet")
    cfg = unet.engine_config
    assert cfg.attention_head_dim == S.HEADS and cfg.use_linear_projection and not cfg.use_motion_module and cfg.cross_attention_dim == 1024
    assert unet.config.upcast_attention is True and unet.config.attention_head_dim == list(S.HEADS) and unet.config.sample_size == 96
    mine = unet.state_dict()
    assert set(mine) == set(sd2d) and all(torch.equal(mine[k], v) for k, v in sd2d.items())
    # the 2-D forward golden: the module's weights through the engine as a one-frame clip
    g = load_golden(golden_dir, "sd2d_unet_sd21_fwd.npz")
    unet = UNet2DConditionModel(**S.TINY_2D, compute_dtype=torch.float32)
    unet.load_state_dict(sd21_weights(S.sd21_cfg_2d(), int(g["weight_seed"])), strict=True)
    want = S.sd21_cfg_2d()
    assert all(getattr(unet.engine_config, k) == getattr(want, k) for k in ("block_out_channels", "attention_head_dim", "use_linear_projection", "cross_attention_dim",
                                                                             "use_motion_module", "use_fps_condition", "conv_in_channels", "use_inflated_groupnorm"))
    eng = UNet3DEngine(pack_unet(unet.state_dict(), unet.engine_config, torch.float32, "cpu"), ops=EmuOps())
    eng.prepare_context(g["text"])
    B, C, H, Wd = g["sample"].shape
    x = torch.zeros(B * H * Wd, 64)
    x[:, :C] = g["sample"].permute(0, 2, 3, 1).reshape(-1, C)
    _, temb = eng.prepare_time_embeddings([int(g["timestep"])], None, None, B)
    out = eng.forward(x, temb, B, 1, H, Wd).reshape(B, H, Wd, 4).permute(0, 3, 1, 2)
    r = rel(out, g["out"])
    print(f"2-D forward on the emulator: rel-L2 {r:.3e} (heads[0] everywhere: {float(g['ctl_heads0']):.3e})")
    assert r < S.TOL_F32 and float(g["ctl_heads0"]) >= 50 * S.TOL_F32


def test_unet2d_needs_the_switch_too(dropin, monkeypatch):
    from diffusers import UNet2DConditionModel
    monkeypatch.delenv("FYC_UNET_VARIANTS")
    with pytest.raises(NotImplementedError, match="FYC_UNET_VARIANTS=1"):
        UNet2DConditionModel(**S.TINY_2D)
    UNet2DConditionModel(**dict(S.TINY_2D, attention_head_dim=8, use_linear_projection=False))       # upcast_attention alone is accepted


# ---- converter ---------------------------------------------------------------------------------------------------------------------------
def test_converter_maps_an_sd2_ldm_state_dict(dropin, golden_dir):
    """the reference converter's key -> shape map for a synthetic v2 LDM state dict: the 2-D proj_in / proj_out weights pass through"""
    from types import SimpleNamespace
    from animatediff.utils.convert_from_ckpt import convert_ldm_unet_checkpoint
    ref = S.load_json(golden_dir, "convert_keymap_sd21.json.gz")
    src = {k: torch.full(tuple(shape), float(i)) for i, (k, shape) in enumerate(ref["src_shapes"].items())}
    src[next(k for k in src if k.startswith("cond_stage_model"))].fill_(-1.0)
    by_tag = {float(v.flatten()[0]): k for k, v in src.items()}
    for config in ({"layers_per_block": 2, "class_embed_type": None, "use_linear_projection": True},
                   SimpleNamespace(layers_per_block=2, class_embed_type=None, use_linear_projection=True)):
        out = convert_ldm_unet_checkpoint(src, config)
        assert sorted([by_tag[float(v.flatten()[0])], k, list(v.shape)] for k, v in out.items()) == ref["unet"]
    lin = [t for t in ref["unet"] if t[1].endswith(("proj_in.weight", "proj_out.weight"))]
    assert len(lin) == 32 and all(t[2] == [2, 2] for t in lin)


# ---- text encoder ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.bfloat16, 3e-2)])      # the bounds of tests/test_encoders_emulated.py
def test_clip_text_gelu_on_emulator(dtype, tol):
    """2 layers, hidden 128, 2 heads of 64, hidden_act "gelu" against transformers.CLIPTextModel"""
    sd, ids, ref = S.clip_gelu_case()
    eng = EN.ClipTextEngine(EN.pack_clip_text(sd, EN.ClipTextConfig(**S.CLIP_GELU), dtype, "cpu"), ops=EmuOps())
    out = eng.encode(ids)
    r = rel(out, ref)
    print(f"CLIP text gelu on the emulator {dtype}: rel-L2 {r:.3e}")
    assert out.shape == ref.shape and r < tol, r
    if dtype == torch.float32:      # the case tells the two activations apart
        quick = EN.ClipTextEngine(EN.pack_clip_text(sd, EN.ClipTextConfig(**dict(S.CLIP_GELU, hidden_act="quick_gelu")), dtype, "cpu"), ops=EmuOps())
        assert rel(quick.encode(ids), ref) > 100 * tol
