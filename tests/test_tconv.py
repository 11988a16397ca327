"""The per-frame GroupNorm / temporal-conv UNet variants (use_inflated_groupnorm, use_temporal_conv) without a GPU: the specification of
FYC_GEMM_CONV_T3 (tests/tconv_spec.py) against nn.Conv3d and the reference's TemporalConvBlock, the engine on the op emulator against goldens
of the real reference (tools/make_golden_tconv.py), the state-dict schema, the drop-in, the shared CFG prefix and the launch schedule."""
import json
import os
import subprocess
import sys

import pytest
import torch

import tconv_spec
from tconv_spec import TINY, TconvEmuOps, engine_forward, load_golden, rel, tconv_cfg, tconv_weights
from followyourclick_amd.engine.schema import unet_schema
from followyourclick_amd.engine.unet3d import UNet3DEngine
from followyourclick_amd.engine.weights import pack_unet
from oracle import refshim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the specification against the reference modules ------------------------------------------------------------------------------
SPEC_VS_REFERENCE = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from oracle import refshim
refshim.install()
import tconv_spec
from followyourclick_amd.engine.weights import pack_conv_t3
from animatediff.models.resnet import TemporalConvBlock
import torch.nn.functional as F

def t3(ops, x, w, b, clips, Fr, HW, C, residual=None):
    out = torch.zeros(clips * Fr * HW, C)
    ops.gemm(x, pack_conv_t3(w, torch.float32, "cpu"), out, M=clips * Fr * HW, N=C, K=3 * C, lda=C, ldw=3 * C, ldo=C, bias=b, residual=residual, ldr=C,
             mode=3, conv=dict(Cin=C, frames=Fr, rows=HW))
    return out

def gn_silu(x, g, b, clips, Fr, HW, C):       # nn.GroupNorm(32, C) on the 5-D tensor: statistics over (C / 32, F, H, W) per clip
    v = x.reshape(clips, Fr * HW, 32, C // 32).double()
    m = v.mean(dim=(1, 3), keepdim=True)
    var = (v * v).mean(dim=(1, 3), keepdim=True) - m * m
    y = ((v - m) * torch.rsqrt(var + 1e-5)).reshape(clips * Fr * HW, C).float() * g + b
    return F.silu(y)

ops = tconv_spec.TconvEmuOps()
for clips, Fr, HW, C in ((2, 1, 4, 64), (2, 2, 16, 64), (1, 5, 15, 128), (2, 16, 16, 320)):
    torch.manual_seed(C + Fr)
    H, Wd = (HW, 1) if HW % 4 else (HW // 4, 4)
    x5 = torch.randn(clips, C, Fr, H, Wd)
    rows = x5.permute(0, 2, 3, 4, 1).reshape(-1, C).contiguous()
    conv = torch.nn.Conv3d(C, C, (3, 1, 1), padding=(1, 0, 0))
    with torch.no_grad():
        ref = conv(x5).permute(0, 2, 3, 4, 1).reshape(-1, C)
        got = t3(ops, rows, conv.weight, conv.bias, clips, Fr, HW, C)
        print("MAXABS conv", clips, Fr, HW, C, float((got - ref).abs().max()), float(ref.abs().max()))
        blk = TemporalConvBlock(C, C, dropout=0.1, spatial_aware=False).eval()
        for seq in (blk.conv1, blk.conv2, blk.conv3, blk.conv4):        # (conv4 is zero-initialised by the constructor: make the block visible)
            torch.nn.init.normal_(seq[0].weight, 1.0, 0.1)
            torch.nn.init.normal_(seq[0].bias, 0.0, 0.05)
            torch.nn.init.normal_(seq[-1].weight, 0.0, (3 * C) ** -0.5)
            torch.nn.init.normal_(seq[-1].bias, 0.0, 0.05)
        refb = blk(x5).permute(0, 2, 3, 4, 1).reshape(-1, C)
        h = rows
        for i, seq in enumerate((blk.conv1, blk.conv2, blk.conv3, blk.conv4)):
            n = gn_silu(h, seq[0].weight, seq[0].bias, clips, Fr, HW, C)
            h = t3(ops, n, seq[-1].weight, seq[-1].bias, clips, Fr, HW, C, residual=rows if i == 3 else None)
        print("MAXABS block", clips, Fr, HW, C, float((h - refb).abs().max()), float(refb.abs().max()))
"""

SPEC_SHAPES = [(2, 1, 4, 64), (2, 2, 16, 64), (1, 5, 15, 128), (2, 16, 16, 320)]


@pytest.mark.skipif(not refshim.available(), reason="the reference tree is not present")
def test_spec_matches_reference_conv3d_and_temporal_conv_block():
    """f32, (clips, F, H*W, C) = (2,1,4,64), (2,2,16,64), (1,5,15,128), (2,16,16,320): the T3 specification fed the packed weight against
    nn.Conv3d((3,1,1), padding=(1,0,0)), and the reference's TemporalConvBlock against a composition of the specification: max abs <= 1e-5.
    In a subprocess: the reference's `animatediff` package and the drop-in's cannot share an interpreter."""
    r = subprocess.run([sys.executable, "-c", SPEC_VS_REFERENCE, os.path.join(ROOT, "tests")], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith("MAXABS")]
    assert len(lines) == 2 * len(SPEC_SHAPES), r.stdout
    assert sorted({tuple(map(int, l[2:6])) for l in lines}) == sorted(SPEC_SHAPES)
    for _, what, clips, F, HW, C, err, mag in lines:
        print(f"spec vs reference {what} clips={clips} F={F} HW={HW} C={C}: max abs {float(err):.3e} (|ref| max {float(mag):.3f})")
        assert float(err) <= 1e-5, (what, clips, F, HW, C, err)


# ---- the engine on the emulator against the real reference -------------------------------------------------------------------------
def _engine(g, cfg=None, ops=None, dtype=torch.float32):
    sd = tconv_weights(int(g["weight_seed"]), int(g["extra_seed"]))
    return UNet3DEngine(pack_unet(sd, cfg or tconv_cfg(), dtype, "cpu"), ops=ops or TconvEmuOps())


@pytest.mark.parametrize("F", [5, 16])
def test_engine_on_emulator_matches_reference_golden(golden_dir, F):
    g = load_golden(golden_dir, F)
    assert int(g["F"]) == F and g["sample"].shape[2] == F
    r = rel(engine_forward(_engine(g), g), g["out"])
    print(f"tconv engine on the emulator, F={F}: rel-L2 {r:.3e}")
    assert r < 1e-3, r
    # controls: the fixture sees the temporal blocks and the per-frame norms (the reference's own distances are stored with it)
    ra = rel(engine_forward(_engine(g, tconv_cfg(use_temporal_conv=False)), g), g["out"])
    rb = rel(engine_forward(_engine(g, tconv_cfg(use_inflated_groupnorm=False)), g), g["out"])
    print(f"  temporal blocks skipped: rel-L2 {ra:.3e} (reference {float(g['ctl_no_tconv']):.3e}); cross-frame ResNet norms: {rb:.3e} "
          f"(reference {float(g['ctl_cross_frame']):.3e})")
    assert float(g["ctl_no_tconv"]) > 0.1 and float(g["ctl_cross_frame"]) > 0.05
    assert ra > 0.5 * float(g["ctl_no_tconv"]), ra
    assert rb > 0.5 * float(g["ctl_cross_frame"]), rb


def test_temporal_norm_keeps_32_groups_and_default_eps(golden_dir):
    """the temporal block's GroupNorm has 32 groups and eps 1e-5 whatever norm_num_groups / norm_eps of the UNet say, and is cross-frame"""
    seen = []

    class Spy(TconvEmuOps):
        def gn_apply_cs(self, x1, cs1, gamma, beta, y, **kw):
            seen.append((kw["groups"], kw["eps"], kw["rows_per_sample"]))
            return super().gn_apply_cs(x1, cs1, gamma, beta, y, **kw)

        def gn_apply(self, x, stats, g_, b_, y, **kw):
            seen.append((kw["groups"], kw["eps"], kw["rows_per_sample"]))
            return super().gn_apply(x, stats, g_, b_, y, **kw)
    g = load_golden(golden_dir, 5)
    eng = _engine(g, tconv_cfg(norm_num_groups=16, norm_eps=1e-6), ops=Spy())
    engine_forward(eng, g)
    t = [s for s in seen if s[0] == 32]
    assert len(t) == 4 * 22 and all(e == 1e-5 and rps % 5 == 0 for _, e, rps in t), t[:4]
    # every other GroupNorm of a ResNet / conv_norm_out is per frame with the model's group count; transformers use eps 1e-6 of their own
    assert all(gr == 16 for gr, _, _ in seen if gr != 32)


# ---- schema and drop-in ------------------------------------------------------------------------------------------------------------
def test_schema_matches_reference(golden_dir):
    with open(os.path.join(golden_dir, "schema_unet_tiny_tconv.json")) as f:
        ref = json.load(f)
    mine = unet_schema(tconv_cfg())
    assert {k: list(v) for k, v in mine.items()} == ref
    assert sum(".temporal_conv." in k for k in mine) == 352
    assert not any(".temporal_conv." in k for k in unet_schema(tconv_cfg(use_temporal_conv=False)))


@pytest.fixture()
def dropin(monkeypatch):
    import followyourclick_amd
    monkeypatch.setenv("FYC_UNET_VARIANTS", "1")          # the drop-in builds these model families on request only
    followyourclick_amd.install_dropin(force=True)
    yield
    for name in [k for k in sys.modules if k.split(".")[0] in ("animatediff", "diffusers", "ip_adapter")]:
        del sys.modules[name]


def test_dropin_accepts_both_options(dropin, golden_dir):
    from animatediff.models.unet import UNet3DConditionModel
    unet = UNet3DConditionModel(**TINY, use_inflated_groupnorm=True, use_temporal_conv=True, compute_dtype=torch.float32)
    cfg = unet.engine_config
    assert cfg.use_inflated_groupnorm and cfg.use_temporal_conv
    off = UNet3DConditionModel(**TINY, compute_dtype=torch.float32).engine_config
    assert not off.use_inflated_groupnorm and not off.use_temporal_conv
    with open(os.path.join(golden_dir, "schema_unet_tiny_tconv.json")) as f:
        ref = json.load(f)
    sd = unet.state_dict()
    assert {k: list(v.shape) for k, v in sd.items()} == ref
    # conv4 is zero after construction, the other three are not
    for k, v in sd.items():
        if ".temporal_conv.conv4.3." in k:
            assert not v.any(), k
        elif ".temporal_conv." in k and k.endswith(".weight"):
            assert v.any(), k
    # a reference-layout state dict round-trips with no missing and no unexpected keys
    full = tconv_weights(0, 11)
    res = unet.load_state_dict({k: full[k] for k in ref}, strict=False)
    assert not res.missing_keys and not res.unexpected_keys
    back = unet.state_dict()
    assert set(back) == set(ref) and all(torch.equal(back[k], full[k]) for k in ref)


def test_dropin_zero_conv4_is_the_identity(dropin, golden_dir):
    """a model with zero conv4 and the option on equals the same model with the option off, bit for bit"""
    from animatediff.models.unet import UNet3DConditionModel
    g = load_golden(golden_dir, 5)
    off = UNet3DConditionModel(**TINY, use_inflated_groupnorm=True, compute_dtype=torch.float32)
    on = UNet3DConditionModel(**TINY, use_inflated_groupnorm=True, use_temporal_conv=True, compute_dtype=torch.float32)
    res = on.load_state_dict(off.state_dict(), strict=False)          # the other weights of `off`; the temporal blocks keep their initial values
    assert not res.unexpected_keys and len(res.missing_keys) == 352
    outs = []
    for m in (off, on):
        eng = UNet3DEngine(pack_unet(m.state_dict(), m.engine_config, torch.float32, "cpu"), ops=TconvEmuOps())
        outs.append(engine_forward(eng, g))
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


def test_dropin_still_refuses_pseudo_conv3d(dropin):
    from animatediff.models.unet import UNet3DConditionModel
    with pytest.raises(NotImplementedError, match="use_pseudo_conv3d"):
        UNet3DConditionModel(**TINY, use_pseudo_conv3d=True)


def test_dropin_builds_the_variants_on_request_only(dropin, monkeypatch):
    """without FYC_UNET_VARIANTS=1 both options stay refused, with a message that names the switch"""
    from animatediff.models.unet import UNet3DConditionModel
    monkeypatch.delenv("FYC_UNET_VARIANTS")
    for opts in (dict(use_inflated_groupnorm=True), dict(use_temporal_conv=True), dict(use_inflated_groupnorm=True, use_temporal_conv=True)):
        with pytest.raises(NotImplementedError, match="FYC_UNET_VARIANTS=1"):
            UNet3DConditionModel(**TINY, **opts)


# ---- shared CFG prefix ---------------------------------------------------------------------------------------------------------------
class SharingEmu(TconvEmuOps):
    """the emulator plus a specification of fyc_repeat and q_batch_mod (as tests/test_shared_prefix_emulated.py): the shared schedule on the CPU"""

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
    """the temporal conv never crosses clips: the CFG pair with the prefix run once agrees with the duplicated batch (f32: 2e-4, the bound of
    tests/test_shared_prefix_emulated.py)"""
    g = load_golden(golden_dir, 5)
    eng = _engine(g, ops=SharingEmu())
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


# ---- schedule ------------------------------------------------------------------------------------------------------------------------
def _trace(cfg, sd, B=2, F=4, H=32, Wd=32, share=1):
    import trace_ops
    ops = trace_ops.TraceOps(fused=True)
    eng = UNet3DEngine(pack_unet(sd, cfg, torch.bfloat16, "cpu"), ops=ops)
    eng.prepare_context(torch.zeros(B, 77, 64))
    _, temb = eng.prepare_time_embeddings([500], [2] * B, [4] * B, B)
    ops.reset()
    eng.forward(torch.zeros(B // share * F * H * Wd, 64, dtype=torch.bfloat16), temb, B, F, H, Wd, shared_prefix=share)
    return ops.log


def test_schedule_records_four_t3_gemms_per_resnet():
    import trace_ops
    default = trace_ops.run_unet(trace_ops.unet_cases()[0]).log
    assert not any(l.op == "gemm" and l.args.get("mode", 0) == 3 for l in default)
    for share in (1, 2):
        log = _trace(tconv_cfg(norm_num_groups=16), tconv_weights(0, 11), share=share)      # (16: the temporal norms are the ones with 32 groups)
        t3 = [l for l in log if l.op == "gemm" and l.args.get("mode", 0) == 3]
        assert len(t3) == 4 * 22, len(t3)
        for i, l in enumerate(t3):
            a = l.args
            assert a["K"] == 3 * a["N"] == 3 * a["conv"]["Cin"] and a["conv"]["frames"] == 4 and a["M"] % (4 * a["conv"]["rows"]) == 0
            assert (a["residual"] is not None) == (i % 4 == 3), i
            assert a["bias"] is not None
        # the fourth convolution's residual is the ResNet's output: the buffer the first temporal norm of the block read
        norms = [l for l in log if l.op in ("gn_apply_cs", "gn_apply") and l.args["groups"] == 32]
        assert len(norms) == 4 * 22
        for b in range(22):
            x_in = norms[4 * b].args["x1" if norms[4 * b].op == "gn_apply_cs" else "x"]
            assert t3[4 * b + 3].args["residual"].storage == x_in.storage
