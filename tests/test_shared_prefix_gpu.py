"""The CFG-shared UNet prefix: fyc_repeat, fyc_attention with q_batch_mod, and UNet3DEngine.forward(shared_prefix=2) against the
reference golden of the duplicated batch (never against the unshared engine alone)."""
import os

import numpy as np
import pytest
import torch

from followyourclick_amd.engine import UNet3DConfig
from followyourclick_amd.engine.unet3d import UNet3DEngine
from followyourclick_amd.engine.weights import pack_unet
from oracle import functional as Fn
from oracle import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    from followyourclick_amd import ops
    h = ops.get()
    h.ensure_init(torch.device(DEV))
    return h


def rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


@pytest.mark.parametrize("times", [1, 2, 3])
@pytest.mark.parametrize("nbytes", [16, 48, 16 * 1001, 16 * 65537])       # odd multiples of 16; the last one is more than one grid-stride pass of a block
def test_repeat_bytes(hip, nbytes, times):
    src = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, generator=torch.Generator().manual_seed(nbytes)).to(DEV)
    dst = torch.full((times * nbytes + 16,), 0xAB, dtype=torch.uint8, device=DEV)
    hip.repeat(src, dst[: times * nbytes], times=times)
    torch.cuda.synchronize()
    assert torch.equal(dst[: times * nbytes].cpu(), src.cpu().repeat(times))
    assert (dst[times * nbytes:] == 0xAB).all()                               # nothing written behind the last copy


def test_repeat_f64_and_argument_checks(hip):
    src = rnd((3, 10, 2), torch.float64, 1).to(DEV)                           # channel sums: [samples][C][2] doubles
    dst = torch.empty(6, 10, 2, dtype=torch.float64, device=DEV)
    hip.repeat(src, dst, times=2)
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), src.cpu().repeat(2, 1, 1))
    with pytest.raises(Exception, match="multiple of 16"):
        hip.repeat(src.reshape(-1)[:3], dst.reshape(-1)[:6], times=2)         # 24 bytes
    with pytest.raises(Exception, match="overlap"):
        hip.repeat(dst[:3], dst, times=2)
    with pytest.raises(ValueError):
        hip.repeat(src, dst, times=3)


@pytest.mark.parametrize("nq,d", [(64, 40), (100, 80)])                       # 100 queries: a ragged query block
def test_attention_q_batch_mod_equals_materialised_repeat(hip, nq, d):
    T = torch.bfloat16
    B, H, nk, mod = 4, 8, 77, 2
    ldvt = ((nk + 7) // 8) * 8
    q, k = rnd((mod * H, nq, d), T, 1).to(DEV), rnd((B * H, nk, d), T, 2).to(DEV)
    vt = torch.zeros(B * H, d, ldvt, dtype=T, device=DEV)
    vt[..., :nk] = rnd((B * H, d, nk), T, 3).to(DEV)
    kw = dict(batch=B, heads=H, n_q=nq, n_k=nk, d=d, ldo=H * d, ldvt=ldvt, scale=d ** -0.5, kv_batch_div=1)
    o_mod = torch.full((B * nq, H * d), float("nan"), dtype=T, device=DEV)
    hip.attention(q, k, vt, o_mod, q_batch_mod=mod, **kw)
    o_rep = torch.full((B * nq, H * d), float("nan"), dtype=T, device=DEV)
    hip.attention(q.reshape(mod, H, nq, d).repeat(B // mod, 1, 1, 1).reshape(B * H, nq, d).contiguous(), k, vt, o_rep, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(o_mod.float()).all()
    assert torch.equal(o_mod, o_rep)
    assert not torch.equal(o_mod[: nq], o_mod[2 * nq: 3 * nq])               # the halves saw different K / V
    with pytest.raises(Exception, match="q_batch_mod"):
        hip.attention(q, k, vt, o_mod, q_batch_mod=B + 1, **kw)


# ---- engine level --------------------------------------------------------------------------------------------------------
def tiny_cfg(**kw):
    return UNet3DConfig(block_out_channels=(64, 128, 256, 256), cross_attention_dim=64, sample_size=8, **kw)


def _nhwc(x9, dtype):
    B, C9, F, H, Wd = x9.shape
    x = torch.zeros(B * F * H * Wd, 64)
    x[:, :C9] = x9.permute(0, 2, 3, 4, 1).reshape(-1, C9)
    return x.to(dtype).to(DEV)


def rel(a, b):
    return ((a.float().cpu() - b.float().cpu()).norm() / b.float().cpu().norm()).item()


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = {k: torch.from_numpy(v) if v.shape else v for k, v in np.load(os.path.join(golden_dir, "unet_tiny_fwd.npz")).items()}
    # the golden batch is a CFG pair: identical inputs and conditioning rows, different text states
    assert g["sample"].shape[0] == 2 and torch.equal(g["sample"][0], g["sample"][1])
    assert g["fps"][0] == g["fps"][1] and g["flow"][0] == g["flow"][1] and not torch.equal(g["text"][0], g["text"][1])
    return g


def _engine(g, dtype):
    sd = W.make_weights(W.unet_state_shapes(Fn.tiny_unet_config()), int(g["weight_seed"]))
    eng = UNet3DEngine(pack_unet(sd, tiny_cfg(), dtype, DEV))
    eng.prepare_context(g["text"])
    _, temb = eng.prepare_time_embeddings([int(g["timestep"])], g["fps"].tolist(), g["flow"].tolist(), 2)
    return eng, temb


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-3), (torch.bfloat16, 5e-2)])
def test_shared_prefix_forward_vs_reference_golden(golden, dtype, tol):
    g = golden
    eng, temb = _engine(g, dtype)
    B, _, F, H, Wd = g["sample"].shape
    assert eng.shares_prefix(B)
    out = eng.forward(_nhwc(g["sample"][:1], dtype), temb, B, F, H, Wd, shared_prefix=2)
    torch.cuda.synchronize()
    assert eng.last_schedule == "shared"
    out = out.float().cpu().reshape(B, F, H, Wd, 4).permute(0, 4, 1, 2, 3)
    assert torch.isfinite(out).all()
    r = rel(out, g["out"])
    print(f"unet fwd shared prefix {dtype}: rel-L2 {r:.3e} vs the reference golden (bound {tol:.0e})")
    assert r < tol, r
    assert not torch.equal(out[0], out[1])                                    # the halves did see their own text states
    if dtype == torch.float32:
        plain = eng.forward(_nhwc(g["sample"], dtype), temb, B, F, H, Wd)
        torch.cuda.synchronize()
        assert eng.last_schedule == "plain"
        r2 = rel(out, plain.float().cpu().reshape(B, F, H, Wd, 4).permute(0, 4, 1, 2, 3))
        print(f"unet fwd shared vs unshared engine f32: rel-L2 {r2:.3e}")
        assert r2 < tol, r2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_shared_prefix_with_temb_first_runs_the_plain_schedule(golden, dtype):
    """a frame-0 time-embedding row (use_first_frame_condition) is outside the shared schedule: forward duplicates the input and runs
    exactly what it runs for the duplicated batch"""
    g = golden
    eng, temb = _engine(g, dtype)
    _, temb0 = eng.prepare_time_embeddings([0], None, None, 1)
    B, _, F, H, Wd = g["sample"].shape
    assert not eng.shares_prefix(B, temb0)
    a = eng.forward(_nhwc(g["sample"][:1], dtype), temb, B, F, H, Wd, temb_first=temb0, shared_prefix=2)
    assert eng.last_schedule == "plain"
    b = eng.forward(_nhwc(g["sample"], dtype), temb, B, F, H, Wd, temb_first=temb0)
    torch.cuda.synchronize()
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    with pytest.raises(ValueError, match="even batch"):
        eng.forward(_nhwc(g["sample"][:1], dtype), temb[:1], 1, F, H, Wd, shared_prefix=2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_shared_prefix_reads_no_unwritten_memory(golden, dtype):
    """the shared schedule (broadcast buffers, half-batch statistics partials folded by their consumers) gives the same bits whether
    every engine buffer starts as 0x00 or as 0xFF bytes (the check of tests/test_uninit_gpu.py, on forward(shared_prefix=2))"""
    from followyourclick_amd import ops as ops_mod
    from followyourclick_amd.engine import base
    g = golden
    eng, temb = _engine(g, dtype)
    B, _, F, H, Wd = g["sample"].shape
    x = _nhwc(g["sample"][:1], dtype)
    outs = []
    old = base.ALLOC_FILL
    try:
        for fill in (0x00, 0xFF):
            base.ALLOC_FILL = fill
            ws = ops_mod.get()._ws
            if ws is not None:
                ws.fill_(fill)
            outs.append(eng.forward(x, temb, B, F, H, Wd, shared_prefix=2)[:, :4].contiguous())
            torch.cuda.synchronize()
            assert eng.last_schedule == "shared"
    finally:
        base.ALLOC_FILL = old
    assert torch.isfinite(outs[1].float()).all()
    assert torch.equal(outs[0], outs[1])
