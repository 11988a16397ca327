"""FYC_GEMM_CONV_T3 (the 3-tap convolution along the frame axis) and the per-frame GroupNorm / temporal-conv UNet variants on the GPU, all
through the C ABI: parity against the f64 specification of tests/tconv_spec.py with guard rows of NaN around the input and behind the output,
refusals, split-K, output statistics, repeatability, and engine / drop-in forwards against goldens of the real reference
(tools/make_golden_tconv.py)."""
import functools
import math
import sys

import pytest
import torch

from tconv_spec import TINY, TconvEmuOps, engine_forward, load_golden, rel, tconv_cfg, tconv_weights
from test_kernels_gpu import CONV_TILES, DT, RTOL, close, rnd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from followyourclick_amd import ops
    h = ops.get()
    h.ensure_init(torch.device("cuda:0"))
    assert h.name == "hip"
    return h


SPEC = TconvEmuOps(acc=torch.float64)
# (clips, F, H, W, Cin, Cout): both neighbours absent; two frames; HW = 15 - tiles straddle frames and clips; one row per frame; the 8x8 level of
# the C = 320 width; K = 1920 with 4-row frames
SHAPES = [(1, 1, 4, 4, 64, 64), (2, 2, 4, 4, 64, 64), (2, 3, 3, 5, 64, 128), (3, 5, 1, 1, 128, 64), (1, 16, 8, 8, 320, 320), (2, 16, 2, 2, 640, 320)]
GUARD_OUT = 37          # rows behind the output that must stay NaN


def _kw(shape):
    clips, F, H, W, Cin, Cout = shape
    M = clips * F * H * W
    return dict(M=M, N=Cout, K=3 * Cin, lda=Cin, ldw=3 * Cin, ldo=Cout, ldr=Cout, mode=3, conv=dict(Cin=Cin, frames=F, rows=H * W))


@functools.lru_cache(maxsize=None)
def _problem(shape, dt):
    """operands and the f64 specification's result, computed once per (shape, dtype) and shared by the tile cases"""
    clips, F, H, W, Cin, Cout = shape
    T, kw = DT[dt], _kw(shape)
    x, w = rnd((kw["M"], Cin), T, 1), rnd((Cout, 3 * Cin), T, 2, 1 / math.sqrt(3 * Cin))
    bias, res = rnd((Cout,), torch.float32, 3), rnd((kw["M"], Cout), T, 4)
    ref = torch.zeros(kw["M"], Cout, dtype=T)
    SPEC.gemm(x, w, ref, bias=bias, residual=res, out_scale=1.25, **kw)
    return x, w, bias, res, ref


def _guarded_input(x, rows_per_frame):
    """the input between two guard blocks of HW + 1 NaN rows: a tap that should be absent, or a read across the tensor's end, turns the output non-finite"""
    M, Cin = x.shape
    gr = rows_per_frame + 1
    buf = torch.full((gr + M + gr, Cin), float("nan"), dtype=x.dtype, device="cuda")
    buf[gr:gr + M] = x.cuda()
    return buf, buf[gr:gr + M]


def _guarded_output(M, N, T):
    buf = torch.full((M + GUARD_OUT, N), float("nan"), dtype=T, device="cuda")
    return buf, buf[:M]


@pytest.mark.parametrize("dt,tile_ring", [("bf16", t) for t in CONV_TILES] + [("f16", (0, 0)), ("f32", (0, 0))])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_t3_matches_the_specification(hip, shape, dt, tile_ring):
    """one global relative L2 per case; per element and on every tile of the 16-bit types: the group t3 of tests/gemm_cases.py (tests/test_gemm_epilogues_gpu.py)"""
    clips, F, H, W, Cin, Cout = shape
    T, kw = DT[dt], _kw(shape)
    x, w, bias, res, ref = _problem(shape, dt)
    keep, a = _guarded_input(x, H * W)
    obuf, o_h = _guarded_output(kw["M"], Cout, T)
    hip.set_tuning(1, tile_ring[0])
    hip.set_tuning(2, tile_ring[1])
    try:
        hip.gemm(a, w.cuda(), o_h, bias=bias.cuda(), residual=res.cuda(), out_scale=1.25, **kw)
        torch.cuda.synchronize()
    finally:
        hip.set_tuning(1, 0)
        hip.set_tuning(2, 0)
    close(o_h, ref, f"conv_t3 {dt} tile {tile_ring} {shape}", RTOL[dt])
    assert torch.isnan(obuf[kw["M"]:].float()).all(), "rows behind the output were written"
    assert torch.isnan(keep[: H * W + 1].float()).all() and torch.isnan(keep[-(H * W + 1):].float()).all()


def test_t3_refusals(hip):
    """Cin = 96 and K != 3 * Cin return < 0 with a message and launch nothing"""
    T = torch.bfloat16
    for Cin, K, what in ((96, 288, "multiple of 64"), (64, 128, "3\\*Cin"), (64, 576, "3\\*Cin")):
        M, N = 2 * 2 * 16, 64
        a = torch.zeros(M, Cin, dtype=T, device="cuda")
        w = torch.zeros(N, K, dtype=T, device="cuda")
        o = torch.full((M, N), float("nan"), dtype=T, device="cuda")
        with pytest.raises(Exception, match=what):
            hip.gemm(a, w, o, M=M, N=N, K=K, lda=Cin, ldw=K, ldo=N, mode=3, conv=dict(Cin=Cin, frames=2, rows=16))
        torch.cuda.synchronize()
        assert torch.isnan(o.float()).all()
    a, w = torch.zeros(64, 64, dtype=T, device="cuda"), torch.zeros(64, 192, dtype=T, device="cuda")
    o = torch.full((64, 64), float("nan"), dtype=T, device="cuda")
    with pytest.raises(Exception, match="whole number of clips"):        # M = 64 rows are not whole clips of 3 x 16 rows
        hip.gemm(a, w, o, M=64, N=64, K=192, lda=64, ldw=192, ldo=64, mode=3, conv=dict(Cin=64, frames=3, rows=16))
    torch.cuda.synchronize()
    assert torch.isnan(o.float()).all()


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_t3_split_k(hip, dt):
    """tuning key 10 = 2 makes M = 256, N = 128, Cin = 128 split its K = 384 (6 K tiles: two (slab, tap) triples) over the work items"""
    T = DT[dt]
    shape = (2, 4, 4, 8, 128, 128)
    kw = _kw(shape)
    assert (kw["M"], kw["N"], kw["K"]) == (256, 128, 384)
    x, w, bias, res, ref = _problem(shape, dt)
    keep, a = _guarded_input(x, 32)
    obuf, o_h = _guarded_output(256, 128, T)
    hip.set_tuning(10, 2)
    try:
        assert hip.gemm_split_bytes(T, M=256, N=128, K=384, mode=3) > 0, "this problem is expected to take the split-K path"
        hip.gemm(a, w.cuda(), o_h, bias=bias.cuda(), residual=res.cuda(), out_scale=1.25, **kw)
        torch.cuda.synchronize()
    finally:
        hip.set_tuning(10, 0)
    close(o_h, ref, f"conv_t3 split-K {dt}", RTOL[dt])
    assert torch.isnan(obuf[256:].float()).all()


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape", [(2, 4, 8, 8, 64, 320), (2, 3, 4, 12, 128, 128), (1, 16, 8, 8, 320, 320)], ids=lambda s: "x".join(map(str, s)))
def test_t3_output_statistics(hip, shape, dt):
    """chan_parts from a T3 epilogue folded at out_rows = F * HW (the next temporal norm) and at HW (a per-frame consumer) == f64 sums of the
    stored output; HW = 64 and 48: a row tile touches 2 .. 4 frames"""
    clips, F, H, W, Cin, Cout = shape
    T, kw = DT[dt], _kw(shape)
    M, hw = kw["M"], H * W
    x, w, bias, res, ref = _problem(shape, dt)
    keep, a = _guarded_input(x, hw)
    nt, tile_rows, slots = hip.gemm_stat_layout(T, M=M, N=Cout, K=kw["K"], cs_rows=hw, mode=3)
    assert 2 <= slots <= 4 and tile_rows > hw, (tile_rows, slots)
    parts = torch.full((nt * slots * Cout * 2,), float("nan"), dtype=torch.float32, device="cuda")
    o_h = torch.full((M, Cout), float("nan"), dtype=T, device="cuda")
    hip.gemm(a, w.cuda(), o_h, bias=bias.cuda(), residual=res.cuda(), out_scale=1.25, chan_parts=parts, cs_rows=hw, **kw)
    torch.cuda.synchronize()
    close(o_h, ref, f"conv_t3 + stats {dt} {shape}", RTOL[dt])
    v = o_h.cpu().double()
    for out_rows in (F * hw, hw):
        cs = torch.full((M // out_rows, Cout, 2), float("nan"), dtype=torch.float64, device="cuda")
        hip.chan_stats_reduce(parts, cs, rows=M, N=Cout, cs_rows=hw, tile_rows=tile_rows, slots=slots, out_rows=out_rows)
        torch.cuda.synchronize()
        vs = v.reshape(M // out_rows, out_rows, Cout)
        close(cs, torch.stack([vs.sum(dim=1), (vs * vs).sum(dim=1)], dim=-1), f"conv_t3 chan stats {dt} out_rows {out_rows} ({tile_rows}-row tiles, {slots} slots)", 2e-6)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_t3_is_repeatable(hip, dt):
    shape = (2, 5, 4, 4, 128, 320)
    clips, F, H, W, Cin, Cout = shape
    T, kw = DT[dt], _kw(shape)
    x, w, bias, res, _ = _problem(shape, dt)
    cs_rows = F * H * W          # 80-row samples: a 128-row tile touches up to 3
    nt, tile_rows, slots = hip.gemm_stat_layout(T, M=kw["M"], N=Cout, K=kw["K"], cs_rows=cs_rows, mode=3)
    assert 1 <= slots <= 4
    runs = []
    xa, wa, ba, ra = x.cuda(), w.cuda(), bias.cuda(), res.cuda()
    for _ in range(2):
        parts = torch.full((nt * slots * Cout * 2,), float("nan"), dtype=torch.float32, device="cuda")
        o = torch.full((kw["M"], Cout), float("nan"), dtype=T, device="cuda")
        hip.gemm(xa, wa, o, bias=ba, residual=ra, chan_parts=parts, cs_rows=cs_rows, **kw)
        torch.cuda.synchronize()
        runs.append((o.cpu(), parts.cpu()))
    assert torch.isfinite(runs[0][0].float()).all()
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(torch.nan_to_num(runs[0][1], nan=-1.0), torch.nan_to_num(runs[1][1], nan=-1.0))


# ---- engine and drop-in against the real reference -----------------------------------------------------------------------------------
TOL = {torch.float32: 1e-3, torch.bfloat16: 5e-2, torch.float16: 5e-2}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("F", [5, 16])
def test_engine_forward_vs_reference_golden(golden_dir, F, dtype):
    from followyourclick_amd.engine.unet3d import UNet3DEngine
    from followyourclick_amd.engine.weights import pack_unet
    g = load_golden(golden_dir, F)
    eng = UNet3DEngine(pack_unet(tconv_weights(int(g["weight_seed"]), int(g["extra_seed"])), tconv_cfg(), dtype, "cuda:0"))
    assert eng.ops.name == "hip"
    out = engine_forward(eng, g, dtype, "cuda:0")
    assert torch.isfinite(out).all()
    r = rel(out, g["out"])
    print(f"tconv engine forward F={F} {dtype}: rel-L2 {r:.3e} (bound {TOL[dtype]:.0e})")
    assert r < TOL[dtype], r


@pytest.fixture(scope="module")
def dropin():
    import os
    import followyourclick_amd
    old = os.environ.get("FYC_UNET_VARIANTS")
    os.environ["FYC_UNET_VARIANTS"] = "1"                 # the drop-in builds these model families on request only
    followyourclick_amd.install_dropin(force=True)
    yield
    if old is None:
        del os.environ["FYC_UNET_VARIANTS"]
    else:
        os.environ["FYC_UNET_VARIANTS"] = old
    for name in [k for k in sys.modules if k.split(".")[0] in ("animatediff", "diffusers", "ip_adapter")]:
        del sys.modules[name]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("F", [5, 16])
def test_dropin_forward_vs_reference_golden(dropin, golden_dir, F, dtype):
    from animatediff.models.unet import UNet3DConditionModel
    g = load_golden(golden_dir, F)
    unet = UNet3DConditionModel(**TINY, use_inflated_groupnorm=True, use_temporal_conv=True, compute_dtype=dtype).to("cuda")
    res = unet.load_state_dict(tconv_weights(int(g["weight_seed"]), int(g["extra_seed"])), strict=False)
    assert not res.missing_keys and not res.unexpected_keys
    out = unet(g["sample"].cuda(), torch.tensor(int(g["timestep"])), g["text"].cuda(), use_fps_condition=True,
               fps_tensor=g["fps"].cuda(), flow_control=g["flow"].cuda()).sample.float().cpu()
    assert torch.isfinite(out).all()
    r = rel(out, g["out"])
    print(f"tconv drop-in forward F={F} {dtype}: rel-L2 {r:.3e} (bound {TOL[dtype]:.0e})")
    assert r < TOL[dtype], r
