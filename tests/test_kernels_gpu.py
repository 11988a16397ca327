"""Per-op parity of the HIP kernels (through the C ABI) against the torch-CPU op specification
(tests/emu_ops.py).  Tolerances: f32 mode rel-L2 <= 2e-5; bf16 mode rel-L2 <= 4e-3 (inputs are the
same bf16 values on both sides, so the only differences are accumulation order and the final
round-to-bf16)."""
import math

import pytest
import torch

from emu_ops import EmuOps

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f32": torch.float32, "f16": torch.float16}
RTOL = {"bf16": 4e-3, "f32": 2e-5, "f16": 5e-4}      # f16 (FYC_F16): same operand values on both sides, one rounding to 11 bits at the end
F16_TILES = [(0, 0), (1, 2), (2, 2), (3, 2), (5, 2), (6, 2)]      # the f16 instantiations share the tile templates: a subset keeps the suite short


@pytest.fixture(scope="module")
def hip():
    from followyourclick_amd import ops
    h = ops.get()
    h.ensure_init(torch.device("cuda:0"))
    return h


@pytest.fixture(scope="module")
def emu():
    return EmuOps(acc=torch.float64)


def rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def close(hip_t, emu_t, tag, rtol):
    a, b = hip_t.detach().cpu().double().reshape(-1), emu_t.detach().double().reshape(-1)
    assert a.shape == b.shape, (tag, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{tag}: non-finite values in HIP output ({(~torch.isfinite(a)).sum().item()} of {a.numel()})"
    err = (a - b).norm() / (b.norm() + 1e-30)
    mx = (a - b).abs().max().item()
    bad = ((a - b).abs() > 10 * rtol * (b.abs().max() + 1e-30)).nonzero().reshape(-1)
    assert err.item() <= rtol, (f"{tag}: rel-L2 {err.item():.3e} > {rtol:.1e}; max abs {mx:.3e} (ref max {b.abs().max().item():.3e}); "
                                f"{bad.numel()}/{a.numel()} elements off, first at {bad[:8].tolist()}")


# ---------------------------------------------------------------------------------------------
PLAIN_TILES = [(0, 0), (1, 2), (1, 3), (2, 2), (3, 2), (4, 2), (5, 2), (6, 2), (7, 2), (8, 2), (10, 2), (11, 2)]
CONV_TILES = [(0, 0), (1, 3), (3, 2), (4, 2), (5, 2), (6, 2), (7, 2), (8, 2), (10, 2), (11, 2)]


def _dt_tiles(tiles):
    """f32 parity mode has a fixed tile choice: only the automatic one is parametrised for it"""
    return [("bf16", t) for t in tiles] + [("f32", (0, 0))] + [("f16", t) for t in F16_TILES]


# NOT a tile sweep for the 16-bit types, whatever the parameters look like: rows_per_batch = 50 is neither a multiple of the row-tile height nor
# of 16, so the packed LINEAR epilogue cannot stage the row-bias groups and csrc/gemm_plan.h plans every bf16 / f16 case NARROW (wide = 0) - and the narrow
# per-lane epilogue only exists for tile configs 1 / 2 (gemm_plan.h::gemm_executed_cfg rewrites the rest).  All (tile, ring) pairs below run 128x128 or
# 128x64 with the per-lane epilogue and a 2-deep ring.  The test stays as the narrow epilogue's check on six shapes; the packed epilogue on the tiles it
# names is tests/test_gemm_epilogues_gpu.py, and tests/test_gemm_cases.py pins on the CPU what both launch.
@pytest.mark.parametrize("dt,tile_ring", _dt_tiles(PLAIN_TILES))
@pytest.mark.parametrize("M,N,K", [(256, 128, 128), (300, 320, 320), (154, 64, 768), (8, 256, 64), (1000, 960, 40), (513, 4, 576)])
def test_gemm_plain(hip, emu, dt, tile_ring, M, N, K):
    T = DT[dt]
    a, w = rnd((M, K), T, 1), rnd((N, K), T, 2, 1 / math.sqrt(K))
    bias, res = rnd((N,), torch.float32, 3), rnd((M, N), T, 4)
    rpb = 50
    rowb = rnd(((M + rpb - 1) // rpb, N), torch.float32, 5)
    kw = dict(M=M, N=N, K=K, lda=K, ldw=K, ldo=N, ldr=N, rows_per_batch=rpb, out_scale=0.75)
    hip.set_tuning(1, tile_ring[0])
    hip.set_tuning(2, tile_ring[1])
    try:
        o_h = torch.full((M, N), float("nan"), dtype=T, device="cuda")
        hip.gemm(a.cuda(), w.cuda(), o_h, bias=bias.cuda(), rowbias=rowb.cuda(), residual=res.cuda(), **kw)
        torch.cuda.synchronize()
    finally:
        hip.set_tuning(1, 0)
        hip.set_tuning(2, 0)
    o_e = torch.zeros(M, N, dtype=T)
    emu.gemm(a, w, o_e, bias=bias, rowbias=rowb, residual=res, **kw)
    close(o_h, o_e, f"gemm {dt} {M}x{N}x{K} tile/ring={tile_ring}", RTOL[dt])


# Six of the nine shapes take the NARROW epilogue on config 1 / 2 in bf16 / f16 for the same reason as test_gemm_plain: the row bias has one group per
# frame, and Hout * Wout = 120, 1, 1, 45, 9 is no multiple of 16 (or N = 4 is no multiple of 8).  Only the first three shapes - frames of 64, 192 and
# 64 output rows, all CONV3X3 - keep the wide epilogue and run the forced tile: no CONV3X3_UP2 case and no single-pixel case does.  The wide epilogue of
# every geometry on every tile is tests/test_gemm_epilogues_gpu.py.
@pytest.mark.parametrize("dt,tile_ring", _dt_tiles(CONV_TILES))
@pytest.mark.parametrize("mode,stride,frames,H,W,Cin,Cout", [
    (1, 1, 3, 8, 8, 64, 64), (1, 1, 2, 16, 12, 128, 320), (1, 2, 2, 16, 16, 64, 128), (2, 1, 2, 6, 5, 64, 64),
    (1, 1, 5, 1, 1, 64, 64), (1, 1, 1, 32, 32, 192, 4), (1, 2, 3, 2, 2, 64, 64), (3, 1, 2, 3, 5, 64, 64), (3, 1, 1, 2, 2, 64, 128)])
def test_gemm_conv(hip, emu, dt, tile_ring, mode, stride, frames, H, W, Cin, Cout):
    T = DT[dt]
    if mode == 3:                      # nearest upsample to a forwarded, non-2x size (odd resolutions)
        mode, Ho, Wo = 2, 2 * H - 1, 2 * W - 1
    else:
        Ho, Wo = (2 * H, 2 * W) if mode == 2 else ((H - 1) // stride + 1, (W - 1) // stride + 1)
    M, K = frames * Ho * Wo, 9 * Cin
    x, w = rnd((frames * H * W, Cin), T, 1), rnd((Cout, K), T, 2, 1 / math.sqrt(K))
    bias = rnd((Cout,), torch.float32, 3)
    rowb = rnd((frames, Cout), torch.float32, 5)
    res = rnd((M, Cout), T, 6)
    conv = dict(Hout=Ho, Wout=Wo, Hin=H, Win=W, Cin=Cin, stride=stride)
    kw = dict(M=M, N=Cout, K=K, lda=Cin, ldw=K, ldo=Cout, ldr=Cout, mode=mode, conv=conv, rows_per_batch=Ho * Wo)
    o_h = torch.full((M, Cout), float("nan"), dtype=T, device="cuda")
    hip.set_tuning(1, tile_ring[0])
    hip.set_tuning(2, tile_ring[1])
    try:
        hip.gemm(x.cuda(), w.cuda(), o_h, bias=bias.cuda(), rowbias=rowb.cuda(), residual=res.cuda(), **kw)
        torch.cuda.synchronize()
    finally:
        hip.set_tuning(1, 0)
        hip.set_tuning(2, 0)
    o_e = torch.zeros(M, Cout, dtype=T)
    emu.gemm(x, w, o_e, bias=bias, rowbias=rowb, residual=res, **kw)
    close(o_h, o_e, f"conv {dt} mode={mode} s={stride} {frames}x{H}x{W} {Cin}->{Cout}", RTOL[dt])


# (GEGLU, HEADS, activation, LayerNorm fold and dual-source K below are judged by one global relative L2 here; per element, per form and in guarded buffers they are the
# groups geglu / heads / act / lnfold / dualk of tests/gemm_cases.py, launched by tests/test_gemm_epilogues_gpu.py)
@pytest.mark.parametrize("dt", ["bf16", "f32", "f16"])
def test_gemm_geglu(hip, emu, dt):
    T = DT[dt]
    M, C = 200, 64
    a, w, bias = rnd((M, C), T, 1), rnd((8 * C, C), T, 2, 1 / 8), rnd((8 * C,), torch.float32, 3)
    kw = dict(M=M, N=8 * C, K=C, lda=C, ldw=C, ldo=4 * C, epilogue=1)
    o_h = torch.full((M, 4 * C), float("nan"), dtype=T, device="cuda")
    hip.gemm(a.cuda(), w.cuda(), o_h, bias=bias.cuda(), **kw)
    torch.cuda.synchronize()
    o_e = torch.zeros(M, 4 * C, dtype=T)
    emu.gemm(a, w, o_e, bias=bias, **kw)
    close(o_h, o_e, f"geglu {dt}", RTOL[dt])


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 7, 8, 10])
@pytest.mark.parametrize("M", [300, 4096, 8192])
def test_gemm_geglu_every_tile(hip, emu, M, tile):
    """GEGLU + folded LayerNorm at the SD-1.5 width (N = 2560, K = 320) with every tile configuration and with the library's own
    choice at row counts the UNet does not issue (round 3: the automatic choice at M = 4096 / 8192 was the 128x320 tile over 2x4
    waves, whose waves own 5 column blocks - the value / gate pairing broke and the output stayed unwritten)"""
    T, C, hid = torch.bfloat16, 320, 1280
    a, w, bias = rnd((M, C), T, 1), rnd((2 * hid, C), T, 2, C ** -0.5), rnd((2 * hid,), torch.float32, 3)
    cs = w.float().sum(dim=1)
    st = torch.stack([a.float().mean(dim=1), (a.float().var(dim=1, unbiased=False) + 1e-5).rsqrt()], dim=1).contiguous()
    kw = dict(M=M, N=2 * hid, K=C, lda=C, ldw=C, ldo=hid, epilogue=1)
    o_h = torch.full((M, hid), float("nan"), dtype=T, device="cuda")
    hip.gemm(a.cuda(), w.cuda(), o_h, bias=bias.cuda(), ln_stats=st.cuda(), ln_colsum=cs.cuda(), tile=tile, **kw)
    torch.cuda.synchronize()
    n = min(M, 384)
    o_e = torch.zeros(n, hid, dtype=T)
    emu.gemm(a[:n], w, o_e, bias=bias, ln_stats=st[:n], ln_colsum=cs, **dict(kw, M=n))
    assert torch.isfinite(o_h.float()).all(), f"GEGLU M={M} tile={tile}: unwritten / non-finite output"
    close(o_h[:n], o_e, f"geglu M={M} tile={tile}", RTOL["bf16"])


def test_gemm_geglu_rejects_odd_wave_tiles(hip):
    T, C, hid, M = torch.bfloat16, 320, 1280, 256
    a, w = rnd((M, C), T, 1).cuda(), rnd((2 * hid, C), T, 2, C ** -0.5).cuda()
    o = torch.empty(M, hid, dtype=T, device="cuda")
    hip.gemm(a, w, o, M=M, N=2 * hid, K=C, lda=C, ldw=C, ldo=hid, epilogue=1, tile=6)      # a forced config 6 is replaced, not launched
    torch.cuda.synchronize()
    assert torch.isfinite(o.float()).all()


def _retired_tile_operands():
    M, N, K = 300, 320, 320
    T = torch.bfloat16
    ops = dict(a=rnd((M, K), T, 1).cuda(), w=rnd((N, K), T, 2, 1 / math.sqrt(K)).cuda(), bias=rnd((N,), torch.float32, 3).cuda(), res=rnd((M, N), T, 4).cuda())
    return ops, dict(M=M, N=N, K=K, lda=K, ldw=K, ldo=N, ldr=N)


def _retired_tile_run(hip, ops, kw, tile):
    o = torch.full((kw["M"], kw["N"]), float("nan"), dtype=torch.bfloat16, device="cuda")
    hip.gemm(ops["a"], ops["w"], o, bias=ops["bias"], residual=ops["res"], tile=tile, **kw)
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("tile", [12, 13, 14])
def test_gemm_retired_mi32_tiles_are_refused(hip, tile):
    """tile configs 12 / 13 / 14 (the retired 32x32x16 main loop) are not built: the call is refused with the number named, before any launch"""
    from followyourclick_amd._lib import FycError
    ops, kw = _retired_tile_operands()
    o = torch.full((kw["M"], kw["N"]), float("nan"), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(FycError, match=rf"tile config {tile}\b"):
        hip.gemm(ops["a"], ops["w"], o, bias=ops["bias"], residual=ops["res"], tile=tile, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(o.float()).all(), f"tile {tile}: the refused call wrote output"


@pytest.mark.parametrize("tile,twin", [(21, 5), (22, 6), (23, 7), (31, 6)])
def test_gemm_retired_loop_tiles_run_their_twins(hip, tile, twin):
    """tile configs 21 / 22 / 23 / 31 (the retired round-4 main loops) run the one-phase tile of the same shape: bitwise the twin's output"""
    ops, kw = _retired_tile_operands()
    got, want = _retired_tile_run(hip, ops, kw, tile), _retired_tile_run(hip, ops, kw, twin)
    assert torch.isfinite(want.float()).all()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"tile {tile} vs {twin}: {(got != want).sum().item()} elements differ"


@pytest.mark.parametrize("dt", ["bf16", "f32", "f16"])
@pytest.mark.parametrize("tokens,heads,d", [(64, 8, 8), (77, 8, 40), (20, 2, 160)])
def test_gemm_heads(hip, emu, dt, tokens, heads, d):
    T = DT[dt]
    Bn, C = 3, heads * d
    M, ld = Bn * tokens, ((tokens + 7) // 8) * 8
    a, w, bias = rnd((M, 64), T, 1), rnd((3 * C, 64), T, 2, 1 / 8), rnd((3 * C,), torch.float32, 3)

    def outs(dev):
        return [torch.zeros(Bn, heads, tokens, d, dtype=T, device=dev), torch.zeros(Bn, heads, tokens, d, dtype=T, device=dev),
                torch.zeros(Bn, heads, d, ld, dtype=T, device=dev)]
    oh, oe = outs("cuda"), outs("cpu")
    kw = dict(M=M, N=3 * C, K=64, lda=64, ldw=64, epilogue=2)
    hip.gemm(a.cuda(), w.cuda(), None, bias=bias.cuda(), heads=dict(seg_cols=C, heads=heads, tokens=tokens, outs=oh, transposed=[0, 0, 1], ld=[0, 0, ld]), **kw)
    torch.cuda.synchronize()
    emu.gemm(a, w, None, bias=bias, heads=dict(seg_cols=C, heads=heads, tokens=tokens, outs=oe, transposed=[0, 0, 1], ld=[0, 0, ld]), **kw)
    for i, n in enumerate("qkv"):
        close(oh[i], oe[i], f"heads {dt} seg {n}", RTOL[dt])


@pytest.mark.parametrize("tile", [1, 5, 6, 11])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gemm_heads_every_wide_tile(hip, emu, dt, tile):
    """the wide head-split epilogue (q / k as 16-byte runs along the head dim, V^T along the token axis) at the SD-1.5 level-0 width
    (N = 3 x 320, d = 40) with a folded LayerNorm, on every tile config the engine may give it - incl. 128x160 (round 6)"""
    T = DT[dt]
    Bn, heads, d, tokens, K = 5, 8, 40, 64, 320
    C, M = heads * d, Bn * tokens
    a, w, bias = rnd((M, K), T, 1), rnd((3 * C, K), T, 2, 1 / math.sqrt(K)), rnd((3 * C,), torch.float32, 3)
    st = torch.stack([0.1 * rnd((M,), torch.float32, 4), 1 + 0.1 * rnd((M,), torch.float32, 5).abs()], dim=1).contiguous()
    cs = rnd((3 * C,), torch.float32, 6)

    def outs(dev):
        return [torch.zeros(Bn, heads, tokens, d, dtype=T, device=dev), torch.zeros(Bn, heads, tokens, d, dtype=T, device=dev),
                torch.zeros(Bn, heads, d, tokens, dtype=T, device=dev)]
    oh, oe = outs("cuda"), outs("cpu")
    kw = dict(M=M, N=3 * C, K=K, lda=K, ldw=K, epilogue=2)
    hip.gemm(a.cuda(), w.cuda(), None, bias=bias.cuda(), ln_stats=st.cuda(), ln_colsum=cs.cuda(), tile=tile,
             heads=dict(seg_cols=C, heads=heads, tokens=tokens, outs=oh, transposed=[0, 0, 1], ld=[0, 0, tokens]), **kw)
    torch.cuda.synchronize()
    emu.gemm(a, w, None, bias=bias, ln_stats=st, ln_colsum=cs, heads=dict(seg_cols=C, heads=heads, tokens=tokens, outs=oe, transposed=[0, 0, 1], ld=[0, 0, tokens]), **kw)
    for i, n in enumerate("qkv"):
        close(oh[i], oe[i], f"heads {dt} tile {tile} seg {n}", RTOL[dt])


@pytest.mark.parametrize("dt", ["bf16", "f32", "f16"])
@pytest.mark.parametrize("M,C", [(300, 64), (1000, 320)])
def test_gemm_dual_source_k(hip, emu, dt, M, C):
    """A = [tok | hidden]: the merged FF2 + output projection GEMM (K = C + 4C)"""
    T = DT[dt]
    tok, hid = rnd((M, C), T, 1), rnd((M, 4 * C), T, 2)
    w, bias, res = rnd((C, 5 * C), T, 3, 1 / math.sqrt(5 * C)), rnd((C,), torch.float32, 4), rnd((M, C), T, 5)
    kw = dict(M=M, N=C, K=5 * C, lda=C, ldw=5 * C, ldo=C, ldr=C, k_split=C, lda2=4 * C)
    o_h = torch.full((M, C), float("nan"), dtype=T, device="cuda")
    hip.gemm(tok.cuda(), w.cuda(), o_h, bias=bias.cuda(), residual=res.cuda(), a2=hid.cuda(), **kw)
    torch.cuda.synchronize()
    o_e = torch.zeros(M, C, dtype=T)
    emu.gemm(tok, w, o_e, bias=bias, residual=res, a2=hid, **kw)
    close(o_h, o_e, f"dual-source gemm {dt} M={M} C={C}", RTOL[dt])


@pytest.mark.parametrize("dt", ["bf16", "f32", "f16"])
def test_gemm_batched(hip, emu, dt):
    """the materialised-attention shape: S[z] = q[z] k[z]^T * scale, d = 40"""
    T = DT[dt]
    Z, N, d = 6, 100, 40
    q, k = rnd((Z, N, d), T, 1), rnd((Z, N, d), T, 2)
    ldo = 104
    kw = dict(M=N, N=N, K=d, lda=d, ldw=d, ldo=ldo, batch=Z, stride_a=N * d, stride_w=N * d, stride_o=N * ldo, out_scale=d ** -0.5)
    o_h = torch.zeros(Z, N, ldo, dtype=T, device="cuda")
    hip.gemm(q.cuda(), k.cuda(), o_h, **kw)
    torch.cuda.synchronize()
    o_e = torch.zeros(Z, N, ldo, dtype=T)
    emu.gemm(q, k, o_e, **kw)
    close(o_h, o_e, f"bgemm {dt}", RTOL[dt])


@pytest.mark.parametrize("dt", ["bf16", "f32", "f16"])
@pytest.mark.parametrize("Z,M,N,K", [(5, 128, 128, 64), (3, 256, 512, 256), (4, 64, 64, 64), (2, 1024, 512, 1024)])
def test_gemm_batched_aligned(hip, emu, dt, Z, M, N, K):
    """the VAE's materialised attention at aligned sizes (tokens and channels multiples of 8: the 16-byte bf16 epilogue; round 4
    first shipped it without the batch offset on the output and every batch element landed on element 0 - only the N = 100 case
    above, which takes the narrow epilogue, was tested)"""
    T = DT[dt]
    a, w = rnd((Z, M, K), T, 1), rnd((Z, N, K), T, 2)
    kw = dict(M=M, N=N, K=K, lda=K, ldw=K, ldo=N, batch=Z, stride_a=M * K, stride_w=N * K, stride_o=M * N, out_scale=K ** -0.5)
    o_h = torch.full((Z, M, N), float("nan"), dtype=T, device="cuda")
    hip.gemm(a.cuda(), w.cuda(), o_h, **kw)
    torch.cuda.synchronize()
    o_e = torch.zeros(Z, M, N, dtype=T)
    emu.gemm(a, w, o_e, **kw)
    close(o_h, o_e, f"bgemm aligned {dt} {Z}x{M}x{N}x{K}", RTOL[dt])


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,nq,nk,d,div", [(2, 8, 256, 256, 40, 1), (4, 8, 64, 77, 40, 2), (1, 8, 100, 300, 80, 1), (2, 8, 64, 64, 160, 1),
                                            (2, 8, 16, 16, 8, 1), (3, 2, 33, 93, 32, 3), (1, 8, 1024, 1024, 40, 1), (2, 8, 1, 1, 32, 1)])
def test_attention(hip, emu, B, H, nq, nk, d, div):
    T = torch.bfloat16
    kvB, ldvt = (B + div - 1) // div, ((nk + 7) // 8) * 8
    q, k = rnd((B * H, nq, d), T, 1), rnd((kvB * H, nk, d), T, 2)
    vt = torch.zeros(kvB * H, d, ldvt, dtype=T)
    vt[..., :nk] = rnd((kvB * H, d, nk), T, 3)
    kw = dict(batch=B, heads=H, n_q=nq, n_k=nk, d=d, ldo=H * d, ldvt=ldvt, scale=d ** -0.5, kv_batch_div=div)
    o_h = torch.full((B * nq, H * d), float("nan"), dtype=T, device="cuda")
    hip.attention(q.cuda(), k.cuda(), vt.cuda(), o_h, **kw)
    torch.cuda.synchronize()
    o_e = torch.zeros(B * nq, H * d, dtype=T)
    emu.attention(q, k, vt, o_e, **kw)
    close(o_h, o_e, f"attn B{B} H{H} nq{nq} nk{nk} d{d}", 6e-3)
    # decoupled IP-Adapter form: o += 0.7 * attn
    o_h2, o_e2 = o_h.clone(), o_e.clone()
    hip.attention(q.cuda(), k.cuda(), vt.cuda(), o_h2, accumulate=True, o_scale=0.7, **kw)
    torch.cuda.synchronize()
    emu.attention(q, k, vt, o_e2, accumulate=True, o_scale=0.7, **kw)
    close(o_h2, o_e2, f"attn-accumulate d{d}", 8e-3)


def test_attention_peaked_softmax(hip, emu):
    """rows whose max jumps by orders of magnitude between key tiles exercise the online rescale"""
    T = torch.bfloat16
    B, H, n, d = 1, 8, 256, 40
    q, k = rnd((B * H, n, d), T, 1), rnd((B * H, n, d), T, 2)
    k[:, 200] = (q[:, 17].float() * 4).to(T)   # one key aligned with one query, late in the sequence
    k[:, 3] = (q[:, 90].float() * 6).to(T)
    vt = rnd((B * H, d, n), T, 3)
    kw = dict(batch=B, heads=H, n_q=n, n_k=n, d=d, ldo=H * d, ldvt=n, scale=d ** -0.5)
    o_h = torch.zeros(B * n, H * d, dtype=T, device="cuda")
    hip.attention(q.cuda(), k.cuda(), vt.cuda(), o_h, **kw)
    torch.cuda.synchronize()
    o_e = torch.zeros(B * n, H * d, dtype=T)
    emu.attention(q, k, vt, o_e, **kw)
    close(o_h, o_e, "attn peaked", 6e-3)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("d,n", [(40, 320), (80, 200), (160, 152)])
def test_attention_propagates_non_finite_inputs(hip, dt, d, n):
    """round-5 advisor: the attention sources are built with -fno-honor-nans (no sNaN-quieting maxima in the softmax).  A NaN or an
    overflowed (Inf) query / key from an upstream layer must still come out NON-FINITE - bench.py's isfinite() assert and the parity
    tests rely on it - and must not leak into the other rows.  (FYC_ATTN_HONOR_NANS=1 at build time restores the quieting maxima.)"""
    T = DT[dt]
    B, H = 1, 2
    q, k, vt = rnd((B * H, n, d), T, 1), rnd((B * H, n, d), T, 2), rnd((B * H, d, n), T, 3)
    q[0, 5, 3] = float("nan")            # one NaN query element: query row 5 of head 0
    q[1, 70, 0] = float("inf")           # an overflowed query element: row 70 of head 1 (inf * finite key -> +-inf scores -> NaN after the max)
    kw = dict(batch=B, heads=H, n_q=n, n_k=n, d=d, ldo=H * d, ldvt=n, scale=d ** -0.5)
    o = torch.zeros(B * n, H * d, dtype=T, device="cuda")
    hip.attention(q.cuda(), k.cuda(), vt.cuda(), o, **kw)
    torch.cuda.synchronize()
    o = o.float().cpu().reshape(n, H, d)
    assert not torch.isfinite(o[5, 0]).any(), "a NaN query must give a non-finite output row"
    assert not torch.isfinite(o[70, 1]).all(), "an Inf query must give a non-finite output row"
    clean = torch.ones(n, H, dtype=torch.bool)
    clean[5, 0] = clean[70, 1] = False
    assert torch.isfinite(o[clean]).all(), "non-finite values leaked into other rows"
    # a NaN KEY poisons every query of its head (as in torch), not the other head
    q2 = rnd((B * H, n, d), T, 1)
    k2 = k.clone()
    k2[1, n - 3, 1] = float("nan")
    o2 = torch.zeros(B * n, H * d, dtype=T, device="cuda")
    hip.attention(q2.cuda(), k2.cuda(), vt.cuda(), o2, **kw)
    torch.cuda.synchronize()
    o2 = o2.float().cpu().reshape(n, H, d)
    assert torch.isfinite(o2[:, 0]).all()
    assert (~torch.isfinite(o2[:, 1])).any(dim=-1).all(), "a NaN key must reach every query row of its head"


@pytest.mark.parametrize("nk", [150, 330])
@pytest.mark.parametrize("d", list(range(8, 161, 8)))
def test_attention_every_head_dim(hip, emu, d, nk):
    """every supported head dim (multiples of 8 up to 160): 32-wide + 16-wide k-steps, the in-MFMA max subtraction (d % 16 == 8)
    and the plain one, the row of ones that carries the softmax denominator; 2.5 key tiles with a ragged tail (no steady-state tile) and
    5.2 key tiles (three tiles of the steady-state loop of round 5, then the general one)"""
    T = torch.bfloat16
    B, H, nq = 2, 3, 80
    ldvt = ((nk + 7) // 8) * 8
    q, k = rnd((B * H, nq, d), T, 11), rnd((B * H, nk, d), T, 12)
    vt = torch.zeros(B * H, d, ldvt, dtype=T)
    vt[..., :nk] = rnd((B * H, d, nk), T, 13)
    kw = dict(batch=B, heads=H, n_q=nq, n_k=nk, d=d, ldo=H * d, ldvt=ldvt, scale=d ** -0.5)
    for qt in (2, 3, 4):
        hip.set_tuning(3, qt)
        try:
            o_h = torch.full((B * nq, H * d), float("nan"), dtype=T, device="cuda")
            hip.attention(q.cuda(), k.cuda(), vt.cuda(), o_h, **kw)
            torch.cuda.synchronize()
        finally:
            hip.set_tuning(3, 0)
        o_e = torch.zeros(B * nq, H * d, dtype=T)
        emu.attention(q, k, vt, o_e, **kw)
        close(o_h, o_e, f"attn d{d} qt{qt}", 6e-3)


@pytest.mark.parametrize("d", [24, 40, 64, 80, 160])
@pytest.mark.parametrize("offset", [-120.0, 0.0, 90.0])
def test_attention_score_offsets_and_late_spikes(hip, emu, d, offset):
    """the running max is only moved when a score exceeds it by 2^6 and the first key block always fixes it: scores far from 0
    (a common offset of +-100 in the exponent), a key that beats everything in the LAST tile, one in the first tile, and rows whose
    maximum creeps up a little in every tile (below the threshold) must all come out right"""
    T = torch.bfloat16
    B, H, n = 1, 4, 448
    g = torch.Generator().manual_seed(5)
    q, k = rnd((B * H, n, d), T, 1), rnd((B * H, n, d), T, 2)
    # a shared direction u: q.u = 1 for every query, k.u = offset / scale -> every score moves by `offset` (natural-log units * scale)
    u = torch.zeros(d)
    u[0] = 1.0
    qf, kf = q.float(), k.float()
    qf[..., 0] = 1.0
    kf[..., 0] = offset * math.sqrt(d) / math.log2(math.e)       # offset is in log2 units
    kf[:, 440] = kf[:, 440] + qf[:, 17] * 5                       # late spike for query 17
    kf[:, 2] = kf[:, 2] + qf[:, 90] * 7                           # early spike for query 90
    ramp = torch.arange(n).float()[None, :, None] * 0.004        # slowly growing scores for all queries
    kf[..., 1] = ramp[..., 0]
    qf[..., 1] = 2.0
    q, k = qf.to(T), kf.to(T)
    vt = rnd((B * H, d, n), T, 3)
    kw = dict(batch=B, heads=H, n_q=n, n_k=n, d=d, ldo=H * d, ldvt=n, scale=d ** -0.5)
    o_h = torch.zeros(B * n, H * d, dtype=T, device="cuda")
    hip.attention(q.cuda(), k.cuda(), vt.cuda(), o_h, **kw)
    torch.cuda.synchronize()
    o_e = torch.zeros(B * n, H * d, dtype=T)
    emu.attention(q, k, vt, o_e, **kw)
    close(o_h, o_e, f"attn offsets d{d} off{offset}", 8e-3)


@pytest.mark.parametrize("dt,height", [("bf16", 150.0), ("bf16", 40.0), ("f16", 40.0), ("f16", 18.0)])
@pytest.mark.parametrize("key", [416 + 3, 416 + 12, 416 + 20, 416 + 29, 200, 31, 63 - 8])
@pytest.mark.parametrize("d", [40, 160])
def test_attention_late_spike_in_every_lane_quad(hip, emu, dt, height, key, d):
    """One key beats a query's running maximum by `height` (log2 units) late in the sequence, for keys held by each of the four lane
    quads of a query column (key % 32 // 8).  Rounds 1-4: hipcc folded the cross-half step of the kernel's quad maximum away
    (fyc_common.h::swap32_max), the running maximum ignored the keys of lanes 32..63 (quads 2, 3), the rescale never fired for them
    and the probability became 2^height: infinite in f16 from 2^16, in bf16 from 2^128 - NaN rows; below that the result was right by
    the grace of the exponent range.  Now every quad moves the maximum and the probabilities stay <= 2^6."""
    T = DT[dt]
    B, H, n, qsel = 1, 4, 448, 17
    q, k = rnd((B * H, n, d), T, 1), rnd((B * H, n, d), T, 2)
    qf, kf = q.float(), k.float()
    unit = (qf[:, qsel] * qf[:, qsel]).sum(-1, keepdim=True) * d ** -0.5 * math.log2(math.e)       # score of key = query, log2 units
    kf[:, key] = kf[:, key] + qf[:, qsel] * (height / unit)
    q, k, vt = qf.to(T), kf.to(T), rnd((B * H, d, n), T, 3)
    kw = dict(batch=B, heads=H, n_q=n, n_k=n, d=d, ldo=H * d, ldvt=n, scale=d ** -0.5)
    o_h = torch.zeros(B * n, H * d, dtype=T, device="cuda")
    hip.attention(q.cuda(), k.cuda(), vt.cuda(), o_h, **kw)
    torch.cuda.synchronize()
    o_e = torch.zeros(B * n, H * d, dtype=T)
    emu.attention(q, k, vt, o_e, **kw)
    close(o_h, o_e, f"attn {dt} d{d} spike of 2^{height} at key {key} (quad {key % 32 // 8})", 8e-3 if dt == "bf16" else 2e-3)
    if height >= 40:                                   # the spiking query's output is that key's value row (the rest weighs < 2^-30)
        got, ref = o_h.float().cpu().reshape(n, H, d)[qsel], vt.float()[:, :, key]
        assert (got - ref).abs().max().item() < (6e-2 if dt == "bf16" else 8e-3)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("clips,F,P,H,d", [(2, 16, 64, 8, 40), (1, 8, 16, 8, 8), (2, 4, 1, 8, 32), (1, 24, 9, 8, 80), (1, 16, 5, 8, 160), (1, 32, 4, 8, 16)])
def test_temporal_attention(hip, emu, dt, clips, F, P, H, d):
    T = DT[dt]
    C = H * d
    qkv = rnd((clips * F * P, 3 * C), T, 1)
    kw = dict(clips=clips, frames=F, pixels=P, heads=H, d=d, scale=d ** -0.5)
    o_h = torch.full((clips * F * P, C), float("nan"), dtype=T, device="cuda")
    hip.temporal_attention(qkv.cuda(), o_h, **kw)
    torch.cuda.synchronize()
    o_e = torch.zeros(clips * F * P, C, dtype=T)
    emu.temporal_attention(qkv, o_e, **kw)
    close(o_h, o_e, f"tattn {dt} F{F} P{P} d{d}", 6e-3 if dt == "bf16" else 2e-5)


def _temporal_operands(with_pe, seed=0, T=torch.bfloat16):
    from followyourclick_amd.engine.weights import Packed, pack_temporal_block
    H, d, F = 8, 40, 16
    C = H * d
    att = Packed(qkv_f=((rnd((3 * C, C), torch.float32, seed + 1) * C ** -0.5).to(T), rnd((3 * C,), torch.float32, seed + 2) * 0.1, None),
                 pe_w=rnd((24, 3 * C), torch.float32, seed + 3) * 0.5 if with_pe else None,
                 o_w=(rnd((C, C), torch.float32, seed + 4) * C ** -0.5).to(T), o_b=rnd((C,), torch.float32, seed + 5) * 0.1)
    att["qkv_f"] = (att.qkv_f[0], att.qkv_f[1], att.qkv_f[0].float().sum(dim=1))
    return pack_temporal_block(att, H, F)


@pytest.mark.parametrize("rr", [True, False])
@pytest.mark.parametrize("with_pe", [True, False])
@pytest.mark.parametrize("clips,P", [(2, 64), (1, 8), (3, 4096)])
def test_temporal_block_fused(hip, emu, clips, P, with_pe, rr):
    """fyc_temporal_block (row statistics + LayerNorm-folded QKV + attention over frames + output projection + residual in
    one kernel) against the torch specification on the per-head operands of engine/weights.py::pack_temporal_block;
    rr: the register-resident kernel on the packed weight stream (csrc/temporal_block_rr.hip) against the specification
    computed from the UNPACKED stream"""
    T, H, d, F = torch.bfloat16, 8, 40, 16
    C = H * d
    ops_e = _temporal_operands(with_pe)
    assert "wstream" in ops_e
    if not rr:
        del ops_e["wstream"]
    ops_h = {k: (v.cuda() if v is not None else None) for k, v in ops_e.items()}
    x = (rnd((clips * F * P, C), torch.float32, 6) * 1.5 + 0.3).to(T)
    kw = dict(clips=clips, frames=F, pixels=P, heads=H, d=d, scale=d ** -0.5)
    shape = dict(clips=clips, frames=F, pixels=P, heads=H, d=d)
    assert hip.temporal_block_supported(T, **shape)
    assert not hip.temporal_block_supported(T, **dict(shape, pixels=P + 1)) and not hip.temporal_block_supported(torch.float32, **shape)
    o_h = torch.full((clips * F * P, C), float("nan"), dtype=T, device="cuda")
    hip.temporal_block(x.cuda(), o_h, **ops_h, **kw)
    torch.cuda.synchronize()
    if P > 64:                                           # the specification on a slice of the pixels (tiles are independent)
        sel = torch.arange(0, P, 61)[:8]
        xs = x.reshape(clips, F, P, C)[:, :, sel].reshape(-1, C)
        o_e = torch.zeros(clips * F * len(sel), C, dtype=T)
        emu.temporal_block(xs, o_e, **ops_e, **dict(kw, pixels=len(sel)))
        o_h = o_h.reshape(clips, F, P, C)[:, :, sel.cuda()].reshape(-1, C)
    else:
        o_e = torch.zeros(clips * F * P, C, dtype=T)
        emu.temporal_block(x, o_e, **ops_e, **kw)
    close(o_h, o_e, f"temporal block clips{clips} P{P} pe{with_pe}", 6e-3)
    with pytest.raises(Exception, match="in-place"):
        xc = x.cuda()
        hip.temporal_block(xc, xc, **ops_h, **kw)


@pytest.mark.parametrize("with_gn,with_res", [(False, True), (True, False), (True, True), (False, False)])
@pytest.mark.parametrize("rows,N,K", [(128, 320, 320), (4096, 640, 640), (131072, 320, 320), (32768, 640, 640), (512, 320, 640), (512, 640, 320)])
def test_panel_linear(hip, emu, rows, N, K, with_gn, with_res):
    """fyc_panel_linear (register-resident rows, fragment-ordered weight stream, optional GroupNorm of the input on the operand
    registers, bias + residual) against the torch specification on the stream of engine/weights.py::pack_panel_linear"""
    from followyourclick_amd.engine.weights import pack_panel_linear
    T = torch.bfloat16
    w = (rnd((N, K), torch.float32, 1) * K ** -0.5).to(T)
    ws = pack_panel_linear(w)
    bias = rnd((N,), torch.float32, 2) * 0.2
    x = (rnd((rows, K), torch.float32, 3) * 1.3 + 0.4).to(T)
    res = rnd((rows, N), T, 4) if with_res else None
    rps = 128 if rows <= 512 else 4096                       # rows per GroupNorm sample (a frame)
    kw = {}
    if with_gn:
        xs = x.double().reshape(rows // rps, rps, K)
        # two statistics samples per norm sample (the kernel folds them): halves of the rows
        half = xs.reshape(rows // rps, 2, rps // 2, K)
        cs = torch.stack([half.sum(2), (half * half).sum(2)], dim=-1).reshape(-1, K, 2).contiguous()
        kw = dict(gn_cs=cs, gn_gamma=rnd((K,), torch.float32, 5) * 0.2 + 1.0, gn_beta=rnd((K,), torch.float32, 6) * 0.2,
                  gn_rows_per_sample=rps, gn_stat_samples=2, gn_groups=32, gn_eps=1e-6)
    assert hip.panel_linear_supported(T, rows=rows, N=N, K=K, gn_rows_per_sample=rps if with_gn else 0)
    assert not hip.panel_linear_supported(T, rows=rows + 64, N=N, K=K) and not hip.panel_linear_supported(T, rows=rows, N=960, K=K)
    assert not hip.panel_linear_supported(torch.float32, rows=rows, N=N, K=K) and not hip.panel_linear_supported(T, rows=rows, N=N, K=K, gn_rows_per_sample=64)
    o_h = torch.full((rows, N), float("nan"), dtype=T, device="cuda")
    hip.panel_linear(x.cuda(), o_h, wstream=ws.cuda(), rows=rows, N=N, K=K, bias=bias.cuda(), residual=res.cuda() if with_res else None,
                     **{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()})
    torch.cuda.synchronize()
    assert torch.isfinite(o_h.float()).all()
    if rows > 4096:                                            # the specification on whole samples from both ends and the middle
        sel = torch.cat([torch.arange(0, rps), torch.arange(rows // 2, rows // 2 + rps), torch.arange(rows - rps, rows)])
    else:
        sel = torch.arange(rows)
    n = len(sel)
    o_e = torch.zeros(n, N, dtype=T)
    kw_e = dict(kw)
    if with_gn:
        samp = torch.unique(sel // rps)
        kw_e["gn_cs"] = kw["gn_cs"].reshape(rows // rps, 2, K, 2)[samp].reshape(-1, K, 2)
    emu.panel_linear(x[sel], o_e, wstream=ws, rows=n, N=N, K=K, bias=bias, residual=res[sel] if with_res else None, **kw_e)
    close(o_h[sel.cuda()], o_e, f"panel linear rows{rows} N{N} K{K} gn{with_gn} res{with_res}", 5e-3)
    with pytest.raises(Exception, match="alias"):
        xc = torch.zeros(rows * max(N, K), dtype=T, device="cuda")      # one buffer as x and as out, large enough for either: the library itself must refuse it
        xc[: rows * K].copy_(x.reshape(-1))
        hip.panel_linear(xc, xc, wstream=ws.cuda(), rows=rows, N=N, K=K)


def _ff_operands(seed=0, T=torch.bfloat16):
    """a packed feed-forward (engine/weights.py::_ff layout) with the LayerNorm folded in, at the kernel's widths"""
    from followyourclick_amd.engine.weights import Packed
    C, hid = 320, 1280
    w1 = (rnd((2 * hid, C), torch.float32, seed + 1) * C ** -0.5).to(T)
    return Packed(w1=w1, b1=rnd((2 * hid,), torch.float32, seed + 2) * 0.2, cs1=w1.float().sum(dim=1).contiguous(),
                  po_w=(rnd((C, C + hid), torch.float32, seed + 3) * (C + hid) ** -0.5).to(T), po_b=rnd((C,), torch.float32, seed + 4) * 0.1)


@pytest.mark.parametrize("variant", [0])      # (round 3 had schedule variants behind fyc_set_tuning key 8; one kernel now)
@pytest.mark.parametrize("rows,with_res,with_stats", [(128, True, True), (512, False, False), (4096, True, True), (131072, True, True)])
def test_ff_block_fused(hip, emu, rows, with_res, with_stats, variant):
    """fyc_ff_block (LayerNorm statistics + FF1 + GEGLU + FF2 + merged output projection + residual + output statistics in one
    kernel) against the torch specification on the weight stream of engine/weights.py::pack_ff_block"""
    from followyourclick_amd.engine.weights import pack_ff_block
    T, C, hid = torch.bfloat16, 320, 1280
    ff = _ff_operands()
    ws = pack_ff_block(ff)
    assert ws.numel() * 2 == hip.ff_block_wstream_bytes()
    x = (rnd((rows, C), torch.float32, 6) * 1.5 + 0.3).to(T)
    x[5] = x[5] * 40 + 100                                       # a row with a large mean: the folded LayerNorm must not lose it
    res = rnd((rows, C), T, 7) if with_res else None
    assert hip.ff_block_supported(T, rows=rows, C_=C, hidden=hid, cs_rows=128 if with_stats else 0)
    assert not hip.ff_block_supported(T, rows=rows + 64, C_=C, hidden=hid) and not hip.ff_block_supported(torch.float32, rows=rows, C_=C, hidden=hid)
    assert not hip.ff_block_supported(T, rows=rows, C_=640, hidden=2560) and not hip.ff_block_supported(T, rows=rows, C_=C, hidden=hid, cs_rows=64)
    o_h = torch.full((rows, C), float("nan"), dtype=T, device="cuda")
    p_h = torch.full((rows // 128, C, 2), float("nan"), dtype=torch.float32, device="cuda") if with_stats else None
    hip.set_tuning(8, variant)
    try:
        hip.ff_block(x.cuda(), res.cuda() if with_res else None, o_h, wstream=ws.cuda(), b_out=ff.po_b.cuda(), rows=rows, C_=C, hidden=hid,
                     chan_parts=p_h, cs_rows=128 if with_stats else 0)
        torch.cuda.synchronize()
    finally:
        hip.set_tuning(8, 0)
    sel = torch.arange(rows) if rows <= 4096 else torch.cat([torch.arange(0, 256), torch.arange(rows // 2 - 128, rows // 2 + 128), torch.arange(rows - 256, rows)])
    n = len(sel)
    o_e = torch.zeros(n, C, dtype=T)
    p_e = torch.zeros(n // 128, C, 2) if with_stats else None
    emu.ff_block(x[sel], res[sel] if with_res else None, o_e, wstream=ws, b_out=ff.po_b, rows=n, C_=C, hidden=hid, chan_parts=p_e, cs_rows=128 if with_stats else 0)
    close(o_h[sel.cuda()], o_e, f"ff block rows{rows} res{with_res} v{variant}", 6e-3)
    if with_stats:
        # the statistics are of the values AS STORED by the kernel: compare with sums of its own output, tile by tile
        t = o_h.double().reshape(rows // 128, 128, C)
        own = torch.stack([t.sum(1), (t * t).sum(1)], dim=-1)
        close(p_h, own.cpu(), f"ff block statistics rows{rows} v{variant}", 2e-5)
    with pytest.raises(Exception, match="alias"):
        xc = x.cuda()
        hip.ff_block(xc, None, xc, wstream=ws.cuda(), b_out=ff.po_b.cuda(), rows=rows, C_=C, hidden=hid)


@pytest.mark.parametrize("rows", [16384, 8192])
def test_ff_block_matches_unfused_schedule(hip, emu, rows):
    """the fused kernel against the three launches it replaces (row statistics, GEGLU GEMM with the folded LayerNorm, dual-K
    output GEMM) on the device: same operands, same roundings up to the accumulation order; both are also held to the
    specification on a slice of the rows so that a failure names the side that is wrong"""
    from followyourclick_amd.engine.weights import pack_ff_block
    from followyourclick_amd import _lib as L
    T, C, hid = torch.bfloat16, 320, 1280
    ff = _ff_operands(10)
    ws = pack_ff_block(ff)
    xc = (rnd((rows, C), torch.float32, 6) * 1.2 - 0.2).to(T)
    rc = rnd((rows, C), T, 7)
    x, res = xc.cuda(), rc.cuda()
    w1, b1, cs1, po_w, po_b = (t.cuda() for t in (ff.w1, ff.b1, ff.cs1, ff.po_w, ff.po_b))
    o_f = torch.full((rows, C), float("nan"), dtype=T, device="cuda")
    hip.ff_block(x, res, o_f, wstream=ws.cuda(), b_out=po_b, rows=rows, C_=C, hidden=hid)
    st = torch.empty(rows, 2, dtype=torch.float32, device="cuda")
    hip.row_stats(x, st, rows=rows, C_=C)
    hmid = torch.full((rows, hid), float("nan"), dtype=T, device="cuda")
    hip.gemm(x, w1, hmid, M=rows, N=2 * hid, K=C, lda=C, ldw=C, ldo=hid, bias=b1, epilogue=L.EPI_GEGLU, ln_colsum=cs1, ln_stats=st)
    o_u = torch.full((rows, C), float("nan"), dtype=T, device="cuda")
    hip.gemm(x, po_w, o_u, M=rows, N=C, K=C + hid, lda=C, ldw=C + hid, ldo=C, bias=po_b, residual=res, ldr=C, a2=hmid, k_split=C, lda2=hid)
    torch.cuda.synchronize()
    n = 512
    o_e = torch.zeros(n, C, dtype=T)
    emu.ff_block(xc[:n], rc[:n], o_e, wstream=ws, b_out=ff.po_b, rows=n, C_=C, hidden=hid)
    close(o_f[:n], o_e, f"ff block vs specification rows{rows}", 6e-3)
    close(o_u[:n], o_e, f"unfused launches vs specification rows{rows}", 6e-3)
    close(o_f, o_u.cpu(), f"ff block vs unfused launches rows{rows}", 6e-3)


@pytest.mark.parametrize("rows", [65536, 8192])
def test_ff_block_is_repeatable(hip, rows):
    """the kernel has no atomics: every launch on the same operands must give the same bits, cold or warm caches.  (Round 3: the
    LayerNorm row sums went through ds_bpermute between LDS-DMA pieces and were consumed early in ~12 % of the 16-row blocks -
    output off by an ulp or two, differently on every launch; tools/ff_stress.py, profiles/r03_ff_block_race.txt)"""
    from followyourclick_amd.engine.weights import pack_ff_block
    T, C, hid = torch.bfloat16, 320, 1280
    ff = _ff_operands(11)
    ws, po_b = pack_ff_block(ff).cuda(), ff.po_b.cuda()
    x = (rnd((rows, C), torch.float32, 8) * 1.2 - 0.2).to(T).cuda()
    res = rnd((rows, C), T, 9).cuda()
    junk = torch.empty(1 << 29, dtype=torch.uint8, device="cuda")
    parts0 = out0 = None
    for it in range(24):
        if it % 3 == 1:
            junk.fill_(it)                                     # cold L2 / Infinity Cache
        out = torch.full((rows, C), float("nan"), dtype=T, device="cuda")
        parts = torch.full((rows // 128, C, 2), float("nan"), dtype=torch.float32, device="cuda")
        hip.ff_block(x, res, out, wstream=ws, b_out=po_b, rows=rows, C_=C, hidden=hid, chan_parts=parts, cs_rows=128)
        torch.cuda.synchronize()
        if out0 is None:
            out0, parts0 = out, parts
            assert torch.isfinite(out.float()).all() and torch.isfinite(parts).all()
            continue
        d = (out.view(torch.int16) != out0.view(torch.int16)).any(dim=1).sum().item()
        assert d == 0, f"launch {it}: {d} of {rows} rows differ from launch 0"
        assert torch.equal(parts, parts0), f"launch {it}: statistics differ from launch 0"


def test_temporal_block_is_repeatable(hip):
    """same for the register-resident temporal sub-block (asm-issued LDS-DMA, lane-swap reductions)"""
    T, H, d, F, clips, P = torch.bfloat16, 8, 40, 16, 2, 4096
    C = H * d
    ops_h = {k: (v.cuda() if v is not None else None) for k, v in _temporal_operands(True, seed=20).items()}
    x = (rnd((clips * F * P, C), torch.float32, 26) * 1.5 + 0.3).to(T).cuda()
    kw = dict(clips=clips, frames=F, pixels=P, heads=H, d=d, scale=d ** -0.5)
    junk = torch.empty(1 << 29, dtype=torch.uint8, device="cuda")
    out0 = None
    for it in range(16):
        if it % 3 == 1:
            junk.fill_(it)
        out = torch.full((clips * F * P, C), float("nan"), dtype=T, device="cuda")
        hip.temporal_block(x, out, **ops_h, **kw)
        torch.cuda.synchronize()
        if out0 is None:
            out0 = out
            assert torch.isfinite(out.float()).all()
            continue
        dd = (out.view(torch.int16) != out0.view(torch.int16)).any(dim=1).sum().item()
        assert dd == 0, f"launch {it}: {dd} rows differ from launch 0"


@pytest.mark.parametrize("C,gn", [(320, True), (320, False), (640, True)])
def test_panel_linear_is_repeatable(hip, C, gn):
    """same for the row-panel linear (asm-issued LDS-DMA as well)"""
    from followyourclick_amd.engine.weights import pack_panel_linear
    T = torch.bfloat16
    rps, samples = (4096, 8) if C == 320 else (1024, 16)
    rows = rps * samples
    w = rnd((C, C), torch.float32, 3, 0.05).to(T)
    ws = pack_panel_linear(w).cuda()
    bias = rnd((C,), torch.float32, 4, 0.1).cuda()
    x = (rnd((rows, C), torch.float32, 5) + 0.3).to(T).cuda()
    res = rnd((rows, C), T, 6).cuda()
    kw = {}
    if gn:
        xf = x.double().reshape(samples, rps, C)
        cs = torch.stack([xf.sum(1), (xf * xf).sum(1)], dim=-1).contiguous()        # [samples][C][2] f64
        kw = dict(gn_cs=cs, gn_gamma=(rnd((C,), torch.float32, 7) * 0.1 + 1).cuda(), gn_beta=(rnd((C,), torch.float32, 8) * 0.1).cuda(),
                  gn_rows_per_sample=rps, gn_groups=32)
    junk = torch.empty(1 << 29, dtype=torch.uint8, device="cuda")
    out0 = None
    for it in range(16):
        if it % 3 == 1:
            junk.fill_(it)
        out = torch.full((rows, C), float("nan"), dtype=T, device="cuda")
        hip.panel_linear(x, out, wstream=ws, rows=rows, N=C, K=C, bias=bias, residual=None if gn else res, **kw)
        torch.cuda.synchronize()
        if out0 is None:
            out0 = out
            assert torch.isfinite(out.float()).all()
            continue
        d = (out.view(torch.int16) != out0.view(torch.int16)).any(dim=1).sum().item()
        assert d == 0, f"launch {it}: {d} of {rows} rows differ from launch 0"


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f32", "f16"])
@pytest.mark.parametrize("samples,rps,C", [(2, 4 * 64, 320), (8, 64, 64), (2, 16 * 16, 2560), (6, 1, 128), (3, 1000, 960), (2, 37, 1920), (2, 16 * 1024, 320)])
def test_groupnorm(hip, emu, dt, samples, rps, C):
    T = DT[dt]
    rows = samples * rps
    x = (rnd((rows, C), torch.float32, 1) * 2 + 0.7).to(T)
    gamma, beta = rnd((C,), torch.float32, 2) * 0.1 + 1, rnd((C,), torch.float32, 3) * 0.1
    st_h = torch.full((samples, 32, 2), float("nan"), dtype=torch.float64, device="cuda")
    hip.gn_stats(x.cuda(), st_h, rows=rows, C_=C, groups=32, rows_per_sample=rps)
    st_e = torch.zeros(samples, 32, 2, dtype=torch.float64)
    emu.gn_stats(x, st_e, rows=rows, C_=C, groups=32, rows_per_sample=rps)
    torch.cuda.synchronize()
    close(st_h, st_e, f"gn_stats {dt} C{C}", 1e-5)
    for _ in range(3):                                # ordered reduction (no atomics): the same bits every launch
        st_2 = torch.full_like(st_h, float("nan"))
        hip.gn_stats(x.cuda(), st_2, rows=rows, C_=C, groups=32, rows_per_sample=rps)
        assert torch.equal(st_2, st_h)
    for silu in (False, True):
        y_h = torch.zeros(rows, C, dtype=T, device="cuda")
        hip.gn_apply(x.cuda(), st_h, gamma.cuda(), beta.cuda(), y_h, rows=rows, C_=C, groups=32, rows_per_sample=rps, eps=1e-5, silu=silu)
        y_e = torch.zeros(rows, C, dtype=T)
        emu.gn_apply(x, st_e, gamma, beta, y_e, rows=rows, C_=C, groups=32, rows_per_sample=rps, eps=1e-5, silu=silu)
        torch.cuda.synchronize()
        close(y_h, y_e, f"gn_apply {dt} C{C} silu={silu}", RTOL[dt])


@pytest.mark.parametrize("dt", ["bf16", "f32", "f16"])
@pytest.mark.parametrize("rows,C,pe", [(100, 320, False), (64, 64, True), (33, 1280, True), (7, 640, False)])
def test_layernorm(hip, emu, dt, rows, C, pe):
    T = DT[dt]
    x = (rnd((rows, C), torch.float32, 1) * 3 + 1).to(T)
    gamma, beta = rnd((C,), torch.float32, 2) * 0.1 + 1, rnd((C,), torch.float32, 3) * 0.1
    pet = rnd((5, C), torch.float32, 4) if pe else None
    kw = dict(rows=rows, C_=C, eps=1e-5, pe_div=3, pe_rows=5) if pe else dict(rows=rows, C_=C, eps=1e-5)
    y_h = torch.zeros(rows, C, dtype=T, device="cuda")
    hip.layernorm(x.cuda(), gamma.cuda(), beta.cuda(), y_h, pe=pet.cuda() if pe else None, **kw)
    y_e = torch.zeros(rows, C, dtype=T)
    emu.layernorm(x, gamma, beta, y_e, pe=pet, **kw)
    torch.cuda.synchronize()
    close(y_h, y_e, f"layernorm {dt} C{C}", RTOL[dt])


@pytest.mark.parametrize("dt", ["bf16", "f32", "f16"])
def test_softmax_rows(hip, emu, dt):
    T = DT[dt]
    x = (rnd((50, 104), torch.float32, 1) * 4).to(T)
    x_h = x.cuda()
    hip.softmax_rows(x_h, rows=50, cols=100, ld=104)
    x_e = x.clone()
    emu.softmax_rows(x_e, rows=50, cols=100, ld=104)
    torch.cuda.synchronize()
    close(x_h[:, :100], x_e[:, :100], f"softmax {dt}", RTOL[dt])
    assert torch.equal(x_h[:, 100:].cpu(), x[:, 100:])


@pytest.mark.parametrize("dt", ["bf16", "f32", "f16"])
def test_elementwise(hip, emu, dt):
    T = DT[dt]
    a, b = rnd((77, 64), T, 1), rnd((77, 128), T, 2)
    y_h = torch.zeros(77, 192, dtype=T, device="cuda")
    hip.concat_channels(a.cuda(), b.cuda(), y_h, rows=77, c1=64, c2=128)
    torch.cuda.synchronize()
    assert torch.equal(y_h.cpu(), torch.cat([a, b], 1))
    x = rnd((1000,), torch.float32, 3)
    y = torch.zeros(1000, device="cuda")
    hip.silu_f32(x.cuda(), y)
    close(y, torch.nn.functional.silu(x), "silu", 1e-6)
    x = rnd((10, 9), torch.float32, 4)
    y_h, y_e = torch.ones(10, 16, dtype=T, device="cuda"), torch.ones(10, 16, dtype=T)
    hip.cast_from_f32(x.cuda(), y_h, rows=10, cols=9, ld=16)
    emu.cast_from_f32(x, y_e, rows=10, cols=9, ld=16)
    torch.cuda.synchronize()
    assert torch.equal(y_h.cpu(), y_e)
    z_h = torch.zeros(10, 9, device="cuda")
    hip.cast_to_f32(y_h, z_h, rows=10, cols=9, ld=16)
    torch.cuda.synchronize()
    assert torch.equal(z_h.cpu(), y_e[:, :9].float())


@pytest.mark.parametrize("dt", ["bf16", "f32", "f16"])
@pytest.mark.parametrize("use_mask,cfg", [(True, 2), (False, 1)])
def test_unet_input_and_ddim(hip, emu, dt, use_mask, cfg):
    T = DT[dt]
    B, F, HW, CL, cp = 2, 4, 48, 4, 64
    lat, first = rnd((B, CL, F, HW), torch.float32, 1), rnd((B, CL, HW), torch.float32, 2)
    mask = (rnd((B, 1, HW), torch.float32, 3) * 2) if use_mask else None
    x_h, x_e = torch.ones(cfg * B * F * HW, cp, dtype=T, device="cuda"), torch.ones(cfg * B * F * HW, cp, dtype=T)
    hip.unet_input(lat.cuda(), mask.cuda() if use_mask else None, first.cuda(), x_h, B=B, F=F, HW=HW, c_latent=CL, c_pad=cp, cfg_dup=cfg)
    emu.unet_input(lat, mask, first, x_e, B=B, F=F, HW=HW, c_latent=CL, c_pad=cp, cfg_dup=cfg)
    torch.cuda.synchronize()
    assert torch.equal(x_h.cpu(), x_e)
    pred = rnd((cfg * B * F * HW, cp), T, 5)
    coef = torch.tensor([0.6, 0.8, 0.7, 0.714], dtype=torch.float32)
    for ptype in (0, 1, 2):
        l_h, l_e = lat.clone().cuda(), lat.clone()
        kw = dict(B=B, F=F, HW=HW, c_latent=CL, ld=cp, cfg=cfg == 2, guidance=8.0, pred_type=ptype, clip_sample=ptype == 0)
        hip.cfg_ddim_step(pred.cuda(), l_h, coef.cuda(), **kw)
        emu.cfg_ddim_step(pred, l_e, coef, **kw)
        torch.cuda.synchronize()
        close(l_h, l_e, f"cfg_ddim {dt} type{ptype}", 1e-6)


@pytest.mark.parametrize("dt", ["bf16", "f32", "f16"])
def test_vae_layout_kernels(hip, emu, dt):
    T = DT[dt]
    z = rnd((3, 4, 30), torch.float32, 1)
    x_h, x_e = torch.ones(3 * 30, 64, dtype=T, device="cuda"), torch.ones(3 * 30, 64, dtype=T)
    hip.nchw_to_nhwc(z.cuda(), x_h, N=3, C_=4, HW=30, c_pad=64, scale=1 / 0.18215)
    emu.nchw_to_nhwc(z, x_e, N=3, C_=4, HW=30, c_pad=64, scale=1 / 0.18215)
    torch.cuda.synchronize()
    close(x_h, x_e, f"nchw_to_nhwc {dt}", RTOL[dt])
    img = rnd((3 * 30, 64), T, 2)
    y_h, y_e = torch.zeros(3, 3, 30, device="cuda"), torch.zeros(3, 3, 30)
    hip.nhwc_to_nchw(img.cuda(), y_h, N=3, C_=3, HW=30, ld=64, mul=0.5, add=0.5, lo=0.0, hi=1.0)
    emu.nhwc_to_nchw(img, y_e, N=3, C_=3, HW=30, ld=64, mul=0.5, add=0.5, lo=0.0, hi=1.0)
    torch.cuda.synchronize()
    close(y_h, y_e, f"nhwc_to_nchw {dt}", 1e-6)


def test_missing_device_tensor_raises(hip):
    from followyourclick_amd._lib import FycError
    with pytest.raises(FycError):
        hip.silu_f32(torch.zeros(4), torch.zeros(4))


# ---- conditioning-encoder ops ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f32", "f16"])
@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("M,N,K", [(154, 3072, 768), (514, 320, 1280), (32, 64, 64), (77, 264, 72)])
def test_gemm_activation(hip, emu, dt, act, M, N, K):
    """LINEAR epilogue with erf-GELU / quick-GELU (CLIP MLP fc1, Resampler FF): act(a w^T + bias), then residual, then scale"""
    T = DT[dt]
    a, w = rnd((M, K), T, 1), rnd((N, K), T, 2, 2 / math.sqrt(K))
    bias, res = rnd((N,), torch.float32, 3), rnd((M, N), T, 4)
    kw = dict(M=M, N=N, K=K, lda=K, ldw=K, ldo=N, ldr=N, out_scale=1.0, act=act)
    o_h = torch.full((M, N), float("nan"), dtype=T, device="cuda")
    hip.gemm(a.cuda(), w.cuda(), o_h, bias=bias.cuda(), residual=res.cuda(), **kw)
    o_e = torch.zeros(M, N, dtype=T)
    emu.gemm(a, w, o_e, bias=bias, residual=res, **kw)
    close(o_h, o_e, f"gemm act={act} {dt} {M}x{N}x{K}", RTOL[dt])
    with pytest.raises(Exception, match="LINEAR"):
        hip.gemm(a.cuda(), w.cuda(), o_h, M=M, N=N - N % 32, K=K, lda=K, ldw=K, ldo=N, epilogue=1, act=act)


@pytest.mark.parametrize("dt", ["bf16", "f32", "f16"])
def test_softmax_rows_causal(hip, emu, dt):
    T = DT[dt]
    heads, n, ld = 3, 77, 80
    x = rnd((heads * n, ld), T, 11, 3.0)
    xh = x.clone().cuda()
    hip.softmax_rows(xh, rows=heads * n, cols=n, ld=ld, causal_rows=n)
    xe = x.clone()
    emu.softmax_rows(xe, rows=heads * n, cols=n, ld=ld, causal_rows=n)
    close(xh[:, :n], xe[:, :n], f"causal softmax {dt}", RTOL[dt])
    assert float(xh[0, 1:n].float().abs().sum()) == 0.0 and abs(float(xh[0, 0]) - 1.0) < 1e-6      # first query sees only itself
    assert torch.equal(xh[:, n:].cpu(), x[:, n:])                                                    # padding columns untouched


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_embed_tokens_and_patchify(hip, emu, dt):
    T = DT[dt]
    vocab, seq, C, B = 1000, 77, 768, 2
    table, pos = rnd((vocab, C), torch.float32, 1), rnd((seq, C), torch.float32, 2)
    ids = torch.randint(0, vocab, (B, seq), generator=torch.Generator().manual_seed(3))
    ids[0, 0], ids[1, -1] = 0, vocab - 1
    o_h = torch.empty(B * seq, C, dtype=T, device="cuda")
    hip.embed_tokens(ids.cuda(), table.cuda(), pos.cuda(), o_h, rows=B * seq, seq=seq, C_=C)
    o_e = torch.empty(B * seq, C, dtype=T)
    emu.embed_tokens(ids, table, pos, o_e, rows=B * seq, seq=seq, C_=C)
    assert torch.equal(o_h.cpu(), o_e)                              # one rounding of an f32 sum: bit-exact
    img = rnd((B, 3, 28, 42), torch.float32, 5)
    P, ld = 14, 592
    p_h = torch.full((B * 2 * 3, ld), float("nan"), dtype=T, device="cuda")
    hip.patchify(img.cuda(), p_h, B=B, Cin=3, H=28, W=42, P=P, ld=ld)
    p_e = torch.empty(B * 2 * 3, ld, dtype=T)
    emu.patchify(img, p_e, B=B, Cin=3, H=28, W=42, P=P, ld=ld)
    assert torch.equal(p_h.cpu(), p_e)
    # unfold + GEMM == the strided convolution it replaces
    w = rnd((32, 3, P, P), torch.float32, 6)
    ref = torch.nn.functional.conv2d(img, w, stride=P).permute(0, 2, 3, 1).reshape(-1, 32)
    assert torch.allclose(p_e.float()[:, :588] @ w.reshape(32, -1).t(), ref, atol=2e-1 if dt == "bf16" else 1e-4)
    with pytest.raises(Exception, match="patch size"):
        hip.patchify(img.cuda(), p_h, B=B, Cin=3, H=28, W=42, P=16, ld=1024)


@pytest.mark.parametrize("dt", ["bf16", "f32", "f16"])
def test_weight_packers_match_the_host_packers(hip, dt):
    """fyc_pack_conv3x3 / fyc_pack_geglu (the layouts fyc_gemm expects, for hosts without torch) == engine/weights.py, bit for bit"""
    from followyourclick_amd.engine import weights as Wt
    T = DT[dt]
    for O, I in ((32, 4), (64, 320), (16, 100)):                     # I = 4: the latent conv_in; 100: padding inside a slab
        w = rnd((O, I, 3, 3), torch.float32, O + I)
        ref = Wt.pack_conv3x3(w, T, "cpu")
        out = torch.full(ref.shape, float("nan"), dtype=T, device="cuda")
        hip.pack_conv3x3(w.cuda(), out)
        assert torch.equal(out.cpu(), ref), (O, I)
    for O, I in ((64, 40), (2560, 320)):
        w, b = rnd((O, I), torch.float32, 7), rnd((O,), torch.float32, 8)
        rw, rb = Wt.pack_geglu(w, b, T, "cpu")
        ow, ob = torch.empty(O, I, dtype=T, device="cuda"), torch.empty(O, device="cuda")
        hip.pack_geglu(w.cuda(), b.cuda(), ow, ob)
        assert torch.equal(ow.cpu(), rw) and torch.equal(ob.cpu(), rb), (O, I)
    with pytest.raises(Exception, match="multiple of 32"):
        hip.pack_geglu(torch.zeros(48, 8, device="cuda"), None, torch.empty(48, 8, dtype=T, device="cuda"), None)


# ---- LayerNorm folded into the consuming GEMM ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f32", "f16"])
@pytest.mark.parametrize("rows,C", [(300, 320), (64, 64), (1000, 1280), (33, 640)])
def test_row_stats(hip, emu, dt, rows, C):
    T = DT[dt]
    x = (rnd((rows, C), torch.float32, 3) * 2 + 0.7).to(T)
    st_h = torch.full((rows, 2), float("nan"), device="cuda")
    hip.row_stats(x.cuda(), st_h, rows=rows, C_=C, eps=1e-5)
    st_e = torch.zeros(rows, 2)
    emu.row_stats(x, st_e, rows=rows, C_=C, eps=1e-5)
    close(st_h, st_e, f"row_stats {dt} {rows}x{C}", 2e-5)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("epi", ["linear", "linear_narrow", "geglu", "heads"])
@pytest.mark.parametrize("M,C", [(300, 320), (4096, 640), (77, 64)])
def test_gemm_layernorm_fold(hip, emu, dt, epi, M, C):
    """rstd*(x W'^T - mean*colsum) + bias in every epilogue == LayerNorm(x) followed by the plain GEMM (checked against the op spec,
    and the spec against torch's layer_norm)"""
    T = DT[dt]
    N = {"linear": 3 * C, "linear_narrow": C + 4, "geglu": 8 * C, "heads": 3 * C}[epi]
    x = (rnd((M, C), torch.float32, 1) * 1.5 + 0.3).to(T)
    gamma, beta = 1 + 0.2 * rnd((C,), torch.float32, 2), 0.1 * rnd((C,), torch.float32, 3)
    w, b = rnd((N, C), torch.float32, 4, 1 / math.sqrt(C)), rnd((N,), torch.float32, 5)
    wf = (w * gamma[None, :]).to(T)
    bias = w @ beta + b
    cs = wf.float().sum(dim=1)
    st = torch.zeros(M, 2)
    emu.row_stats(x, st, rows=M, C_=C)
    kw = dict(M=M, N=N, K=C, lda=C, ldw=C, bias=bias)
    if epi in ("linear", "linear_narrow"):
        kw.update(ldo=N)
        o_h, o_e = torch.full((M, N), float("nan"), dtype=T, device="cuda"), torch.zeros(M, N, dtype=T)
    elif epi == "geglu":
        kw.update(ldo=N // 2, epilogue=1)
        o_h, o_e = torch.full((M, N // 2), float("nan"), dtype=T, device="cuda"), torch.zeros(M, N // 2, dtype=T)
    else:
        heads, tokens = 8, M
        d, ld = C // heads, (M + 7) // 8 * 8
        mk = lambda dev: [torch.zeros(1, heads, tokens, d, dtype=T, device=dev), torch.zeros(1, heads, tokens, d, dtype=T, device=dev),
                          torch.zeros(1, heads, d, ld, dtype=T, device=dev)]
        oh, oe = mk("cuda"), mk("cpu")
        kw.update(epilogue=2)
    cu = lambda t: t.cuda()
    if epi == "heads":
        hd = lambda outs: dict(seg_cols=C, heads=8, tokens=M, outs=outs, transposed=[0, 0, 1], ld=[0, 0, ld])
        hip.gemm(cu(x), cu(wf), None, **dict(kw, bias=cu(bias)), heads=hd(oh), ln_stats=cu(st), ln_colsum=cu(cs))
        emu.gemm(x, wf, None, **kw, heads=hd(oe), ln_stats=st, ln_colsum=cs)
        for i in range(3):
            close(oh[i], oe[i], f"ln-fold heads {dt} seg {i}", RTOL[dt])
        ref = torch.nn.functional.layer_norm(x.float(), (C,), gamma, beta) @ w.t() + b            # what the fold stands for
        got = oe[0].float().permute(0, 2, 1, 3).reshape(M, C)
        assert ((got - ref[:, :C]).norm() / ref[:, :C].norm()).item() < (2e-2 if dt == "bf16" else 1e-5)
        return
    hip.gemm(cu(x), cu(wf), o_h, **dict(kw, bias=cu(bias)), ln_stats=cu(st), ln_colsum=cu(cs))
    emu.gemm(x, wf, o_e, **kw, ln_stats=st, ln_colsum=cs)
    close(o_h, o_e, f"ln-fold {epi} {dt} {M}x{N}x{C}", RTOL[dt])
    if epi != "geglu":
        ref = torch.nn.functional.layer_norm(x.float(), (C,), gamma, beta) @ w.t() + b
        assert ((o_e.float() - ref).norm() / ref.norm()).item() < (2e-2 if dt == "bf16" else 1e-5)
    with pytest.raises(Exception, match="come together"):
        hip.gemm(cu(x), cu(wf), o_h, **dict(kw, bias=cu(bias)), ln_stats=cu(st))


@pytest.mark.parametrize("dt", ["bf16", "f32", "f16"])
def test_ddim_three_way_guidance(hip, emu, dt):
    """single + video_scale*(uncond - single) + guidance*(cond - uncond) (reference pipeline_animation.py:754-760)"""
    T = DT[dt]
    B, F, HW, CL, ld = 2, 3, 20, 4, 8
    pred, single = rnd((2 * B * F * HW, ld), T, 1), rnd((B * F * HW, ld), T, 2)
    lat = rnd((B, CL, F, HW), torch.float32, 3)
    coef = torch.tensor([0.8, 0.6, 0.9, 0.43589])
    kw = dict(B=B, F=F, HW=HW, c_latent=CL, ld=ld, cfg=True, guidance=7.5, pred_type=0, clip_sample=False, video_scale=0.7)
    l_h = lat.clone().cuda()
    hip.cfg_ddim_step(pred.cuda(), l_h, coef.cuda(), pred_single=single.cuda(), **kw)
    l_e = lat.clone()
    emu.cfg_ddim_step(pred, l_e, coef, pred_single=single, **kw)
    close(l_h, l_e, f"three-way guidance {dt}", 1e-5)
    with pytest.raises(Exception, match="needs classifier-free"):
        hip.cfg_ddim_step(pred.cuda(), l_h, coef.cuda(), pred_single=single.cuda(), **dict(kw, cfg=False))


# ---- statistics fused into the producing epilogue (fyc_gemm chan_stats / row_parts, fyc_gn_apply_cs) --------------------------
STAT_TILES = [0, 1, 2, 3, 4, 5, 6, 7, 11]


@pytest.mark.parametrize("dt,tile", [("bf16", t) for t in STAT_TILES] + [("f32", 0)] + [("f16", t) for t in (0, 5, 6)])
@pytest.mark.parametrize("M,N,K,cs_rows,res", [(512, 320, 320, 64, True), (768, 640, 128, 128, True), (1152, 128, 64, 192, False),
                                               (4096, 320, 64, 4096, True), (1280, 328, 72, 640, False), (1040, 64, 64, 80, False),
                                               (1152, 320, 64, 144, True), (2304, 640, 128, 576, True)])     # 12x12 / 24x24 frames (768^2): samples straddle wave rows
def test_gemm_output_statistics(hip, emu, dt, tile, M, N, K, cs_rows, res):
    """per-(row tile, sample, channel) and per-row {sum, sum of squares} written by the LINEAR epilogue, folded by
    fyc_chan_stats_reduce == sums of the values it stored (partial row / column tiles, up to 4 samples per tile, samples
    straddling tiles); the column sums are bitwise repeatable (ordered reduction, no atomics)"""
    T = DT[dt]
    a, w = rnd((M, K), T, 1), rnd((N, K), T, 2, 1 / math.sqrt(K))
    bias, r = rnd((N,), torch.float32, 3), (rnd((M, N), T, 4) if res else None)
    hip.set_tuning(1, tile)
    again = []
    try:
        nparts = hip.gemm_row_parts(T, M=M, N=N, K=K)
        nt, tile_rows, slots = hip.gemm_stat_layout(T, M=M, N=N, K=K, cs_rows=cs_rows)
        if slots > 4:
            pytest.skip("more than 4 samples per row tile: the engine falls back to the separate statistics pass")
        o_h = torch.full((M, N), float("nan"), dtype=T, device="cuda")
        parts = torch.full((nt * slots * N * 2,), float("nan"), dtype=torch.float32, device="cuda")
        rp = torch.full((M, nparts, 2), float("nan"), dtype=torch.float32, device="cuda")
        hip.gemm(a.cuda(), w.cuda(), o_h, M=M, N=N, K=K, lda=K, ldw=K, ldo=N, ldr=N, bias=bias.cuda(), residual=None if r is None else r.cuda(),
                 out_scale=1.25, chan_parts=parts, cs_rows=cs_rows, row_parts=rp, row_nparts=nparts)
        cs = torch.full((M // cs_rows, N, 2), float("nan"), dtype=torch.float64, device="cuda")
        hip.chan_stats_reduce(parts, cs, rows=M, N=N, cs_rows=cs_rows, tile_rows=tile_rows, slots=slots)
        for _ in range(3):
            p2 = torch.full_like(parts, float("nan"))
            hip.gemm(a.cuda(), w.cuda(), torch.empty_like(o_h), M=M, N=N, K=K, lda=K, ldw=K, ldo=N, ldr=N, bias=bias.cuda(), residual=None if r is None else r.cuda(),
                     out_scale=1.25, chan_parts=p2, cs_rows=cs_rows)
            again.append(p2)
        torch.cuda.synchronize()
    finally:
        hip.set_tuning(1, 0)
    for p2 in again:
        assert torch.equal(torch.nan_to_num(p2, nan=-1.0), torch.nan_to_num(parts, nan=-1.0)), f"column sums differ between launches ({dt}, tile {tile})"
    o_e = torch.zeros(M, N, dtype=T)
    emu.gemm(a, w, o_e, M=M, N=N, K=K, lda=K, ldw=K, ldo=N, ldr=N, bias=bias, residual=r, out_scale=1.25)
    close(o_h, o_e, f"gemm+stats {dt} tile {tile}", RTOL[dt])
    v = o_h.cpu().double()
    vs = v.reshape(M // cs_rows, cs_rows, N)
    close(cs, torch.stack([vs.sum(dim=1), (vs * vs).sum(dim=1)], dim=-1), f"chan stats {dt} tile {tile} ({tile_rows}-row tiles, {slots} slots)", 2e-6)
    rows = rp.cpu().double().sum(dim=1)
    close(rows, torch.stack([v.sum(dim=1), (v * v).sum(dim=1)], dim=-1), f"row_parts {dt} tile {tile} ({nparts} parts)", 2e-6)


@pytest.mark.parametrize("dt", ["bf16", "f32", "f16"])
def test_conv_output_statistics(hip, emu, dt):
    T = DT[dt]
    frames, H, W, Cin, Cout = 4, 16, 16, 64, 320
    M, K = frames * H * W, 9 * Cin
    x, w, bias = rnd((M, Cin), T, 1), rnd((Cout, K), T, 2, 1 / math.sqrt(K)), rnd((Cout,), torch.float32, 3)
    res = rnd((M, Cout), T, 4)
    conv = dict(Hout=H, Wout=W, Hin=H, Win=W, Cin=Cin, stride=1)
    for cs_rows in (H * W, 2 * H * W):
        nt, tile_rows, slots = hip.gemm_stat_layout(T, M=M, N=Cout, K=K, cs_rows=cs_rows, mode=1)
        parts = torch.full((nt * slots * Cout * 2,), float("nan"), dtype=torch.float32, device="cuda")
        o_h = torch.empty(M, Cout, dtype=T, device="cuda")
        hip.gemm(x.cuda(), w.cuda(), o_h, M=M, N=Cout, K=K, lda=Cin, ldw=K, ldo=Cout, ldr=Cout, bias=bias.cuda(), residual=res.cuda(),
                 mode=1, conv=conv, chan_parts=parts, cs_rows=cs_rows)
        cs = torch.empty(M // cs_rows, Cout, 2, dtype=torch.float64, device="cuda")
        hip.chan_stats_reduce(parts, cs, rows=M, N=Cout, cs_rows=cs_rows, tile_rows=tile_rows, slots=slots)
        torch.cuda.synchronize()
        vs = o_h.cpu().double().reshape(M // cs_rows, cs_rows, Cout)
        close(cs, torch.stack([vs.sum(dim=1), (vs * vs).sum(dim=1)], dim=-1), f"conv chan stats {dt} rows/sample {cs_rows}", 2e-6)
    with pytest.raises(Exception, match="cs_rows"):
        hip.gemm(x.cuda(), w.cuda(), o_h, M=M, N=Cout, K=K, lda=Cin, ldw=K, ldo=Cout, mode=1, conv=conv, chan_parts=parts, cs_rows=40)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("M,C", [(384, 320), (200, 640), (512, 1280)])
def test_layernorm_fold_from_producer_row_parts(hip, emu, dt, M, C):
    """producer GEMM writes row partial sums -> consumer GEMM derives mean / rstd from them == LayerNorm + GEMM"""
    T = DT[dt]
    a, wp = rnd((M, C), T, 1), rnd((C, C), T, 2, 1 / math.sqrt(C))
    bp = 0.5 + rnd((C,), torch.float32, 9)           # a non-zero mean: the variance comes from E[x^2] - mean^2
    gamma, beta = 1 + 0.2 * rnd((C,), torch.float32, 3), 0.1 * rnd((C,), torch.float32, 4)
    w = rnd((2 * C, C), torch.float32, 5, 1 / math.sqrt(C))
    wf = (w * gamma[None, :]).to(T)
    bias, cs = w @ beta, wf.float().sum(dim=1)
    n = hip.gemm_row_parts(T, M=M, N=C, K=C)
    tok = torch.empty(M, C, dtype=T, device="cuda")
    rp = torch.empty(M, n, 2, dtype=torch.float32, device="cuda")
    hip.gemm(a.cuda(), wp.cuda(), tok, M=M, N=C, K=C, lda=C, ldw=C, ldo=C, bias=bp.cuda(), row_parts=rp, row_nparts=n)
    o_h = torch.empty(M, 2 * C, dtype=T, device="cuda")
    hip.gemm(tok, wf.cuda(), o_h, M=M, N=2 * C, K=C, lda=C, ldw=C, ldo=2 * C, bias=bias.cuda(), ln_stats=rp, ln_nparts=n, ln_eps=1e-5,
             ln_colsum=cs.cuda())
    torch.cuda.synchronize()
    ref = torch.nn.functional.layer_norm(tok.cpu().double(), (C,), gamma.double(), beta.double()) @ w.double().t()
    err = ((o_h.cpu().double() - ref).norm() / ref.norm()).item()
    assert err < (1.2e-2 if dt == "bf16" else 2e-5), err


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("samples,rps,C1,C2,silu,nf", [(2, 256, 320, 0, True, 1), (3, 64, 64, 64, False, 1), (2, 640, 1280, 640, True, 5),
                                                       (1, 4096, 320, 320, True, 16), (4, 128, 2560 - 1280, 1280, True, 2)])
def test_groupnorm_apply_from_channel_sums(hip, emu, dt, samples, rps, C1, C2, silu, nf):
    """fyc_gn_apply_cs: GroupNorm (+SiLU) from per-(sample, channel) sums, channel concat of two sources with groups that
    straddle them (1280 + 640 channels: 60 channels per group)"""
    T = DT[dt]
    rows, Cc = samples * rps, C1 + C2
    x1 = (rnd((rows, C1), torch.float32, 1) * 1.3 + 0.4).to(T)
    x2 = (rnd((rows, C2), torch.float32, 2) * 0.7 - 0.2).to(T) if C2 else None
    gamma, beta = 1 + 0.2 * rnd((Cc,), torch.float32, 3), 0.1 * rnd((Cc,), torch.float32, 4)

    def sums(x):          # per statistics sample (frame): nf of them make up one GroupNorm sample
        v = x.double().reshape(samples * nf, rps // nf, -1)
        return torch.stack([v.sum(dim=1), (v * v).sum(dim=1)], dim=-1).contiguous()
    cs1, cs2 = sums(x1), (sums(x2) if C2 else None)
    y_h = torch.full((rows, Cc), float("nan"), dtype=T, device="cuda")
    kw = dict(rows=rows, C1=C1, groups=32, rows_per_sample=rps, eps=1e-5, silu=silu, cs_rows=rps // nf)
    hip.gn_apply_cs(x1.cuda(), cs1.cuda(), gamma.cuda(), beta.cuda(), y_h, x2=None if x2 is None else x2.cuda(),
                    cs2=None if cs2 is None else cs2.cuda(), C2=C2, **kw)
    torch.cuda.synchronize()
    y_e = torch.zeros(rows, Cc, dtype=T)
    emu.gn_apply_cs(x1, cs1, gamma, beta, y_e, x2=x2, cs2=cs2, C2=C2, **kw)
    close(y_h, y_e, f"gn_apply_cs {dt} {samples}x{rps}x({C1}+{C2})", RTOL[dt])
    ref = torch.nn.functional.group_norm(torch.cat([x1] + ([x2] if C2 else []), dim=1).float().reshape(samples, rps, Cc).permute(0, 2, 1), 32,
                                         gamma, beta, 1e-5).permute(0, 2, 1).reshape(rows, Cc)
    ref = torch.nn.functional.silu(ref) if silu else ref
    assert ((y_e.float() - ref).norm() / ref.norm()).item() < (5e-3 if dt == "bf16" else 1e-5)


@pytest.mark.parametrize("kind,M,N,K,res", [("gemm", 2048, 1280, 6400, True), ("gemm", 1000, 640, 2560, False), ("conv", 2048, 1280, 11520, True),
                                            ("conv", 512, 320, 5760, False), ("gemm", 4096, 256, 2048, True)])
def test_gemm_split_k(hip, emu, kind, M, N, K, res):
    """small M + long K: K slices per output tile with f32 partials in the caller's workspace == the unsplit result"""
    T = torch.bfloat16
    w, bias = rnd((N, K), T, 2, 1 / math.sqrt(K)), rnd((N,), torch.float32, 3)
    r = rnd((M, N), T, 4) if res else None
    if kind == "conv":
        Cin, side = K // 9, 8
        frames = M // (side * side)
        a = rnd((M, Cin), T, 1)
        kw = dict(M=M, N=N, K=K, lda=Cin, ldw=K, ldo=N, ldr=N, mode=1, conv=dict(Hout=side, Wout=side, Hin=side, Win=side, Cin=Cin, stride=1))
    else:
        a = rnd((M, K), T, 1)
        kw = dict(M=M, N=N, K=K, lda=K, ldw=K, ldo=N, ldr=N)
    assert hip.gemm_split_bytes(T, M=M, N=N, K=K, mode=kw.get("mode", 0)) > 0
    rowb = rnd(((M + 63) // 64, N), torch.float32, 5)
    o_h = torch.full((M, N), float("nan"), dtype=T, device="cuda")
    hip.gemm(a.cuda(), w.cuda(), o_h, bias=bias.cuda(), rowbias=rowb.cuda(), rows_per_batch=64, residual=None if r is None else r.cuda(), out_scale=0.5, **kw)
    torch.cuda.synchronize()
    o_e = torch.zeros(M, N, dtype=T)
    emu.gemm(a, w, o_e, bias=bias, rowbias=rowb, rows_per_batch=64, residual=r, out_scale=0.5, **kw)
    close(o_h, o_e, f"split-K {kind} {M}x{N}x{K}", RTOL["bf16"])
    hip.set_tuning(0, 1)          # key 0 = 1: split-K off -> same numbers from the plain path
    try:
        o_p = torch.full((M, N), float("nan"), dtype=T, device="cuda")
        hip.gemm(a.cuda(), w.cuda(), o_p, bias=bias.cuda(), rowbias=rowb.cuda(), rows_per_batch=64, residual=None if r is None else r.cuda(), out_scale=0.5, **kw)
        torch.cuda.synchronize()
    finally:
        hip.set_tuning(0, 0)
    close(o_p, o_e, f"unsplit {kind} {M}x{N}x{K}", RTOL["bf16"])


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("kind,M,N,K,cs_rows,res", [("conv", 2048, 1280, 11520, 64, True), ("conv", 2048, 1280, 23040, 64, False), ("gemm", 2048, 1280, 6400, 64, True),
                                                    ("gemm", 1008, 640, 2560, 48, False), ("conv", 512, 320, 5760, 64, False), ("gemm", 512, 5120, 2560, 64, False)])
def test_gemm_split_k_output_statistics(hip, emu, dt, kind, M, N, K, cs_rows, res):
    """round 6: the split-K finish kernel writes the per-(128-row tile, sample slot, channel) sums of the values it stores - the 8x8-level
    convolutions no longer send their consumers to the separate statistics pass - in the layout fyc_gemm_stat_layout announces; bitwise
    repeatable (ordered adds, no atomics), incl. samples that straddle tiles (48-row samples) and a ragged last tile.  512x5120x2560 is the
    smallest shape whose unsplit tile (256 rows) is higher than the split one: a layout announced for the wrong one of the two shows here"""
    T = DT[dt]
    w, bias = rnd((N, K), T, 2, 1 / math.sqrt(K)), rnd((N,), torch.float32, 3)
    r = rnd((M, N), T, 4) if res else None
    if kind == "conv":
        Cin, side = K // 9, 8
        a = rnd((M, Cin), T, 1)
        kw = dict(M=M, N=N, K=K, lda=Cin, ldw=K, ldo=N, ldr=N, mode=1, conv=dict(Hout=side, Wout=side, Hin=side, Win=side, Cin=Cin, stride=1))
    else:
        a = rnd((M, K), T, 1)
        kw = dict(M=M, N=N, K=K, lda=K, ldw=K, ldo=N, ldr=N)
    assert hip.gemm_split_bytes(T, M=M, N=N, K=K, mode=kw.get("mode", 0)) > 0, "this shape is expected to take the split-K path"
    nt, tile_rows, slots = hip.gemm_stat_layout(T, M=M, N=N, K=K, cs_rows=cs_rows, mode=kw.get("mode", 0))
    assert tile_rows == 128 and nt == (M + 127) // 128 and 1 <= slots <= 4, (nt, tile_rows, slots)
    outs, parts_all = [], []
    for it in range(3):
        parts = torch.full((nt * slots * N * 2,), float("nan"), device="cuda")
        o_h = torch.full((M, N), float("nan"), dtype=T, device="cuda")
        hip.gemm(a.cuda(), w.cuda(), o_h, bias=bias.cuda(), residual=None if r is None else r.cuda(), chan_parts=parts, cs_rows=cs_rows, **kw)
        torch.cuda.synchronize()
        outs.append(o_h.cpu())
        parts_all.append(parts.cpu())
    assert torch.equal(parts_all[0], parts_all[1]) and torch.equal(parts_all[0], parts_all[2]), "column sums differ between launches"
    o_e = torch.zeros(M, N, dtype=T)
    emu.gemm(a, w, o_e, bias=bias, residual=r, **kw)
    close(outs[0], o_e, f"split-K + stats {dt} {kind} {M}x{N}x{K}", RTOL[dt] if dt == "bf16" else 6e-4)
    cs = torch.zeros(M // cs_rows, N, 2, dtype=torch.float64, device="cuda")
    hip.chan_stats_reduce(parts_all[0].cuda(), cs, rows=M, N=N, cs_rows=cs_rows, tile_rows=tile_rows, slots=slots)
    torch.cuda.synchronize()
    v = outs[0].double().reshape(M // cs_rows, cs_rows, N)
    close(cs, torch.stack([v.sum(dim=1), (v * v).sum(dim=1)], dim=-1), f"split-K chan stats {dt} {kind} ({slots} slots)", 2e-6)
