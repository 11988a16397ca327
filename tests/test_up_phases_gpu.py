"""fyc_conv_up_phases on the GPU through the C ABI: judged per element by tests/kernel_compare.py::compare against the f64 specification of
tests/up_phases_spec.py (same packed, storage-rounded phase weights; K = 4 Cin; C_ACC = 1, no new constant), NaN guard bands round the input and
the output, output statistics folded per clip and per frame against exact integer sums, refusals that launch nothing.

FYC_UP_PHASES_FIGURES=<file>: append the figures of every comparison, with the executed tile, to that file."""
import ctypes
import functools
import math
import os

import pytest
import torch

import up_phases_spec as U
from kernel_compare import BoundTerms, Guard, compare

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
GUARD_ROWS = 19          # NaN rows in front of and behind the output; the input's guard is a frame row + 1 pixels either side

# name: (frames, Hin, Win, Cin real, Cout, frames per group).  a: one tile per phase, all four borders; b: three channel slabs, non-square, group = frame
# of a two-clip batch; c: channel padding (72 -> 128, the pad channels carry finite junk against zero weights) and an N edge tile (328 = 5 x 64 + 8);
# d: G = 256 with M = 16384, where the planner's 256-row tile runs; e / f: the 320-wide tiles of the UNet's own launches (128 x 320 at M = 8192, 256 x 320 at 16384)
CASES = {"a": (2, 8, 8, 64, 64, 2), "b": (4, 16, 8, 192, 320, 1), "c": (2, 8, 16, 72, 328, 1), "d": (16, 16, 16, 64, 128, 1),
         "e": (8, 16, 16, 64, 320, 1), "f": (16, 16, 16, 64, 320, 2)}


@pytest.fixture(scope="module")
def hip():
    from followyourclick_amd import ops
    h = ops.get()
    h.ensure_init(torch.device("cuda:0"))
    assert h.name == "hip"
    return h


@functools.lru_cache(maxsize=None)
def _problem(name, dt):
    """operands, the f64 reference rounded to the storage type and the bound's S: once per (case, dtype)"""
    from followyourclick_amd.engine.weights import pack_conv_up_phases, pad_channels
    frames, Hin, Win, Cin, Cout, fpg = CASES[name]
    T, g = DT[dt], torch.Generator().manual_seed(sum(map(ord, name + dt)))
    Cp = pad_channels(Cin)
    x = torch.randn(frames, Hin, Win, Cp, generator=g).to(T)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    bias = torch.randn(Cout, generator=g)
    w_ph = pack_conv_up_phases(w, T, "cpu")
    w4 = U.unpack(w_ph)
    ref = U.phase_conv(x.double(), w4, bias).reshape(-1, Cout).to(T)
    S = U.phase_conv(x.double().abs(), w4.abs(), bias.abs()).reshape(-1, Cout)
    return x, w_ph, bias, ref, S


def _guarded_input(x):
    frames, Hin, Win, Cp = x.shape
    gr = Win + 1
    buf = torch.full((gr + frames * Hin * Win + gr, Cp), float("nan"), dtype=x.dtype, device="cuda")
    buf[gr:-gr] = x.reshape(-1, Cp).cuda()
    return buf, buf[gr:-gr]


def _record(fig, **extra):
    path = os.environ.get("FYC_UP_PHASES_FIGURES")
    line = " ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in {**fig, **extra}.items())
    print(line)
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_matches_the_f64_specification(hip, name, dt):
    frames, Hin, Win, Cin, Cout, fpg = CASES[name]
    T = DT[dt]
    x, w_ph, bias, ref, S = _problem(name, dt)
    Cp, G, M = x.shape[-1], fpg * Hin * Win, 4 * frames * Hin * Win
    assert hip.conv_up_phases_supported(T, Cin=Cp, Cout=Cout, Hin=Hin, Win=Win, group_rows=G)
    nt, tile_rows, slots = hip.conv_up_phases_stat_layout(T, frames=frames, Hin=Hin, Win=Win, Cin=Cp, Cout=Cout, group_rows=G)
    assert slots == 1 and nt * tile_rows == M and G % tile_rows == 0
    if name in "df":
        assert tile_rows == 256, "cases d and f exist for the 256-row tiles"
    keep, a = _guarded_input(x)
    ldo = Cout + 8                                    # 8 pad columns per row: they must stay NaN as well
    obuf = torch.full((GUARD_ROWS + M + GUARD_ROWS, ldo), float("nan"), dtype=T, device="cuda")
    before = obuf.cpu().clone()
    out = obuf[GUARD_ROWS:GUARD_ROWS + M]
    parts = torch.full((nt * Cout * 2,), float("nan"), dtype=torch.float32, device="cuda")
    wa, ba = w_ph.cuda(), bias.cuda()
    hip.conv_up_phases(a, wa, out, frames=frames, Hin=Hin, Win=Win, Cin=Cp, Cout=Cout, group_rows=G, bias=ba, ldo=ldo, chan_parts=parts)
    torch.cuda.synchronize()
    after = obuf.cpu()
    mask = torch.zeros(obuf.shape, dtype=torch.bool)
    mask[GUARD_ROWS:GUARD_ROWS + M, :Cout] = True
    fig = compare(after[GUARD_ROWS:GUARD_ROWS + M, :Cout], ref, dtype=dt, bound_terms=BoundTerms(S, 4 * Cp, (tile_rows, 64)),
                  guard=Guard(before, after, mask), tag=f"up_phases {name} {dt}")
    _record(fig, case=name, tile_rows=tile_rows, row_tiles=nt, G=G, M=M, N=Cout, K=4 * Cp)
    gr = Win + 1
    assert torch.isnan(keep[:gr].float()).all() and torch.isnan(keep[-gr:].float()).all()
    assert torch.isfinite(parts).all()                # every (row tile, channel) partial was written


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_output_statistics_fold_per_clip_and_per_frame(hip, dt):
    """integer-valued operands whose outputs (|.| <= 39) and partial sums are exact in every format: the stored output must equal the f64 reference bit for
    bit, and chan_parts folded by fyc_chan_stats_reduce over the virtual rows (cs_rows = G, out_rows = 4 G) must BE the f64 column sums of the group's
    output rows, for the group = clip (2 frames, G = 256) and the group = frame (G = 128)"""
    from followyourclick_amd.engine.weights import pack_conv_up_phases
    T, g = DT[dt], torch.Generator().manual_seed(7)
    frames, Hin, Win, Cin, Cout = 4, 16, 8, 64, 72
    x = torch.randint(-1, 2, (frames, Hin, Win, Cin), generator=g).to(T)
    w = torch.zeros(Cout, Cin, 3, 3)
    w[:, :4] = torch.randint(-1, 2, (Cout, 4, 3, 3), generator=g).float()      # four live input channels: |out| <= 4 * 9 + 3
    bias = torch.randint(-3, 4, (Cout,), generator=g).float()
    w_ph = pack_conv_up_phases(w, T, "cpu")
    ref = U.phase_conv(x.double(), U.unpack(w_ph), bias).reshape(-1, Cout)
    assert ref.abs().max() <= 39 and torch.equal(ref, ref.round())
    M = ref.shape[0]
    xa, wa = x.reshape(-1, Cin).cuda(), w_ph.cuda()
    for fpg in (2, 1):
        G = fpg * Hin * Win
        nt, tile_rows, slots = hip.conv_up_phases_stat_layout(T, frames=frames, Hin=Hin, Win=Win, Cin=Cin, Cout=Cout, group_rows=G)
        assert slots == 1 and nt * tile_rows == M
        parts = torch.full((nt * Cout * 2,), float("nan"), dtype=torch.float32, device="cuda")
        out = torch.full((M, Cout), float("nan"), dtype=T, device="cuda")
        hip.conv_up_phases(xa, wa, out, frames=frames, Hin=Hin, Win=Win, Cin=Cin, Cout=Cout, group_rows=G, bias=bias.cuda(),
                           chan_parts=parts)
        cs = torch.full((M // (4 * G), Cout, 2), float("nan"), dtype=torch.float64, device="cuda")
        hip.chan_stats_reduce(parts, cs, rows=M, N=Cout, cs_rows=G, tile_rows=tile_rows, slots=slots, out_rows=4 * G)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu().double(), ref), f"group of {fpg} frames: the stored output differs from the exact one"
        v = ref.reshape(M // (4 * G), 4 * G, Cout)
        assert torch.equal(cs.cpu(), torch.stack([v.sum(dim=1), (v * v).sum(dim=1)], dim=-1)), f"group of {fpg} frames"


def test_refused_calls_return_an_error_and_launch_nothing(hip):
    """G = 64 (8 x 8 frames as groups), a residual, f32: an error code with a message, the output untouched"""
    from followyourclick_amd import _lib as L
    T = torch.bfloat16
    frames, Hin, Win, C = 2, 8, 8, 64
    M = 4 * frames * Hin * Win
    x, w_ph = torch.zeros(frames * Hin * Win, C, dtype=T, device="cuda"), torch.zeros(4, C, 4 * C, dtype=T, device="cuda")
    out = torch.full((M, C), float("nan"), dtype=T, device="cuda")
    assert not hip.conv_up_phases_supported(T, Cin=C, Cout=C, Hin=Hin, Win=Win, group_rows=64)
    with pytest.raises(L.FycError, match="group_rows=64"):
        hip.conv_up_phases(x, w_ph, out, frames=frames, Hin=Hin, Win=Win, Cin=C, Cout=C, group_rows=64)
    u = hip._conv_up_phases_args(L.FYC_BF16, frames, Hin, Win, C, C, 4 * C, C, 128)
    u.gemm.a, u.gemm.w, u.gemm.out, u.gemm.residual = x.data_ptr(), w_ph.data_ptr(), out.data_ptr(), out.data_ptr()
    assert hip.lib.fyc_conv_up_phases(ctypes.byref(u), hip._stream()) != 0 and b"residual" in hip.lib.fyc_last_error()
    assert not hip.conv_up_phases_supported(torch.float32, Cin=C, Cout=C, Hin=Hin, Win=Win, group_rows=128)
    o32 = torch.full((M, C), float("nan"), dtype=torch.float32, device="cuda")
    with pytest.raises(L.FycError, match="16-bit"):
        hip.conv_up_phases(x.float(), w_ph.float(), o32, frames=frames, Hin=Hin, Win=Win, Cin=C, Cout=C, group_rows=128)
    torch.cuda.synchronize()
    assert torch.isnan(out.float()).all() and torch.isnan(o32).all()
