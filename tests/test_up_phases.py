"""The four-phase form of nearest-2x upsampling + 3x3 convolution, without a GPU: the weight pack, the equivalence in f64, the virtual-row map,
the fallback of op objects that lack the op, and the header / binding tables."""
import hashlib
import os
import re

import pytest
import torch
import torch.nn.functional as F

import trace_ops
import up_phases_spec as U
from kernel_compare import ulp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "up_phases_parent_schedule.txt")


def _w(O=5, I=7, seed=0):
    return torch.randn(O, I, 3, 3, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("dt,T", [("bf16", torch.bfloat16), ("f16", torch.float16)])
def test_packed_weights_are_the_f64_sums_rounded_once(dt, T):
    """every pre-summed weight = the f64 sum of its 3x3 terms to within one rounding of the storage type (half a unit) plus three f32 additions"""
    from followyourclick_amd.engine.weights import pack_conv_up_phases, up_phase_weights
    w = _w(O=6, I=70, seed=1)
    packed = pack_conv_up_phases(w, T, "cpu")
    assert packed.shape == (4, 6, 4 * 128) and packed.dtype == T
    got = U.unpack(packed)
    exact, mag = up_phase_weights(w.double()), up_phase_weights(w.double().abs())
    assert torch.equal(got[:, :, 70:], torch.zeros_like(got[:, :, 70:]))      # padded channels
    e32 = 3 * 2.0 ** -24 * mag
    bound = 0.5 * ulp(exact.abs() + e32, dt) + e32
    assert ((got[:, :, :70] - exact).abs() <= bound).all()
    # a corner weight of phase (0, 0) is W[0][0] alone, its opposite corner the sum of four
    assert torch.equal(exact[0, :, :, 0, 0], w.double()[:, :, 0, 0])
    assert torch.allclose(exact[0, :, :, 1, 1], w.double()[:, :, 1:, 1:].sum(dim=(2, 3)), rtol=0, atol=1e-14)


def test_phase_form_equals_upsample_then_conv_in_f64():
    """non-square 5 x 7 input: an x / y swap, a wrong phase or a wrong border shows"""
    from followyourclick_amd.engine.weights import up_phase_weights
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, 5, 7, 4, generator=g, dtype=torch.float64)
    w, b = torch.randn(6, 4, 3, 3, generator=g, dtype=torch.float64), torch.randn(6, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest"), w, b, padding=1).permute(0, 2, 3, 1)
    got = U.phase_conv(x, up_phase_weights(w), b)
    assert got.shape == ref.shape == (3, 10, 14, 6)
    assert (got - ref).abs().max().item() < 1e-12


@pytest.mark.parametrize("group", ["clip", "frame"])
def test_virtual_rows_map_onto_the_output_rows_one_to_one(group):
    frames, F_, Hin, Win = 4, 2, 3, 5
    G = (F_ if group == "clip" else 1) * Hin * Win
    M = 4 * frames * Hin * Win
    rows = [U.output_row(m, G, Hin, Win) for m in range(M)]
    assert rows == [U.output_row_by_definition(m, G, Hin, Win) for m in range(M)]
    assert sorted(rows) == list(range(M))
    # the 4 G virtual rows of a group are the output rows of that group's frames, nothing else
    for grp in range(M // (4 * G)):
        assert sorted(rows[grp * 4 * G:(grp + 1) * 4 * G]) == list(range(grp * 4 * G, (grp + 1) * 4 * G))


def _digests():
    out = {}
    for case in trace_ops.unet_cases():
        out["unet " + case[0]] = hashlib.sha256("\n".join(trace_ops.run_unet(case).lines()).encode()).hexdigest()
    for case in trace_ops.vae_cases():
        if case[1] == "decode":
            out["vae " + case[0]] = hashlib.sha256("\n".join(trace_ops.run_vae(case).lines()).encode()).hexdigest()
    return out


def test_op_objects_without_the_op_get_the_parents_launch_sequence():
    """The recording backend and the CPU emulator have no conv_up_phases: every forward of the trace matrix must be, launch for launch and buffer for
    buffer, what the commit before this op ran (tests/golden/up_phases_parent_schedule.txt: sha256 of the trace of each case, taken on that commit
    with tools/schedule_trace.py's lines), and no launch of the new op may appear."""
    import emu_ops
    assert getattr(trace_ops.TraceOps(), "conv_up_phases_supported", None) is None
    assert getattr(emu_ops.EmuOps(), "conv_up_phases_supported", None) is None
    want = dict(line.rsplit(" ", 1) for line in open(GOLDEN).read().splitlines() if line and not line.startswith("#"))
    got = _digests()
    assert sorted(got) == sorted(want)
    assert [k for k in got if got[k] != want[k]] == []
    log = trace_ops.run_unet(trace_ops.unet_cases()[0]).log
    assert not any(l.op == "conv_up_phases" for l in log)
    assert sum(1 for l in log if l.op == "gemm" and l.args.get("mode") == 2) == 3      # the three FYC_GEMM_CONV3X3_UP2 launches


def test_switch_and_dtype_keep_the_3x3_path(monkeypatch):
    """FYC_UP_PHASES=0, f32, a size that is not 2x, missing phase weights: no group, i.e. today's launch"""
    from followyourclick_amd.engine.base import EngineBase

    class Ops:
        def conv_up_phases_supported(self, dtype, **kw):
            return kw["group_rows"] % 128 == 0

    class E(EngineBase):
        ops, dtype, device, groups = Ops(), torch.bfloat16, "cpu", 32

    e = E()
    w, w_ph = torch.zeros(64, 9 * 64), torch.zeros(4, 64, 4 * 64)
    assert e._up_phases_group(w, w_ph, 4, 8, 16, 16, 32, 4 * 2 * 128) == 256          # clip of two frames
    assert e._up_phases_group(w, w_ph, 4, 8, 16, 16, 32, 4 * 128) == 128              # frame
    assert e._up_phases_group(w, w_ph, 4, 8, 16, 16, 32, 0) == 128                    # no consuming norm: the frame
    assert e._up_phases_group(w, w_ph, 4, 8, 8, 16, 16, 4 * 64) == 0                  # 64-row frames: no row tile divides the group
    assert e._up_phases_group(w, None, 4, 8, 16, 16, 32, 4 * 128) == 0
    assert e._up_phases_group(w, w_ph, 4, 8, 16, 17, 32, 4 * 128) == 0                # up_size of an odd level
    monkeypatch.setenv("FYC_UP_PHASES", "0")
    assert e._up_phases_group(w, w_ph, 4, 8, 16, 16, 32, 4 * 128) == 0
    monkeypatch.delenv("FYC_UP_PHASES")
    e.dtype = torch.float32
    assert e._up_phases_group(w, w_ph, 4, 8, 16, 16, 32, 4 * 128) == 0


def test_packers_keep_the_phase_weights_beside_the_3x3_ones():
    P = trace_ops._packed("unet")
    ups = [blk.up for blk in P.up if blk.up is not None]
    assert len(ups) == 3
    for u in ups:
        O, K9 = u.w.shape
        assert u.w_ph.shape == (4, O, K9 // 9 * 4) and u.w_ph.dtype == u.w.dtype
    V = trace_ops._packed("decode")
    assert all(blk.up.w_ph.shape[0] == 4 for blk in V.ups if blk.up is not None)


def test_header_and_binding_carry_the_entry_points():
    from followyourclick_amd import _lib as L
    head = open(os.path.join(ROOT, "include", "fyc.h")).read()
    assert "#define FYC_VERSION 308" in head and L.FYC_VERSION == 308
    assert "typedef struct { fyc_gemm_args gemm; int32_t group_rows; } fyc_conv_up_phases_args;" in head
    for name in ("fyc_conv_up_phases", "fyc_conv_up_phases_stat_layout", "fyc_conv_up_phases_supported"):
        assert re.search(r"\bint " + name + r"\(", head), name
    assert L.OPS["fyc_conv_up_phases"] is L.ConvUpPhasesArgs
    assert "fyc_conv_up_phases_stat_layout" in L.MISC and "fyc_conv_up_phases_supported" in L.MISC
    import ctypes
    assert L.ConvUpPhasesArgs.gemm.offset == 0 and L.ConvUpPhasesArgs.group_rows.offset == ctypes.sizeof(L.GemmArgs)
    # the public mode enum is what it was: the kernel mode is internal
    assert "enum { FYC_GEMM_PLAIN = 0, FYC_GEMM_CONV3X3 = 1, FYC_GEMM_CONV3X3_UP2 = 2, FYC_GEMM_CONV_T3 = 3 };" in head


def test_queries_and_refusals_without_a_gpu():
    """the support query answers from the shape alone; a refused call returns an error code before anything that needs a device"""
    import ctypes
    from followyourclick_amd import _build, _lib as L
    if not os.path.exists(L.LIB_PATH):
        _build.build(verbose=False)
    lib = L.load()
    q = lib.fyc_conv_up_phases_supported
    assert q(L.FYC_BF16, 1280, 1280, 16, 16, 16 * 256, 1) == 1 and q(L.FYC_F16, 64, 64, 8, 16, 128, 1) == 1
    assert q(L.FYC_F32, 64, 64, 8, 16, 128, 1) == 0          # f32 keeps the 3x3 path
    assert q(L.FYC_BF16, 64, 64, 8, 8, 64, 1) == 0           # G = 64: no row tile divides it
    assert q(L.FYC_BF16, 64, 64, 8, 16, 128, 0) == 0         # not exactly 2x
    assert q(L.FYC_BF16, 72, 64, 8, 16, 128, 1) == 0         # channels are padded to 64 by the caller
    assert q(L.FYC_BF16, 64, 64, 8, 16, 192, 1) == 0         # not whole frames
    u = L.ConvUpPhasesArgs()
    assert lib.fyc_conv_up_phases(ctypes.byref(u), None) != 0 and b"fyc_conv_up_phases" in lib.fyc_last_error()
    tr, sl = L.i32(0), L.i32(0)
    g = u.gemm
    g.M, g.N, g.K, g.ldw, g.ldo, g.Cin, g.Hin, g.Win, g.Hout, g.Wout, g.dtype = 4 * 2 * 256, 128, 256, 256, 128, 64, 16, 16, 32, 32, L.FYC_BF16
    u.group_rows = 256
    assert lib.fyc_conv_up_phases_stat_layout(ctypes.byref(u), ctypes.byref(tr), ctypes.byref(sl)) == 4 * 2 * 256 // tr.value
    assert tr.value in (128, 256) and sl.value == 1
