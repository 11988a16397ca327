"""GroupNorm consumers that fold the row-tile partial sums of their producer themselves (fyc_gn_apply_cs parts1 / parts2,
fyc_panel_linear gn_parts) instead of reading sums a fyc_chan_stats_reduce launch prepared.

The partials always come from a real fyc_gemm (chan_parts).  fyc_gn_apply_cs is driven through the engine's own dispatch
(EngineBase._cs_plan -> UNet3DEngine._act / _gn on a weight-less engine) and checked against torch.nn.functional.group_norm (+SiLU)
in f32 on the CPU, applied to the values the producer stored, at the kernel-output tolerance of the existing fyc_gn_apply_cs test
(tests/test_kernels_gpu.py: RTOL, bf16 4e-3 / f32 2e-5 rel-L2).  The same inputs through the reduce launch must meet the same
bound, so a bound that is loose for both shows here."""
import math

import pytest
import torch

from emu_ops import EmuOps
from followyourclick_amd import _lib as L
from followyourclick_amd.engine import unet3d
from followyourclick_amd.engine.unet3d import UNet3DEngine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
RTOL = {"bf16": 4e-3, "f32": 2e-5}


class Recorder:
    """the HIP ops with the names of the kernels that were asked for"""

    def __init__(self, inner):
        self.inner, self.names, self.kwargs = inner, [], []

    def __getattr__(self, name):
        fn = getattr(self.inner, name)
        if not callable(fn) or name.endswith(("_supported", "_layout", "_bytes", "_parts")) or name in ("ensure_init", "set_tuning"):
            return fn

        def call(*a, **kw):
            self.names.append(name)
            self.kwargs.append(kw)
            return fn(*a, **kw)
        return call


class MiniEngine(UNet3DEngine):
    """the statistics plumbing of UNet3DEngine without a model"""

    def __init__(self, ops, dtype, direct):
        self.ops, self.dtype, self.device, self.groups = ops, dtype, torch.device(DEV), 32
        self.fuse_stats, self.fuse_rows, self.direct_stats = True, False, direct

    def produce(self, a, w, stat_rows, out_rows):
        """x = a w^T by fyc_gemm, with the row-tile partial sums for a norm over `out_rows` rows wherever the plan allows them"""
        rows, (N, K) = a.shape[0], w.shape
        st = self._cs_plan(rows, stat_rows, N, K, L.GEMM_PLAIN, out_rows)
        out = self.new(rows, N)
        self.ops.gemm(a, w, out, M=rows, N=N, K=K, lda=K, ldw=K, ldo=N, chan_parts=None if st is None else st.parts,
                      cs_rows=stat_rows if st is not None else 0)
        return self._act(out, N, st)


@pytest.fixture(scope="module")
def hip():
    from followyourclick_amd import ops
    h = ops.get()
    h.ensure_init(torch.device(DEV))
    return h


def rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def rel(a, b):
    a, b = a.detach().cpu().double().reshape(-1), b.detach().cpu().double().reshape(-1)
    assert torch.isfinite(a).all()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def reference(xs, gamma, beta, rows_per_sample, eps, silu):
    """torch's GroupNorm (+SiLU) in f32 on the values the producers stored"""
    x = torch.cat([t.cpu().float() for t in xs], dim=1)
    rows, C = x.shape
    y = torch.nn.functional.group_norm(x.reshape(rows // rows_per_sample, rows_per_sample, C).permute(0, 2, 1), 32, gamma, beta, eps)
    y = y.permute(0, 2, 1).reshape(rows, C)
    return torch.nn.functional.silu(y) if silu else y


# (name, producers [(N, K)], rows, rows per frame, rows per GroupNorm sample, 128-row tile config for bf16 or 0, expected (tile_rows, slots) in bf16)
CASES = [
    ("tile_spans_two_frames", [(320, 64)], 256, 64, 64, 6, (128, 2)),
    ("tile_spans_two_frames_clip_norm", [(320, 64)], 256, 64, 256, 6, (128, 2)),
    ("16_tiles_per_sample", [(640, 64)], 2048, 1024, 2048, 6, (128, 1)),
    ("split_k_producer", [(1280, 2560)], 128, 64, 128, 0, (128, 2)),
    ("two_source_concat", [(320, 64), (640, 64)], 256, 64, 64, 6, (128, 2)),
]


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gn_apply_cs_folds_the_producers_partials(hip, monkeypatch, dt, case):
    name, prods, rows, frame, rps, tile, layout = case
    T = DT[dt]
    monkeypatch.setattr(unet3d, "DIRECT_STATS_BYTES", 1 << 30)          # the cut-off is a speed choice: here every shape folds directly
    C = sum(n for n, _ in prods)
    gamma, beta = 1 + 0.2 * rnd((C,), torch.float32, 3), 0.1 * rnd((C,), torch.float32, 4)
    ops_in = [(rnd((rows, K), T, 10 + i, 1.3).to(DEV), rnd((N, K), T, 20 + i, 1 / math.sqrt(K)).to(DEV)) for i, (N, K) in enumerate(prods)]
    if dt == "bf16" and tile:
        hip.set_tuning(1, tile)
    try:
        if name == "split_k_producer" and dt == "bf16":
            assert hip.gemm_split_bytes(T, M=rows, N=prods[0][0], K=prods[0][1]) > 0, "this shape is expected to take the split-K path"
        results = {}
        for direct in (True, False):
            rec = Recorder(hip)
            eng = MiniEngine(rec, T, direct)
            acts = [eng.produce(a, w, frame, rps) for a, w in ops_in]
            assert all(a.st is not None and a.st.parts is not None for a in acts)
            if dt == "bf16":
                assert all((a.st.tile_rows, a.st.slots) == layout for a in acts), [(a.st.tile_rows, a.st.slots) for a in acts]
            y, cat = eng._gn(acts[0] if len(acts) == 1 else tuple(acts), gamma.to(DEV), beta.to(DEV), rows, rps, 1e-5, True)
            torch.cuda.synchronize()
            assert cat is None
            assert rec.names.count("gn_apply_cs") == 1 and "gn_stats" not in rec.names
            assert rec.names.count("chan_stats_reduce") == (0 if direct else len(acts)), rec.names
            kw = rec.kwargs[rec.names.index("gn_apply_cs")]
            assert (kw.get("parts1") is not None) == direct and (len(acts) == 1 or (kw.get("parts2") is not None) == direct)
            results[direct] = (y, [a.t for a in acts])
    finally:
        hip.set_tuning(1, 0)
    for direct, (y, xs) in results.items():
        err = rel(y, reference(xs, gamma, beta, rps, 1e-5, True))
        print(f"gn_apply_cs {name} {dt} {'direct fold' if direct else 'reduce launch'}: rel-L2 {err:.3e} (bound {RTOL[dt]:.0e})")
        assert err <= RTOL[dt], (name, dt, direct, err)
    assert torch.equal(results[True][1][0], results[False][1][0])       # same producer output on both paths
    # bitwise repeatable: a second direct run gives the same bits
    eng = MiniEngine(hip, T, True)
    if dt == "bf16" and tile:
        hip.set_tuning(1, tile)
    try:
        acts = [eng.produce(a, w, frame, rps) for a, w in ops_in]
        y2, _ = eng._gn(acts[0] if len(acts) == 1 else tuple(acts), gamma.to(DEV), beta.to(DEV), rows, rps, 1e-5, True)
        torch.cuda.synchronize()
    finally:
        hip.set_tuning(1, 0)
    assert torch.equal(y2, results[True][0])


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_frames_of_75_rows_take_the_statistics_pass(hip, dt):
    """300 rows = 4 frames x 75: 75 % 16 != 0, the plan refuses the fused statistics and the norm runs fyc_gn_stats + fyc_gn_apply"""
    T = DT[dt]
    rows, frame, C, K = 300, 75, 320, 64
    gamma, beta = 1 + 0.2 * rnd((C,), torch.float32, 3), 0.1 * rnd((C,), torch.float32, 4)
    rec = Recorder(hip)
    eng = MiniEngine(rec, T, True)
    act = eng.produce(rnd((rows, K), T, 1, 1.3).to(DEV), rnd((C, K), T, 2, 1 / math.sqrt(K)).to(DEV), frame, frame)
    assert act.st is None
    y, _ = eng._gn(act, gamma.to(DEV), beta.to(DEV), rows, frame, 1e-5, True)
    torch.cuda.synchronize()
    assert rec.names == ["gemm", "gn_stats", "gn_apply"], rec.names
    err = rel(y, reference([act.t], gamma, beta, frame, 1e-5, True))
    print(f"gn fall-back 4 x 75 rows {dt}: rel-L2 {err:.3e} (bound {RTOL[dt]:.0e})")
    assert err <= RTOL[dt], err


def test_cut_off_sends_wide_samples_to_the_reduce_launch(hip, monkeypatch):
    """above DIRECT_STATS_BYTES of partials per consumer block the engine keeps the reduce launch"""
    T = torch.bfloat16
    rows, frame, C, K = 2048, 1024, 640, 64
    a, w = rnd((rows, K), T, 1).to(DEV), rnd((C, K), T, 2, 1 / 8).to(DEV)
    gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    for limit, want in ((1 << 30, 0), (1024, 1)):
        monkeypatch.setattr(unet3d, "DIRECT_STATS_BYTES", limit)
        rec = Recorder(hip)
        eng = MiniEngine(rec, T, True)
        eng._gn(eng.produce(a, w, frame, rows), gamma, beta, rows, rows, 1e-5, False)
        assert rec.names.count("chan_stats_reduce") == want, (limit, rec.names)
    torch.cuda.synchronize()


@pytest.mark.parametrize("C", [320, 640])
def test_panel_linear_folds_the_producers_partials(hip, C):
    """GroupNorm -> proj_in with the norm's sums folded from the partials in fyc_panel_linear's prologue: 2 frames of 128 rows, against the
    op specification (tests/emu_ops.py) on the reduced sums, at the existing tolerance of that op (5e-3)"""
    from followyourclick_amd.engine.weights import pack_panel_linear
    T = torch.bfloat16
    rows, frame, K0 = 256, 128, 64
    a, wp = rnd((rows, K0), T, 1, 1.3).to(DEV), rnd((C, K0), T, 2, 1 / math.sqrt(K0)).to(DEV)
    nt, tile_rows, slots = hip.gemm_stat_layout(T, M=rows, N=C, K=K0, cs_rows=frame)
    parts = torch.full((nt * slots * C * 2,), float("nan"), dtype=torch.float32, device=DEV)
    x = torch.empty(rows, C, dtype=T, device=DEV)
    hip.gemm(a, wp, x, M=rows, N=C, K=K0, lda=K0, ldw=K0, ldo=C, chan_parts=parts, cs_rows=frame)
    cs = torch.empty(rows // frame, C, 2, dtype=torch.float64, device=DEV)
    hip.chan_stats_reduce(parts, cs, rows=rows, N=C, cs_rows=frame, tile_rows=tile_rows, slots=slots)
    w = (rnd((C, C), torch.float32, 3) * C ** -0.5).to(T)
    ws = pack_panel_linear(w)
    bias = rnd((C,), torch.float32, 4) * 0.2
    gamma, beta = rnd((C,), torch.float32, 5) * 0.2 + 1.0, rnd((C,), torch.float32, 6) * 0.2
    kw = dict(wstream=ws.to(DEV), rows=rows, N=C, K=C, bias=bias.to(DEV), gn_gamma=gamma.to(DEV), gn_beta=beta.to(DEV), gn_rows_per_sample=frame,
              gn_stat_samples=1, gn_groups=32, gn_eps=1e-6)
    o_direct = torch.full((rows, C), float("nan"), dtype=T, device=DEV)
    hip.panel_linear(x, o_direct, gn_parts=parts, gn_tile_rows=tile_rows, gn_slots=slots, **kw)
    o_reduced = torch.full((rows, C), float("nan"), dtype=T, device=DEV)
    hip.panel_linear(x, o_reduced, gn_cs=cs, **kw)
    torch.cuda.synchronize()
    o_e = torch.zeros(rows, C, dtype=T)
    EmuOps(acc=torch.float64).panel_linear(x.cpu(), o_e, wstream=ws, rows=rows, N=C, K=C, bias=bias, gn_cs=cs.cpu(), gn_gamma=gamma, gn_beta=beta,
                                           gn_rows_per_sample=frame, gn_stat_samples=1, gn_groups=32, gn_eps=1e-6)
    for tag, o in (("direct fold", o_direct), ("reduced sums", o_reduced)):
        err = rel(o, o_e)
        print(f"panel_linear C{C} {tag}: rel-L2 {err:.3e} (bound 5e-3)")
        assert err <= 5e-3, (tag, err)
    with pytest.raises(Exception, match="fyc_panel_linear"):
        hip.panel_linear(x, o_direct, gn_parts=parts, gn_cs=cs, gn_tile_rows=tile_rows, gn_slots=slots, **kw)
