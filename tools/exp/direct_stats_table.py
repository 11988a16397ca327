"""Cut-off table for the direct statistics fold: per consumer shape of the headline workload (B = 2, 16 frames, 512^2), the time of
[fyc_chan_stats_reduce + consumer on reduced sums] against [consumer folding the partials itself], back to back on one stream."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from followyourclick_amd import ops as ops_mod  # noqa: E402
from followyourclick_amd.engine.weights import pack_panel_linear  # noqa: E402

DEV = torch.device("cuda:0")
hip = ops_mod.get()
hip.ensure_init(DEV)
T = torch.bfloat16
FR = 32          # frames of the CFG pair
lines = []


def timeit(fn, iters=40, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(3):
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        best = min(best, s.elapsed_time(e) * 1000.0 / iters)
    return best


def case(level, frame, Cs, clip, tile_rows, slots, consumer):
    rows = FR * frame
    rps = frame * (16 if clip else 1)
    C = sum(Cs)
    xs = [torch.randn(rows, c, device=DEV).to(T) for c in Cs]
    nt = (rows + tile_rows - 1) // tile_rows
    parts = [torch.rand(nt * slots * c * 2, device=DEV) for c in Cs]
    cs = [torch.empty(rows // rps, c, 2, dtype=torch.float64, device=DEV) for c in Cs]
    gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    y = torch.empty(rows, C, dtype=T, device=DEV)
    tiles = max(rps // tile_rows, 1)
    kb = tiles * slots * C * 8 / 1024.0

    def reduce_all():
        for p, c_, n in zip(parts, cs, Cs):
            hip.chan_stats_reduce(p, c_, rows=rows, N=n, cs_rows=frame, tile_rows=tile_rows, slots=slots, out_rows=rps)
    if consumer == "gn_apply_cs":
        kw = dict(rows=rows, C1=Cs[0], groups=32, rows_per_sample=rps, eps=1e-5, silu=clip)
        two = len(Cs) == 2

        def old():
            reduce_all()
            hip.gn_apply_cs(xs[0], cs[0], gamma, beta, y, cs_rows=rps, x2=xs[1] if two else None, cs2=cs[1] if two else None, C2=Cs[1] if two else 0, **kw)

        def new():
            hip.gn_apply_cs(xs[0], None, gamma, beta, y, parts1=parts[0], tile_rows1=tile_rows, slots1=slots, parts_cs_rows=frame,
                            x2=xs[1] if two else None, parts2=parts[1] if two else None, tile_rows2=tile_rows, slots2=slots, C2=Cs[1] if two else 0, **kw)
    else:
        w = (torch.randn(C, C) * C ** -0.5).to(T)
        ws = pack_panel_linear(w).to(DEV)
        bias = torch.zeros(C, device=DEV)
        kw = dict(wstream=ws, rows=rows, N=C, K=C, bias=bias, gn_gamma=gamma, gn_beta=beta, gn_rows_per_sample=rps, gn_groups=32, gn_eps=1e-6)

        def old():
            reduce_all()
            hip.panel_linear(xs[0], y, gn_cs=cs[0], gn_stat_samples=1, **kw)

        def new():
            hip.panel_linear(xs[0], y, gn_parts=parts[0], gn_tile_rows=tile_rows, gn_slots=slots, gn_stat_samples=rps // frame, **kw)
    t_old, t_new = timeit(old), timeit(new)
    line = (f"{level:>6} {consumer:>12} {'clip' if clip else 'frame':>5} C={'+'.join(map(str, Cs)):>9} tile_rows={tile_rows:3d} slots={slots} tiles/sample={tiles:3d} "
            f"partials/block={kb:7.1f} KB   reduce+consumer {t_old:7.1f} us   direct {t_new:7.1f} us   gain {t_old - t_new:+6.1f} us")
    print(line, flush=True)
    lines.append(line)


for lvl, frame, C in (("64x64", 4096, 320), ("32x32", 1024, 640), ("16x16", 256, 1280), ("8x8", 64, 1280)):
    rows = FR * frame
    conv = hip.gemm_stat_layout(T, M=rows, N=C, K=9 * C, cs_rows=frame, mode=1)
    lin = hip.gemm_stat_layout(T, M=rows, N=C, K=5 * C, cs_rows=frame, mode=0)
    line = f"layout {lvl}: conv3x3 (tiles, tile_rows, slots) = {conv}, feed-forward output GEMM K = 5C: {lin}"
    print(line, flush=True)
    lines.append(line)
# per-frame norms (in front of a transformer / motion module); producers: 256-row conv tiles, 128-row ff_block / split-K tiles
case("64x64", 4096, [320], False, 256, 1, "panel_linear")
case("64x64", 4096, [320], False, 128, 1, "panel_linear")
case("32x32", 1024, [640], False, 256, 1, "panel_linear")
case("32x32", 1024, [640], False, 128, 1, "panel_linear")
case("16x16", 256, [1280], False, 256, 1, "gn_apply_cs")
case("16x16", 256, [1280], False, 128, 1, "gn_apply_cs")
case("8x8", 64, [1280], False, 128, 2, "gn_apply_cs")
case("8x8", 64, [1280], False, 256, 4, "gn_apply_cs")
# clip-level norms (ResNet norm1 / norm2, conv_norm_out), single source and the up blocks' concat
case("8x8", 64, [1280], True, 128, 2, "gn_apply_cs")
case("8x8", 64, [1280, 1280], True, 128, 2, "gn_apply_cs")
case("16x16", 256, [1280], True, 256, 1, "gn_apply_cs")
case("16x16", 256, [1280, 1280], True, 256, 1, "gn_apply_cs")
case("16x16", 256, [1280, 640], True, 256, 1, "gn_apply_cs")
case("32x32", 1024, [640], True, 256, 1, "gn_apply_cs")
case("32x32", 1024, [640, 640], True, 256, 1, "gn_apply_cs")
case("64x64", 4096, [320], True, 256, 1, "gn_apply_cs")
case("64x64", 4096, [320, 320], True, 256, 1, "gn_apply_cs")
if len(sys.argv) > 1:            # optional: also keep the table in a file
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
