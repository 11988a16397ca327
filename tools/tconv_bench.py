"""FYC_GEMM_CONV_T3 timing, and the whole UNet forward with and without the two options it serves.

  python tools/tconv_bench.py [--rounds 7] [--iters 20] [--no-forward] [--out FILE]

Part 1, per shape (the UNet's T3 shapes at 16 frames, 512^2, CFG batch 2, bf16), three ways to compute the same convolution:
  (i)   one FYC_GEMM_CONV_T3 launch with bias, residual and output statistics;
  (ii)  the PLAIN fyc_gemm at the same M, N, K = 3C with the same epilogue inputs - the same work minus the gather: the yardstick;
  (iii) what the library could run before this mode: PLAIN launches that accumulate the three taps on row-shifted views, the centre tap over
        all rows and the two neighbour taps per clip (1 + 2 * clips launches; no statistics - they would need a pass of their own).
The variants alternate inside every round, so that they share whatever else the machine is doing; each figure is the median over the rounds of
the mean time of `iters` back-to-back launches between two device events, with the min .. max of the rounds as the spread.  TFLOP/s counts
2 * M * C * 3C.  (iii) is checked against (i) before it is timed.

Part 2: ms per forward of the full-width UNet (random weights) with (a) neither option, (b) use_inflated_groupnorm, (c) both, alternating."""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from followyourclick_amd import _lib as L  # noqa: E402
from followyourclick_amd import ops  # noqa: E402

F, CLIPS = 16, 2
# (label, pixels per frame, C, residual)
SHAPES = [("64x64  C=320 ", 4096, 320, True), ("32x32  C=640 ", 1024, 640, True), ("16x16  C=1280", 256, 1280, True), ("8x8    C=1280", 64, 1280, True),
          ("64x64  C=320 conv1-3 form (no residual), as in the up path", 4096, 320, False)]


def timed(variants, rounds, iters):
    times = {k: [] for k in variants}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in variants.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / iters * 1e3)
    return times


def per_shape(h, dev, rounds, iters, lines):
    T = torch.bfloat16
    lines.append(f"FYC_GEMM_CONV_T3, bf16, {CLIPS} clips x {F} frames; {rounds} rounds x {iters} launches, median (min .. max) us, TFLOP/s of 2*M*C*3C")
    for label, hw, C, with_res in SHAPES:
        M, K = CLIPS * F * hw, 3 * C
        g = torch.Generator(device="cpu").manual_seed(C + hw)
        x = torch.randn(M, C, generator=g).to(T).to(dev)
        w3 = (torch.randn(C, C, 3, generator=g) / math.sqrt(K)).to(T)             # (O, I, tap)
        w = w3.reshape(C, C // 64, 64, 3).permute(0, 1, 3, 2).reshape(C, K).contiguous().to(dev)      # [O][slab][tap][c]
        wt = [w3[:, :, t].contiguous().to(dev) for t in range(3)]
        xg = torch.randn(M, K, generator=g).to(T).to(dev)                          # the yardstick's operand: any [M][3C]
        bias = torch.randn(C, generator=g).to(dev)
        res = torch.randn(M, C, generator=g).to(T).to(dev) if with_res else None
        o1, o2, o3 = (torch.empty(M, C, dtype=T, device=dev) for _ in range(3))
        st = {}
        for mode in (L.GEMM_CONV_T3, L.GEMM_PLAIN):
            nt, tr, sl = h.gemm_stat_layout(T, M=M, N=C, K=K, cs_rows=hw, mode=mode)
            st[mode] = torch.empty(nt * sl * C * 2, dtype=torch.float32, device=dev)
        kw = dict(M=M, N=C, K=K, ldw=K, ldo=C, ldr=C, bias=bias, residual=res, cs_rows=hw)

        def t3():
            h.gemm(x, w, o1, lda=C, mode=L.GEMM_CONV_T3, conv=dict(Cin=C, frames=F, rows=hw), chan_parts=st[L.GEMM_CONV_T3], **kw)

        def plain():
            h.gemm(xg, w, o2, lda=K, chan_parts=st[L.GEMM_PLAIN], **kw)

        def shifted():
            h.gemm(x, wt[1], o3, M=M, N=C, K=C, lda=C, ldw=C, ldo=C, ldr=C, bias=bias, residual=res)
            rows = (F - 1) * hw
            for c in range(CLIPS):
                r0 = c * F * hw
                lo, hi = o3[r0 + hw:r0 + F * hw], o3[r0:r0 + rows]
                h.gemm(x[r0:r0 + rows], wt[0], lo, M=rows, N=C, K=C, lda=C, ldw=C, ldo=C, ldr=C, residual=lo)          # frame f reads f - 1
                h.gemm(x[r0 + hw:r0 + F * hw], wt[2], hi, M=rows, N=C, K=C, lda=C, ldw=C, ldo=C, ldr=C, residual=hi)   # frame f reads f + 1
        t3()
        shifted()
        torch.cuda.synchronize()
        d = ((o1.float() - o3.float()).norm() / o1.float().norm()).item()
        assert d < 2e-2, f"the shifted-view composition disagrees with CONV_T3: rel-L2 {d}"
        times = timed({"t3": t3, "plain": plain, "shifted": shifted}, rounds, iters)
        flop = 2.0 * M * C * K
        med = {k: statistics.median(v) for k, v in times.items()}
        lines.append(f"M={M:6d} {label}   (shifted-view result vs CONV_T3: rel-L2 {d:.1e}, two more roundings)")
        for name, tag in (("t3", "(i)   CONV_T3, one launch          "), ("plain", "(ii)  PLAIN, same M N K            "),
                          ("shifted", f"(iii) PLAIN x {1 + 2 * CLIPS}, shifted row views ")):
            t = times[name]
            lines.append(f"    {tag}: {med[name]:8.1f} ({min(t):.1f} .. {max(t):.1f}) us   {flop / med[name] / 1e6:6.1f} TFLOP/s")
        sp = (max(times["plain"]) - min(times["plain"])) / med["plain"]
        lines.append(f"    (i)/(ii) = {med['t3'] / med['plain']:.3f}   (i)/(iii) = {med['t3'] / med['shifted']:.3f}   spread of (ii) over the rounds: {100 * sp:.1f} %")
        del x, xg, o1, o2, o3, res


def whole_forward(dev, rounds, lines):
    from followyourclick_amd.engine import UNet3DConfig
    from followyourclick_amd.engine.schema import random_state_dict, unet_schema
    from followyourclick_amd.engine.unet3d import UNet3DEngine
    from followyourclick_amd.engine.weights import pack_unet
    B, H, W = 2, 64, 64
    engines = {}
    sd = None
    for name, opts in (("c", dict(use_inflated_groupnorm=True, use_temporal_conv=True)), ("b", dict(use_inflated_groupnorm=True)), ("a", {})):
        cfg = UNet3DConfig(**opts)
        keys = unet_schema(cfg)
        if sd is None:
            sd = random_state_dict(keys, 0)        # the superset (c); (a) and (b) take the entries they know
        eng = UNet3DEngine(pack_unet({k: sd[k] for k in keys}, cfg, torch.bfloat16, dev))
        eng.prepare_context(torch.randn(B, 77, cfg.cross_attention_dim, generator=torch.Generator().manual_seed(1)))
        _, temb = eng.prepare_time_embeddings([500], [8.0] * B, [4.0] * B, B)
        engines[name] = (eng, temb)
    x = torch.randn(B * F * H * W, 64, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).to(dev)
    x[:, 9:] = 0
    times = {k: [] for k in ("a", "b", "c")}
    for k in times:
        eng, temb = engines[k]
        out = eng.forward(x, temb, B, F, H, W)
        assert torch.isfinite(out.float()).all(), k
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k in ("a", "b", "c"):
            eng, temb = engines[k]
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(3):
                eng.forward(x, temb, B, F, H, W)
            e.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e) / 3)
    # the temporal blocks' matrix work: per ResNet 4 convolutions of 2 * M * C * 3C
    boc, lpb = (320, 640, 1280, 1280), 2
    levels = [(B * F * (H >> i) * (W >> i), c) for i, c in enumerate(boc)]
    n_res = [lpb + (lpb + 1) for _ in boc]
    n_res[-1] += 2                                   # the mid block's two ResNets run at the last level's size
    flop = sum(n * 4 * 2.0 * m * c * 3 * c for n, (m, c) in zip(n_res, levels))
    lines.append("")
    lines.append(f"UNet3DEngine.forward, full width, bf16, {B} clips x {F} frames x {H}x{W} latents (plain schedule, random weights); {rounds} rounds x 3 forwards, median (min .. max) ms")
    for k, tag in (("a", "(a) neither option               "), ("b", "(b) use_inflated_groupnorm       "), ("c", "(c) both (+ 88 CONV_T3 launches)")):
        t = times[k]
        lines.append(f"    {tag}: {statistics.median(t):8.2f} ({min(t):.2f} .. {max(t):.2f}) ms")
    extra = statistics.median(times["c"]) - statistics.median(times["b"])
    lines.append(f"    (c) - (b) = {extra:.2f} ms for {flop / 1e12:.2f} TFLOP of temporal convolutions ({sum(n_res)} ResNets x 4) plus their 88 GroupNorm + SiLU passes: "
                 f"{flop / extra / 1e9:.0f} TFLOP/s over that difference")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tconv_bench needs the GPU: timings are not taken anywhere else")
    dev = torch.device("cuda:0")
    h = ops.get()
    h.ensure_init(dev)
    lines = []
    per_shape(h, dev, a.rounds, a.iters, lines)
    if not a.no_forward:
        whole_forward(dev, a.rounds, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
