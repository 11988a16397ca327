"""The attention call sites beside the UNet - the VAE's mid block (one head of 512) and the encoders (CLIP text: causal; CLIP vision; Resampler) - as ONE fyc_attention
launch (ABI 308: causal mask, head dims up to 512; csrc/attention_wide.h and, for d <= 160 without the mask, the kernels of ABI 307) against the materialised sequence
the engines ran before (engine/vae.py: zeros / empty + batched score GEMM + fyc_softmax_rows + batched P V GEMM over all frames; engine/encoders.py: the same three
launches per batch element, fyc_softmax_rows with causal_rows for the text tower).

  python tools/wide_attn_bench.py [--rounds 5] [--out FILE] [--only SUBSTRING] [--dtypes bf16,f16,f32]

In the pattern of tools/attn_f32_bench.py: device events, every variant warmed up on every shape, a ring of operand copies (at least two), fused and materialised
alternating inside every round of one process; each figure is the median over the rounds of the mean time of one attention, min .. max of the rounds as the spread.
f32 runs with split-bf16 products on both sides.  TFLOP/s = 4 B H n_q n_k d / time (causal: half of that, the visible triangle), and its share of the bf16 MFMA peak of
2500 TFLOP/s (the tier issues three matrix instructions per product: its share counts the useful third).
The verdict the engines' dispatch follows (engine/base.py::SIDE_FLASH_DEFAULT): a family goes fused by default only if its SLOWEST fused round beats the FASTEST
materialised round."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from followyourclick_amd import ops  # noqa: E402

# family, batch (frames), heads, n_q, n_k, d, causal, batched (True: the VAE's sequence, one batched GEMM over the frames; False: the encoders', per batch element)
SHAPES = [("vae", 16, 1, 4096, 4096, 512, False, True), ("vae-768", 4, 1, 9216, 9216, 512, False, True),
          ("clip_text", 2, 12, 77, 77, 64, True, False), ("clip_vision", 1, 16, 257, 257, 80, False, False), ("resampler", 1, 12, 16, 273, 64, False, False)]
RING_BYTES = 512 << 20
PEAK_TFLOPS = 2500.0
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--only", default="")
    ap.add_argument("--dtypes", default="bf16,f16,f32")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    h = ops.get()
    h.ensure_init(dev)
    sink = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        sink = open(a.out, "w")

    class Lines(list):      # every line is printed and written as it is measured: a long job shows where it is
        def append(self, line):
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
                sink.flush()
    lines = Lines()
    lines.append(f"fyc_attention beside the UNet, library ABI {h.abi_version}; ring of operand copies, {a.rounds} rounds, median (min .. max) us per attention over the whole batch")
    for fam, B, H, n_q, n_k, d, causal, batched in SHAPES:
        for dt in a.dtypes.split(","):
            T, es = DT[dt], 2 if dt != "f32" else 4
            tag = f"{fam:11s} {dt:4s} B={B:2d} H={H:2d} n_q={n_q:4d} n_k={n_k:4d} d={d:3d}{' causal' if causal else '       '}"
            if a.only not in tag:
                continue
            prod = dict(products="split") if dt == "f32" else {}
            C_, ld, scale = H * d, (n_k + 7) // 8 * 8, d ** -0.5
            copy_bytes = B * H * (2 * n_q + n_k + ld) * d * es
            ring = min(16, max(2, -(-RING_BYTES // copy_bytes)))
            g = torch.Generator(device=dev).manual_seed(1)
            q = [torch.randn(B, H, n_q, d, device=dev, generator=g).to(T) for _ in range(ring)]
            k = [torch.randn(B, H, n_k, d, device=dev, generator=g).to(T) for _ in range(ring)]
            vt = []
            for _ in range(ring):
                t = torch.zeros(B, H, d, ld, device=dev, dtype=T)      # pad keys are zeros, as the engines write them
                t[..., :n_k] = torch.randn(B, H, d, n_k, device=dev, generator=g).to(T)
                vt.append(t)
            outs = {name: [torch.zeros(B * n_q, C_, device=dev, dtype=T) for _ in range(ring)] for name in ("fused", "materialised")}

            def fused(i):
                h.attention(q[i], k[i], vt[i], outs["fused"][i], batch=B, heads=H, n_q=n_q, n_k=n_k, d=d, ldo=C_, ldvt=ld, scale=scale, causal=causal, **prod)

            def materialised(i):
                out = outs["materialised"][i]
                if batched:      # engine/vae.py::attention (heads = 1)
                    S = torch.zeros(B, n_q, ld, device=dev, dtype=T) if ld != n_k else torch.empty(B, n_q, ld, device=dev, dtype=T)
                    h.gemm(q[i], k[i], S, M=n_q, N=n_k, K=d, lda=d, ldw=d, ldo=ld, batch=B, stride_a=n_q * d, stride_w=n_k * d, stride_o=n_q * ld, out_scale=scale, **prod)
                    h.softmax_rows(S, rows=B * n_q, cols=n_k, ld=ld)
                    h.gemm(S, vt[i], out, M=n_q, N=d, K=ld, lda=ld, ldw=ld, ldo=d, batch=B, stride_a=n_q * ld, stride_w=d * ld, stride_o=n_q * d, **prod)
                    return
                for b in range(B):      # engine/encoders.py::attention
                    S = torch.zeros(H, n_q, ld, device=dev, dtype=T)
                    h.gemm(q[i][b], k[i][b], S, M=n_q, N=n_k, K=d, lda=d, ldw=d, ldo=ld, batch=H, stride_a=n_q * d, stride_w=n_k * d, stride_o=n_q * ld, out_scale=scale, **prod)
                    h.softmax_rows(S, rows=H * n_q, cols=n_k, ld=ld, causal_rows=n_q if causal else 0)
                    h.gemm(S, vt[i][b], out[b * n_q:(b + 1) * n_q], M=n_q, N=d, K=ld, lda=ld, ldw=ld, ldo=C_, batch=H, stride_a=n_q * ld, stride_w=d * ld, stride_o=d, **prod)

            variants = {"fused": fused, "materialised": materialised}
            times = {name: [] for name in variants}
            for fn in variants.values():      # warm-up of every shape: code objects, LDS attributes, the allocator's blocks
                fn(0)
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for name, fn in variants.items():
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for i in range(ring):
                        fn(i)
                    e.record()
                    torch.cuda.synchronize()
                    times[name].append(s.elapsed_time(e) / ring * 1e3)
            flop = 4.0 * B * H * n_q * n_k * d * (0.5 if causal else 1.0)
            for name, t in times.items():
                tf = flop / (statistics.median(t) * 1e-6) / 1e12
                lines.append(f"{tag} {name:12s}: {statistics.median(t):10.1f} ({min(t):.1f} .. {max(t):.1f}) us  {tf:7.1f} TFLOP/s = {100 * tf / PEAK_TFLOPS:5.2f} % of the bf16 MFMA peak  (ring of {ring})")
            fu, ma = outs["fused"][1].double(), outs["materialised"][1].double()
            wins = max(times["fused"]) < min(times["materialised"])
            lines.append(f"{tag} fused vs materialised rel-L2 {((fu - ma).norm() / ma.norm()).item():.2e};  speed-up {statistics.median(times['materialised']) / statistics.median(times['fused']):.2f} x;  "
                         f"slowest fused round {max(times['fused']):.1f} us {'<' if wins else '>='} fastest materialised round {min(times['materialised']):.1f} us: "
                         f"{'FUSED' if wins else 'stays materialised'}")
            del q, k, vt, outs
            torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
