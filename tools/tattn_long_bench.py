"""Per-launch time of the long-clip temporal attention kernel (csrc/temporal_attn_long.hip), and the long against the register-resident kernel
at 64 frames.

  python tools/tattn_long_bench.py [--rounds 7] [--iters 20] [--out profiles/long_clip.txt]

Shapes: the three UNet levels of a 512 x 512 clip with the CFG batch of 2 - (pixels, heads x d) = (4096, 8 x 40), (1024, 8 x 80), (256, 8 x 160) -
in bf16, NULL tables and RoPE, at 96, 128 and 256 frames through fyc_temporal_attention; at 64 frames fyc_temporal_attention (the register-
resident kernel) against fyc_temporal_attention_long.  A shape whose tensors do not fit the device is reported as not measured.

All variants of a shape run in ONE process and alternate inside every round, so that they share whatever else the machine is doing; every
variant is warmed up first; each figure is the median over the rounds of the mean time of `iters` back-to-back launches between two device
events, with the min .. max of the rounds as the spread.  Device-event time of back-to-back launches includes the launch gaps (a few us, small
against these kernels); the clocks are whatever the device ran at - compare variants inside one run, not across runs.
Bytes: q, k, v read once and o written once (what the algorithm needs; the kernels' HBM traffic was not counted here).  FLOP: 4 F^2 d per
(clip, pixel, head) task - both products, padding and the softmax not counted - over the launch time: the rate of useful matrix work, not a
share of the MFMA peak."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from followyourclick_amd import ops  # noqa: E402
from followyourclick_amd.engine.weights import rope_tables  # noqa: E402

LEVELS = ((4096, 8, 40), (1024, 8, 80), (256, 8, 160))
CLIPS = 2


def measure(variants, rounds, iters):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    h = ops.get()
    h.ensure_init(dev)
    lines = [f"temporal attention over long clips, bf16, {CLIPS} clips (CFG pair) of a 512 x 512 video; {torch.cuda.get_device_name(0)}, library ABI {h.abi_version}",
             f"{a.rounds} rounds x {a.iters} launches per variant, variants alternating inside a round; median (min .. max) us per launch",
             "GB = q|k|v read + o written once; TB/s and TFLOP/s (4 F^2 d per task) are that work over the launch time", ""]
    for F in (64, 96, 128, 256):
        for P, H, d in LEVELS:
            head = f"F={F:3d} pixels={P:4d} heads x d = {H} x {d:3d}"
            try:
                qkv = torch.randn(CLIPS * F * P, 3 * H * d, device=dev, dtype=torch.bfloat16)
                outs = [torch.empty(CLIPS * F * P, H * d, dtype=torch.bfloat16, device=dev) for _ in range(2)]
            except torch.cuda.OutOfMemoryError:
                lines.append(f"{head}: not measured (the tensors do not fit the device)")
                continue
            kw = dict(clips=CLIPS, frames=F, pixels=P, heads=H, d=d, scale=d ** -0.5)
            tables = tuple(t.to(dev) for t in rope_tables(d, F))
            if F <= 64:
                variants = {"register-resident kernel": lambda: h.temporal_attention(qkv, outs[0], **kw),
                            "long kernel": lambda: h.temporal_attention(qkv, outs[1], kernel="long", **kw),
                            "register-resident kernel, RoPE": lambda: h.temporal_attention(qkv, outs[0], rope=tables, **kw),
                            "long kernel, RoPE": lambda: h.temporal_attention(qkv, outs[1], kernel="long", rope=tables, **kw)}
            else:
                variants = {"long kernel": lambda: h.temporal_attention(qkv, outs[0], **kw),
                            "long kernel, RoPE": lambda: h.temporal_attention(qkv, outs[1], rope=tables, **kw)}
            times = measure(variants, a.rounds, a.iters)
            nbytes = 4.0 * CLIPS * F * P * H * d * 2
            flop = 4.0 * F * F * d * CLIPS * P * H
            for name, t in times.items():
                med = statistics.median(t)
                lines.append(f"{head} {name:31s}: {med:9.1f} ({min(t):.1f} .. {max(t):.1f}) us   {nbytes / 1e9:5.2f} GB  {nbytes / med / 1e6:5.2f} TB/s  {flop / med / 1e6:6.1f} TFLOP/s")
            if F <= 64:
                m = {k: statistics.median(v) for k, v in times.items()}
                lines.append(f"{head} long / register-resident: {m['long kernel'] / m['register-resident kernel']:.2f}x the time (NULL tables), "
                             f"{m['long kernel, RoPE'] / m['register-resident kernel, RoPE']:.2f}x (RoPE)")
            del qkv, outs
            torch.cuda.empty_cache()
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
