"""One full-width CFG-pair UNet forward of the SD-2.1 family next to the SD-1.5 forward, and fyc_attention at d = 64 per query tile.

  python tools/sd21_bench.py [--rounds 5] [--sizes 64 96] [--out FILE]

Part 1, per latent size (64x64 = 512^2 pixels, 96x96 = 768^2, SD-2.1's sample_size): ms per UNet3DEngine.forward(shared_prefix=2) - one clip of 16
frames and its CFG duplicate, bf16, random weights - of
  (sd21) widths (320, 640, 1280, 1280), heads (5, 10, 20, 20) = head dim 64, context 1024, use_linear_projection, use_inflated_groupnorm, a mid-block
         motion module: the configuration of the reference's ..._sd_v2.1 YAMLs;
  (sd15) the default configuration (8 heads: head dim 40 / 80 / 160, context 768), the flagship workload of bench.py.
The two alternate inside every round; each figure is the median over the rounds of the mean of 3 back-to-back forwards between two device events, with
the min .. max of the rounds.  Then one instrumented forward per model (an event pair around every launch, queued behind a device-side spin so that the
pairs bracket kernel execution), summed per kernel family as bench.py --full does.

Part 2: the spatial self-attention of the three levels (batch = 32 frames) and the cross-attention of level 0 at d = 64, with tuning key 3 (16-query
tiles per wave, QT) at 0 (the dispatch's own choice: QT = 2 at d = 64), 2, 3, 4, alternating; TFLOP/s counts 4 B H n_q n_k d.

There is no reference golden at full width in a 16-bit type: these are timings of a model whose numerics are checked at the tiny width
(tests/test_sd21_gpu.py) and whose kernels are checked at this head layout there."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from followyourclick_amd import ops  # noqa: E402
from followyourclick_amd.profiling import TimedOps  # noqa: E402

F, B = 16, 2
TUNE_ATTN_VARIANT = 3


def configs():
    from followyourclick_amd.engine import UNet3DConfig
    return {"sd21": UNet3DConfig(attention_head_dim=(5, 10, 20, 20), cross_attention_dim=1024, sample_size=96, use_linear_projection=True,
                                 use_inflated_groupnorm=True, motion_module_mid_block=True, temporal_position_encoding_max_len=32),
            "sd15": UNet3DConfig()}


def build(cfg, dev):
    from followyourclick_amd.engine.schema import random_state_dict, unet_schema
    from followyourclick_amd.engine.unet3d import UNet3DEngine
    from followyourclick_amd.engine.weights import pack_unet
    eng = UNet3DEngine(pack_unet(random_state_dict(unet_schema(cfg), 0), cfg, torch.bfloat16, dev))
    eng.prepare_context(torch.randn(B, 77, cfg.cross_attention_dim, generator=torch.Generator().manual_seed(1)))
    _, temb = eng.prepare_time_embeddings([500], [8.0] * B, [4.0] * B, B)
    return eng, temb


def forwards(engines, dev, size, rounds, lines):
    H = W = size
    x = torch.randn(B // 2 * F * H * W, 64, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).to(dev)
    x[:, 9:] = 0
    for name, (eng, temb) in engines.items():       # warm-up: every shape of the timed window
        out = eng.forward(x, temb, B, F, H, W, shared_prefix=2)
        assert eng.last_schedule == "shared" and torch.isfinite(out.float()).all(), name
    torch.cuda.synchronize()
    times = {k: [] for k in engines}
    for _ in range(rounds):
        for name, (eng, temb) in engines.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(3):
                eng.forward(x, temb, B, F, H, W, shared_prefix=2)
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / 3)
    lines.append(f"UNet3DEngine.forward(shared_prefix=2), full width, bf16, CFG pair of one {F}-frame clip at {H}x{W} latents; {rounds} rounds x 3 forwards, "
                 "median (min .. max) ms")
    for name, t in times.items():
        lines.append(f"    {name}: {statistics.median(t):8.2f} ({min(t):.2f} .. {max(t):.2f}) ms")
    lines.append(f"    sd21 / sd15 = {statistics.median(times['sd21']) / statistics.median(times['sd15']):.3f}")
    for name, (eng, temb) in engines.items():
        timed = TimedOps(eng.ops)
        eng.ops = timed
        try:
            eng.forward(x, temb, B, F, H, W, shared_prefix=2)       # lazy host-side state of the instrumented path
            torch.cuda.synchronize()
            timed.reset()
            torch.cuda._sleep(100_000_000)
            eng.forward(x, temb, B, F, H, W, shared_prefix=2)
            torch.cuda.synchronize()
            summ = timed.summary()
        finally:
            eng.ops = timed.inner
        total = sum(v["ms"] for v in summ.values())
        lines.append(f"    {name} per kernel family, one instrumented forward ({total:.2f} ms of kernel time in {sum(v['launches'] for v in summ.values())} launches):")
        for k, v in sorted(summ.items(), key=lambda kv: -kv[1]["ms"]):
            tf = f"  {v['flops'] / (v['ms'] * 1e-3) / 1e12:6.1f} TFLOP/s" if v["flops"] and v["ms"] > 0 else ""
            lines.append(f"        {k:16s} {v['ms']:8.3f} ms  {v['launches']:4d} launches{tf}")
    lines.append("")
    del x


def attention(h, dev, size, rounds, iters, lines):
    T = torch.bfloat16
    BF = B * F
    shapes = [(f"self  level {i}", BF, heads, (size >> i) ** 2, (size >> i) ** 2, 1) for i, heads in enumerate((5, 10, 20))]
    shapes.append(("cross level 0", BF, 5, size * size, 77, F))
    lines.append(f"fyc_attention, bf16, d = 64, {size}x{size} latents, batch {BF}; {rounds} rounds x {iters} launches, median (min .. max) us per query tile setting")
    g = torch.Generator().manual_seed(3)
    for label, batch, H, nq, nk, div in shapes:
        kvb, ld = (batch + div - 1) // div, (nk + 7) // 8 * 8
        q = torch.randn(batch, H, nq, 64, generator=g).to(T).to(dev)
        k = torch.randn(kvb, H, nk, 64, generator=g).to(T).to(dev)
        vt = torch.zeros(kvb, H, 64, ld, dtype=T)
        vt[..., :nk] = torch.randn(kvb, H, 64, nk, generator=g).to(T)
        vt = vt.to(dev)
        o = torch.empty(batch * nq, H * 64, dtype=T, device=dev)

        def run():
            h.attention(q, k, vt, o, batch=batch, heads=H, n_q=nq, n_k=nk, d=64, ldo=H * 64, ldvt=ld, scale=0.125, kv_batch_div=div)
        times = {qt: [] for qt in (0, 2, 3, 4)}
        try:
            for qt in times:
                h.set_tuning(TUNE_ATTN_VARIANT, qt)
                for _ in range(3):
                    run()
            torch.cuda.synchronize()
            for _ in range(rounds):
                for qt in times:
                    h.set_tuning(TUNE_ATTN_VARIANT, qt)
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for _ in range(iters):
                        run()
                    e.record()
                    torch.cuda.synchronize()
                    times[qt].append(s.elapsed_time(e) / iters * 1e3)
        finally:
            h.set_tuning(TUNE_ATTN_VARIANT, 0)
        flop = 4.0 * batch * H * nq * nk * 64
        lines.append(f"  {label}: H={H} n_q={nq} n_k={nk}")
        for qt, t in times.items():
            med = statistics.median(t)
            lines.append(f"      QT {'auto' if qt == 0 else qt:>4}: {med:9.1f} ({min(t):.1f} .. {max(t):.1f}) us   {flop / med / 1e6:6.1f} TFLOP/s")
        del q, k, vt, o
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 96])
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sd21_bench needs the GPU: timings are not taken anywhere else")
    dev = torch.device("cuda:0")
    h = ops.get()
    h.ensure_init(dev)
    lines = []
    if not a.no_forward:
        engines = {name: build(cfg, dev) for name, cfg in configs().items()}
        for size in a.sizes:
            forwards(engines, dev, size, a.rounds, lines)
        del engines
    for size in a.sizes:
        attention(h, dev, size, a.rounds, a.iters, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
