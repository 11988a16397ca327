"""fyc_attention on f32 tensors with split-bf16 products (the fused flash kernel, csrc/attention_f32x3.hip) against the materialised sequence the engine ran before it
(engine/unet3d.py::_attend: zeros + batched score GEMM + fyc_softmax_rows + batched P V GEMM, all with products="split"), optionally against the fused kernel of
another build of the library (the SLP A/B).

  python tools/attn_f32_bench.py [--other-lib PATH] [--rounds 5] [--out FILE] [--only SUBSTRING]

Shapes: the spatial attentions of the benchmarked UNets - 8 heads of 40 / 80 / 160 / 160 at 64x64 .. 8x8 latents and the SD-2.1 family's heads of 64 - as
self-attention (n_k = n_q), against 77 text keys, and against 16 / 4 image-prompt keys with o_accumulate; a few frames per shape (the materialised sequence runs frame
by frame, the fused call takes them in one launch - as in the engine).  Cold operands: every timed pass walks a ring of operand copies larger than the last-level cache
(at least two copies and 512 MB, at most 16 copies); the materialised side also streams its score tensor.  All variants run in ONE process and alternate inside every
round; each figure is the median over the rounds of the mean time of one attention (all frames) between two device events, min .. max of the rounds as the spread.
The fused kernel is timed as the dispatch chooses its query tiles per wave and, where both are built (d <= 80), with QT forced to 2 and to 4 (tuning key 3).
The verdict the engine's dispatch follows: a shape goes fused only if its SLOWEST fused round beats the FASTEST materialised round."""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from followyourclick_amd import _lib as L  # noqa: E402
from followyourclick_amd import ops  # noqa: E402

# frames, heads, n_q, n_k, d, kv_batch_div, accumulate
SHAPES = [(2, 8, 4096, 4096, 40, 1, False), (8, 8, 1024, 1024, 80, 1, False), (32, 8, 256, 256, 160, 1, False), (32, 8, 64, 64, 160, 1, False),
          (2, 5, 4096, 4096, 64, 1, False), (8, 10, 1024, 1024, 64, 1, False), (32, 20, 256, 256, 64, 1, False), (32, 20, 64, 64, 64, 1, False),
          (4, 8, 4096, 77, 40, 4, False), (8, 8, 1024, 77, 80, 8, False), (32, 8, 256, 77, 160, 16, False), (32, 8, 64, 77, 160, 16, False), (8, 10, 1024, 77, 64, 8, False),
          (4, 8, 4096, 16, 40, 4, True), (4, 8, 4096, 4, 40, 4, True), (32, 8, 256, 16, 160, 16, True), (32, 8, 64, 4, 160, 16, True)]
RING_BYTES = 512 << 20
TUNE_ATTN_VARIANT = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-lib")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    h = ops.get()
    h.ensure_init(dev)
    other = None
    if a.other_lib:
        other = C.CDLL(os.path.abspath(a.other_lib))
        other.fyc_version.restype = C.c_int
        other.fyc_init.argtypes = [C.c_void_p]
        other.fyc_attention.argtypes = [C.POINTER(L.AttnArgs), C.c_void_p]
        assert other.fyc_version() == h.abi_version, "the other library must be a build of the same header"
        zero = torch.zeros(4096, dtype=torch.uint8, device=dev)
        assert other.fyc_init(zero.data_ptr()) == 0
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"fyc_attention, f32 tensors, split-bf16 products, library ABI {h.abi_version}" + (f", other library {a.other_lib}" if other else "") +
             f"; cold ring of operands, {a.rounds} rounds, median (min .. max) us per attention over all frames"]
    for B, H, n_q, n_k, d, div, acc in SHAPES:
        tag = f"frames={B:2d} H={H:2d} n_q={n_q:4d} n_k={n_k:4d} d={d:3d}{' acc' if acc else '    '}"
        if a.only not in tag:
            continue
        C_, ldvt, ldS, kvB, scale = H * d, (n_k + 7) // 8 * 8, (n_k + 7) // 8 * 8, B // div, d ** -0.5
        copy_bytes = (2 * B * H * n_q * d + kvB * H * (n_k + ldvt) * d) * 4
        ring = min(16, max(2, -(-RING_BYTES // copy_bytes)))
        g = torch.Generator(device=dev).manual_seed(1)
        q = [torch.randn(B, H, n_q, d, device=dev, generator=g) for _ in range(ring)]
        k = [torch.randn(kvB, H, n_k, d, device=dev, generator=g) for _ in range(ring)]
        vt = []
        for _ in range(ring):
            t = torch.zeros(kvB, H, d, ldvt, device=dev)      # pad keys are zeros, as the engine writes them
            t[..., :n_k] = torch.randn(kvB, H, d, n_k, device=dev, generator=g)
            vt.append(t)
        prev = torch.randn(B * n_q, C_, device=dev, generator=g)
        outs = {name: [prev.clone() for _ in range(ring)] for name in ("fused", "qt2", "qt4", "other", "materialised")}
        kw = dict(batch=B, heads=H, n_q=n_q, n_k=n_k, d=d, ldo=C_, ldvt=ldvt, scale=scale, kv_batch_div=div, accumulate=acc, o_scale=0.7)

        def fused(name, qt):
            def run(i):
                if qt:
                    h.set_tuning(TUNE_ATTN_VARIANT, qt)
                h.attention(q[i], k[i], vt[i], outs[name][i], products="split", **kw)
                if qt:
                    h.set_tuning(TUNE_ATTN_VARIANT, 0)
            return run

        def call_other(i):
            oa = L.AttnArgs()
            oa.q, oa.k, oa.vt, oa.o = q[i].data_ptr(), k[i].data_ptr(), vt[i].data_ptr(), outs["other"][i].data_ptr()
            oa.batch, oa.heads, oa.n_q, oa.n_k, oa.d, oa.ldo, oa.ldvt = B, H, n_q, n_k, d, C_, ldvt
            oa.kv_batch_div, oa.o_accumulate, oa.scale, oa.o_scale, oa.dtype, oa.f32_products = div, int(acc), scale, 0.7, L.FYC_F32, L.PRODUCTS_SPLIT_BF16
            rc = other.fyc_attention(C.byref(oa), stream)
            assert rc == 0, rc

        def materialised(i):      # engine/unet3d.py::_attend's sequence, call for call
            out = outs["materialised"][i]
            for b in range(B):
                kb = b // div
                S = torch.zeros(H, n_q, ldS, device=dev)
                h.gemm(q[i][b], k[i][kb], S, M=n_q, N=n_k, K=d, lda=d, ldw=d, ldo=ldS, batch=H, stride_a=n_q * d, stride_w=n_k * d, stride_o=n_q * ldS, out_scale=scale,
                       products="split")
                h.softmax_rows(S, rows=H * n_q, cols=n_k, ld=ldS)
                dst = out[b * n_q:(b + 1) * n_q]
                if acc:
                    tmp = torch.empty(n_q, C_, device=dev)
                    h.gemm(S, vt[i][kb], tmp, M=n_q, N=d, K=ldS, lda=ldS, ldw=ldvt, ldo=C_, batch=H, stride_a=n_q * ldS, stride_w=d * ldvt, stride_o=d, products="split")
                    dst.add_(tmp, alpha=0.7)
                else:
                    h.gemm(S, vt[i][kb], dst, M=n_q, N=d, K=ldS, lda=ldS, ldw=ldvt, ldo=C_, batch=H, stride_a=n_q * ldS, stride_w=d * ldvt, stride_o=d, products="split")

        variants = {"fused": fused("fused", 0)}
        if d <= 80:
            variants["qt2"], variants["qt4"] = fused("qt2", 2), fused("qt4", 4)
        if other is not None:
            variants["other"] = call_other
        variants["materialised"] = materialised
        times = {name: [] for name in variants}
        for fn in variants.values():      # warm-up: code objects, LDS attributes, the allocator's blocks
            fn(0)
        torch.cuda.synchronize()
        for name in variants:             # the warm-up accumulated once into copy 0: start every variant from the same values again
            outs[name][0].copy_(prev)
        for _ in range(a.rounds):
            for name, fn in variants.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for i in range(ring):
                    fn(i)
                e.record()
                torch.cuda.synchronize()
                times[name].append(s.elapsed_time(e) / ring * 1e3)
        label = {"fused": "fused (dispatch)", "qt2": "fused, QT = 2", "qt4": "fused, QT = 4", "other": "fused, other library", "materialised": "materialised"}
        for name, t in times.items():
            lines.append(f"{tag} {label[name]:21s}: {statistics.median(t):9.1f} ({min(t):.1f} .. {max(t):.1f}) us   (ring of {ring})")
        fu, ma = outs["fused"][1].double(), outs["materialised"][1].double()      # (copy 1 was written rounds times from the same inputs, or accumulated rounds times on both sides)
        wins = max(times["fused"]) < min(times["materialised"])
        lines.append(f"{tag} fused vs materialised rel-L2 {((fu - ma).norm() / ma.norm()).item():.2e};  speed-up {statistics.median(times['materialised']) / statistics.median(times['fused']):.1f} x;  "
                     f"slowest fused round {max(times['fused']):.1f} us {'<' if wins else '>='} fastest materialised round {min(times['materialised']):.1f} us: "
                     f"{'FUSED' if wins else 'stays materialised'}")
        del q, k, vt, outs
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
