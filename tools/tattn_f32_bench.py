"""fyc_temporal_attention on f32 tensors: the exact (scalar) kernel against the split-bf16 matrix-instruction kernel (f32_products), optionally against the
exact kernel of another build of the library.

  python tools/tattn_f32_bench.py [--other-lib PATH] [--rounds 7] [--out FILE]

Shapes: the motion-module levels of the benchmarked clips (2 clips x 16 frames at 64x64 .. 8x8 latents, 8 heads of 40 / 80 / 160 / 160), one 32-frame clip at
96x96 and one 64-frame clip with RoPE.  Cold operands: every launch of a timed run reads and writes its own copy of qkv / o out of a ring that is larger than
the last-level cache (at least two copies and 768 MB), so no launch finds what the previous one left there.  All variants run in ONE process and alternate inside
every round, so that they share whatever else the machine is doing; each figure is the median over the rounds of the mean time of one pass over the ring between
two device events, with the min .. max of the rounds as the spread.  TB/s counts 16 C bytes per token row: q, k, v read once, o written once, 4 bytes each.
--other-lib: a libfyc_hip.so built from another commit (FYC_BUILD_LIB=... python -m followyourclick_amd._build), called through the argument struct of ABI 305 -
the prefix of today's - for the exact kernel.  (FYC_LIB_PATH=<that library> runs the whole tool on it instead; a library older than ABI 306 has no split kernel
and only its exact timings are printed.)  The exact outputs of the two libraries are compared bit for bit, the split output with the exact one in relative L2."""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from followyourclick_amd import _lib as L  # noqa: E402
from followyourclick_amd import ops  # noqa: E402
from followyourclick_amd.engine.weights import rope_tables  # noqa: E402

SHAPES = [(2, 16, 4096, 8, 40, False), (2, 16, 1024, 8, 80, False), (2, 16, 256, 8, 160, False), (2, 16, 64, 8, 160, False), (1, 32, 9216, 8, 40, False),
          (1, 64, 1024, 8, 80, True)]      # clips, F, pixels, heads, d, RoPE
RING_BYTES = 768 << 20


class OldTAttnArgs(C.Structure):      # fyc_tattn_args before f32_products was appended
    _fields_ = L.TAttnArgs._fields_[:11]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-lib")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    h = ops.get()
    h.ensure_init(dev)
    has_split = h.abi_version >= 306
    other = None
    if a.other_lib:
        other = C.CDLL(os.path.abspath(a.other_lib))
        other.fyc_version.restype = C.c_int
        other.fyc_init.argtypes = [C.c_void_p]
        other.fyc_temporal_attention.argtypes = [C.POINTER(OldTAttnArgs), C.c_void_p]
        zero = torch.zeros(4096, dtype=torch.uint8, device=dev)
        assert other.fyc_init(zero.data_ptr()) == 0
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"fyc_temporal_attention, f32 tensors, library ABI {h.abi_version}" + (f", other library ABI {other.fyc_version()}" if other else "") +
             f"; cold ring of operands, {a.rounds} rounds, median (min .. max) us per launch"]
    for clips, F, P, H, d, rope in SHAPES:
        rows, Cc = clips * F * P, H * d
        copy_bytes = rows * 4 * Cc * 4
        ring = max(2, -(-RING_BYTES // copy_bytes))
        g = torch.Generator(device=dev).manual_seed(1)
        qkv = [torch.randn(rows, 3 * Cc, device=dev, generator=g) for _ in range(ring)]
        outs = {k: [torch.empty(rows, Cc, device=dev) for _ in range(ring)] for k in ("exact", "split", "other")}
        kw = dict(clips=clips, frames=F, pixels=P, heads=H, d=d, scale=d ** -0.5)
        tables = tuple(t.to(dev) for t in rope_tables(d, F)) if rope else None
        if rope:
            kw["rope"] = tables

        def call_other(i):
            oa = OldTAttnArgs(qkv[i].data_ptr(), outs["other"][i].data_ptr(), clips, F, P, H, d, d ** -0.5, L.FYC_F32,
                              tables[0].data_ptr() if rope else None, tables[1].data_ptr() if rope else None)
            rc = other.fyc_temporal_attention(C.byref(oa), stream)
            assert rc == 0, rc
        variants = {"exact": (lambda i: h.temporal_attention(qkv[i], outs["exact"][i], products="exact", **kw)) if has_split else
                             (lambda i: h.temporal_attention(qkv[i], outs["exact"][i], **kw))}
        if other is not None:
            variants["other"] = call_other
        if has_split:
            variants["split"] = lambda i: h.temporal_attention(qkv[i], outs["split"][i], products="split", **kw)
        times = {k: [] for k in variants}
        for fn in variants.values():      # warm-up: code objects, LDS attributes
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
        tag = f"clips={clips} F={F:2d} P={P:4d} H={H} d={d:3d}{' RoPE' if rope else '     '}"
        label = {"exact": "exact", "other": "exact, other library", "split": "split"}
        for name, t in times.items():
            med = statistics.median(t)
            lines.append(f"{tag} {label[name]:21s}: {med:9.1f} ({min(t):.1f} .. {max(t):.1f}) us   {copy_bytes / med / 1e6:.3f} TB/s of q|k|v|o   (ring of {ring})")
        if "other" in variants:
            same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(outs["exact"], outs["other"]))
            lines.append(f"{tag} exact output of the two libraries bit-identical: {same}")
        if has_split:
            ref = "other" if "other" in variants else "exact"
            ex, sp = outs["exact"][0].double(), outs["split"][0].double()
            lines.append(f"{tag} split vs exact rel-L2 {((sp - ex).norm() / ex.norm()).item():.2e};  speed-up over {label[ref]}: "
                         f"{statistics.median(times[ref]) / statistics.median(times['split']):.1f} x  (slowest split round {max(times['split']):.1f} us, "
                         f"fastest {label[ref]} round {min(times[ref]):.1f} us)")
        del qkv, outs
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
