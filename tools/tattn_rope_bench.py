"""fyc_temporal_attention timing: NULL tables against RoPE, clips of 16 / 48 / 64 frames, optionally against another build of the library.

  python tools/tattn_rope_bench.py [--other-lib PATH] [--rounds 7] [--iters 40] [--out FILE]

Shape: BASELINE.json configs[1] level 0 (2 clips, 4096 pixels, 8 heads x 40) in bf16.  All variants run in ONE process and alternate
inside every round, so that they share whatever else the machine is doing; each figure is the median over the rounds of the mean
time of `iters` back-to-back launches between two device events, with the min .. max of the rounds as the spread.  --other-lib: a
libfyc_hip.so built from another commit (FYC_BUILD_LIB=... python -m followyourclick_amd._build), called through the argument struct of
ABI 302 - the prefix of today's - for the NULL-table case only.  Outputs of the two libraries are compared bit for bit."""
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


class OldTAttnArgs(C.Structure):      # fyc_tattn_args before rope_cos / rope_sin were appended
    _fields_ = L.TAttnArgs._fields_[:9]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-lib")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    h = ops.get()
    h.ensure_init(dev)
    other = None
    if a.other_lib:
        other = C.CDLL(os.path.abspath(a.other_lib))
        other.fyc_version.restype = C.c_int
        other.fyc_init.argtypes = [C.c_void_p]
        other.fyc_temporal_attention.argtypes = [C.POINTER(OldTAttnArgs), C.c_void_p]
        zero = torch.zeros(4096, dtype=torch.uint8, device=dev)
        assert other.fyc_init(zero.data_ptr()) == 0
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"fyc_temporal_attention, bf16, 2 clips x 4096 pixels x 8 heads x 40; {a.rounds} rounds x {a.iters} launches, median (min .. max) us per launch"]
    clips, P, H, d = 2, 4096, 8, 40
    for F in (16, 48, 64):
        qkv = torch.randn(clips * F * P, 3 * H * d, device=dev).to(torch.bfloat16)
        outs = {k: torch.empty(clips * F * P, H * d, dtype=torch.bfloat16, device=dev) for k in ("null", "rope", "other")}
        kw = dict(clips=clips, frames=F, pixels=P, heads=H, d=d, scale=d ** -0.5)
        tables = tuple(t.to(dev) for t in rope_tables(d, F))
        oa = OldTAttnArgs(qkv.data_ptr(), outs["other"].data_ptr(), clips, F, P, H, d, d ** -0.5, L.FYC_BF16)
        variants = {"null": lambda: h.temporal_attention(qkv, outs["null"], **kw),
                    "rope": lambda: h.temporal_attention(qkv, outs["rope"], rope=tables, **kw)}
        if other is not None and F <= 32:
            def call_other():
                rc = other.fyc_temporal_attention(C.byref(oa), stream)
                assert rc == 0, rc
            variants["other"] = call_other
        times = {k: [] for k in variants}
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for name, fn in variants.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(a.iters):
                    fn()
                e.record()
                torch.cuda.synchronize()
                times[name].append(s.elapsed_time(e) / a.iters * 1e3)
        nbytes = 4.0 * clips * F * P * H * d * 2          # q, k, v read once, o written once
        for name, t in times.items():
            med = statistics.median(t)
            label = {"null": "NULL tables", "rope": "RoPE", "other": f"NULL tables, other library (ABI {other.fyc_version() if other else 0})"}[name]
            lines.append(f"F={F:2d} {label}: {med:8.1f} ({min(t):.1f} .. {max(t):.1f}) us   {nbytes / med / 1e6:.2f} TB/s of q|k|v|o")
        if "other" in variants:
            same = torch.equal(outs["null"].view(torch.int16), outs["other"].view(torch.int16))
            lines.append(f"F={F:2d} NULL-table output of the two libraries bit-identical: {same}")
        del qkv, outs
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
