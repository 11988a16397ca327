"""Measurements behind profiles/pndm.txt (one MI355X).  bench.py is the yardstick of the default DDIM loop and cannot select a scheduler, so this wrapper starts its
main() with the sampler it constructs replaced:

  python tools/pndm_step_bench.py clip --mode plms [bench.py arguments]      bench.py's timed loop with PNDMSampler (the shipped betas, v_prediction, steps_offset 1) at
                                                                             bench.py's step count: n + 1 UNet evaluations per clip in PLMS mode, n + 9 in Runge-Kutta
                                                                             mode (--mode prk); --mode ddim runs bench.py's own sampler from the same entry
  python tools/pndm_step_bench.py kernel [--launches 50]                     fyc_cfg_pndm_step in its four shapes of use - PLMS step 0 (sample_out + hist_out), PLMS
                                                                             counter == 1 (sample_in, order 2), PLMS order 4 with hist_out, a Runge-Kutta accumulate
                                                                             (sample_in, acc_in == acc_out) - and, as the yardstick, fyc_cfg_sigma_step order 4 with
                                                                             hist_out, back to back on the benchmarked clip's shape (B 1, F 16, HW 4096, 4 latent
                                                                             channels; predictions in the UNet's 8-element rows, CFG on, bf16): device-event times
                                                                             per launch and the bytes each launch must move
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from followyourclick_amd.engine import PNDMConfig             # noqa: E402
from followyourclick_amd.engine.sampler import PNDMSampler    # noqa: E402

PNDM = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", prediction_type="v_prediction", steps_offset=1)


def clip(mode, rest):
    import bench
    if mode != "ddim":
        bench.DDIMSampler = lambda eng, _ddim: PNDMSampler(eng, PNDMConfig(skip_prk_steps=mode == "plms", **PNDM))
    return bench.main(rest)


def kernel(launches):
    from followyourclick_amd import ops
    hip, dev = ops.get(), "cuda:0"
    B, F, HW, CL, ld = 1, 16, 4096, 4, 8
    g = torch.Generator().manual_seed(0)
    rows, n = B * F * HW, B * CL * F * HW
    pred = torch.randn(2 * rows, ld, generator=g).to(torch.bfloat16).to(dev)
    lat0 = torch.randn(B, CL, F, HW, generator=g).to(dev)
    lat = lat0.clone()
    hist = [torch.randn(B, CL, F, HW, generator=g).to(dev) for _ in range(4)]
    sample, acc0 = torch.randn(B, CL, F, HW, generator=g).to(dev), torch.randn(B, CL, F, HW, generator=g).to(dev)
    acc = acc0.clone()
    coef = torch.tensor([1.1521, -1.2198, 1.3085, -0.8206, 0.1996, 1 / 3], device=dev)
    sigma_coef = torch.tensor([0.35, 0.37, 1.0, -1.31, 1.47, -0.93, 0.22, 0.71], device=dev)
    kw = dict(B=B, F=F, HW=HW, c_latent=CL, ld=ld, cfg=True, guidance=8.0)
    # bytes a launch must move: both halves of the predictions' latent channels (whole 16-byte rows are fetched: ld elements), per f32 latent-shaped buffer read or
    # written one latent tensor
    pb, lb = 2 * rows * ld * 2, n * 4
    calls = {
        "cfg_sigma_step order 4 + hist_out (yardstick)": (lambda: hip.cfg_sigma_step(pred, lat, sigma_coef, order=4, hist_out=hist[0], hist_1=hist[1], hist_2=hist[2],
                                                                                     hist_3=hist[3], **kw), pb + 6 * lb),
        "cfg_pndm_step PLMS step 0 (sample_out, hist_out)": (lambda: hip.cfg_pndm_step(pred, lat, coef, order=1, sample_out=sample, hist_out=hist[0], **kw), pb + 4 * lb),
        "cfg_pndm_step PLMS counter 1 (sample_in, order 2)": (lambda: hip.cfg_pndm_step(pred, lat, coef, order=2, sample_in=sample, hist_1=hist[1], **kw), pb + 3 * lb),
        "cfg_pndm_step PLMS order 4 + hist_out": (lambda: hip.cfg_pndm_step(pred, lat, coef, order=4, hist_out=hist[0], hist_1=hist[1], hist_2=hist[2], hist_3=hist[3],
                                                                            **kw), pb + 6 * lb),
        "cfg_pndm_step PRK accumulate (sample_in, acc in place)": (lambda: hip.cfg_pndm_step(pred, lat, coef, order=1, sample_in=sample, acc_in=acc, acc_out=acc, **kw),
                                                                   pb + 4 * lb),
    }
    for name, (fn, nbytes) in calls.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
        for a, b in ev:
            lat.copy_(lat0)            # the in-place updates of repeated launches must not run the latents or the accumulator off to inf (outside the timed pair)
            acc.copy_(acc0)
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        us = sorted(1000.0 * a.elapsed_time(b) for a, b in ev)
        med = us[len(us) // 2]
        print(f"{name:56s} {launches} launches, device events: median {med:7.1f} us, min {us[0]:7.1f} us, max {us[-1]:7.1f} us; {nbytes / 1e6:6.2f} MB "
              f"-> {nbytes / med / 1e3:7.1f} GB/s at the median")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode_", required=True)
    c = sub.add_parser("clip")
    c.add_argument("--mode", choices=["ddim", "plms", "prk"], required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--launches", type=int, default=50)
    args, rest = ap.parse_known_args()
    if args.mode_ == "clip":
        clip(args.mode, rest)
    else:
        kernel(args.launches)
