"""Measurements behind profiles/sigma_samplers.txt (one MI355X).  bench.py is the yardstick of the default DDIM loop and cannot select a scheduler, so this wrapper
starts its main() with the sampler it constructs replaced:

  python tools/sigma_step_bench.py clip --kind euler [bench.py arguments]     bench.py's timed loop with SigmaSampler (the shipped zero-SNR betas, v_prediction) at
                                                                              bench.py's step count; --kind ddim runs bench.py's own sampler from the same entry
  python tools/sigma_step_bench.py kernel [--launches 50]                     fyc_cfg_ddim_step, fyc_cfg_sigma_step (order 1 as Euler calls it - no history stored, no
                                                                              noise -, order 1 with noise, order 4 with hist_out), fyc_unet_input and
                                                                              fyc_unet_input_scaled back to back on the benchmarked clip's shape (B 1, F 16, HW 4096,
                                                                              4 latent channels; predictions in the UNet's 8-element rows, 16-channel input rows,
                                                                              CFG on, bf16): device-event times per launch and the bytes each launch must move;
                                                                              under `rocprofv3 --kernel-trace --stats` the same launches give the kernels' own times
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from followyourclick_amd.engine import SigmaConfig             # noqa: E402
from followyourclick_amd.engine.sampler import SigmaSampler    # noqa: E402

SIGMA = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", prediction_type="v_prediction", rescale_betas_zero_snr=True)


def clip(kind, rest):
    import bench
    if kind != "ddim":
        bench.DDIMSampler = lambda eng, _ddim: SigmaSampler(eng, SigmaConfig(kind=kind, **SIGMA))
    return bench.main(rest)


def kernel(launches):
    from followyourclick_amd import ops
    hip, dev = ops.get(), "cuda:0"
    B, F, HW, CL, ld, cp = 1, 16, 4096, 4, 8, 16
    g = torch.Generator().manual_seed(0)
    rows, n = B * F * HW, B * CL * F * HW
    pred = torch.randn(2 * rows, ld, generator=g).to(torch.bfloat16).to(dev)
    lat0 = torch.randn(B, CL, F, HW, generator=g).to(dev)
    lat = lat0.clone()
    hist = [torch.randn(B, CL, F, HW, generator=g).to(dev) for _ in range(4)]
    noise = torch.randn(B, CL, F, HW, generator=g).to(dev)
    first, mask = torch.randn(B, CL, HW, generator=g).to(dev), torch.rand(B, 1, HW, generator=g).to(dev)
    x = torch.empty(2 * rows, cp, dtype=torch.bfloat16, device=dev)
    ddim_coef = torch.tensor([0.6, 0.8, 0.8, 0.6], device=dev)
    coef = torch.tensor([0.35, 0.37, 1.0, -1.31, 1.47, -0.93, 0.22, 0.71], device=dev)
    kw = dict(B=B, F=F, HW=HW, c_latent=CL, ld=ld, cfg=True, guidance=8.0)
    ikw = dict(B=B, F=F, HW=HW, c_latent=CL, c_pad=cp, cfg_dup=2, mask_frames=1)
    # bytes a launch must move: both halves of the predictions' latent channels (whole 16-byte rows are fetched: ld elements), the latents in and out, and
    # per history / noise buffer one f32 latent tensor; the input builds read the latents, mask and first frame and write cfg_dup rows of c_pad elements
    pb, lb = 2 * rows * ld * 2, n * 4
    calls = {
        "cfg_ddim_step": (lambda: hip.cfg_ddim_step(pred, lat, ddim_coef, pred_type=1, clip_sample=False, **kw), pb + 2 * lb),
        "cfg_sigma_step order 1 (Euler)": (lambda: hip.cfg_sigma_step(pred, lat, coef, order=1, **kw), pb + 2 * lb),
        "cfg_sigma_step order 1 + noise": (lambda: hip.cfg_sigma_step(pred, lat, coef, order=1, noise=noise, **kw), pb + 3 * lb),
        "cfg_sigma_step order 4 (LMS)": (lambda: hip.cfg_sigma_step(pred, lat, coef, order=4, hist_out=hist[0], hist_1=hist[1], hist_2=hist[2], hist_3=hist[3], **kw),
                                         pb + 6 * lb),
        "unet_input": (lambda: hip.unet_input(lat0, mask, first, x, **ikw), lb + 2 * rows * cp * 2),
        "unet_input_scaled": (lambda: hip.unet_input_scaled(lat0, mask, first, x, denom=5.413011074066162, scale_cond=True, **ikw), lb + 2 * rows * cp * 2),
    }
    for name, (fn, nbytes) in calls.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
        for a, b in ev:
            lat.copy_(lat0)            # the in-place update of repeated launches must not run the latents off to inf (outside the timed pair)
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        us = sorted(1000.0 * a.elapsed_time(b) for a, b in ev)
        med = us[len(us) // 2]
        print(f"{name:34s} {launches} launches, device events: median {med:7.1f} us, min {us[0]:7.1f} us, max {us[-1]:7.1f} us; {nbytes / 1e6:6.2f} MB "
              f"-> {nbytes / med / 1e3:7.1f} GB/s at the median")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    c = sub.add_parser("clip")
    c.add_argument("--kind", choices=["ddim", "euler", "euler_ancestral", "lms"], required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--launches", type=int, default=50)
    args, rest = ap.parse_known_args()
    if args.mode == "clip":
        clip(args.kind, rest)
    else:
        kernel(args.launches)
