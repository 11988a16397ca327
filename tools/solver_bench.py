"""Measurements behind profiles/dpm_solver.txt (one MI355X).  bench.py is the yardstick of the default DDIM loop and cannot select a scheduler, so this wrapper
starts its main() with the sampler it constructs replaced:

  python tools/solver_bench.py clip --solver-steps 10 [bench.py arguments]    bench.py's timed loop with SolverSampler (DPM-Solver++(2M), the shipped zero-SNR betas,
                                                                            v_prediction) at that many steps; the JSON line's "ddim_steps" is the solver's step count
  python tools/solver_bench.py kernel [--launches 20]                         fyc_cfg_ddim_step and fyc_cfg_solver_step (orders 1-3) back to back on the benchmarked
                                                                            clip's shape (B 1, F 16, HW 4096, 4 latent channels in the UNet's 8-element rows, bf16):
                                                                            run it under `rocprofv3 --kernel-trace --stats` for the per-launch times; on its own it
                                                                            prints device-event times of the same launches
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from followyourclick_amd.engine import SolverConfig            # noqa: E402
from followyourclick_amd.engine.sampler import SolverSampler   # noqa: E402

SOLVER = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", prediction_type="v_prediction", rescale_betas_zero_snr=True, solver_order=2)


def clip(steps, rest):
    import bench
    bench.DDIMSampler = lambda eng, _ddim: SolverSampler(eng, SolverConfig(**SOLVER))
    return bench.main(["--ddim-steps", str(steps), *rest])


def kernel(launches):
    from followyourclick_amd import ops
    hip, dev = ops.get(), "cuda:0"
    B, F, HW, CL, ld = 1, 16, 4096, 4, 8
    g = torch.Generator().manual_seed(0)
    pred = torch.randn(2 * B * F * HW, ld, generator=g).to(torch.bfloat16).to(dev)
    lat = torch.randn(B, CL, F, HW, generator=g).to(dev)
    hist = [torch.randn(B, CL, F, HW, generator=g).to(dev) for _ in range(3)]
    ddim_coef = torch.tensor([0.6, 0.8, 0.8, 0.6], device=dev)
    coef = torch.tensor([0.6, -0.8, 0.83, 0.47, -0.21, 0.06, 0.0, 0.0], device=dev)
    kw = dict(B=B, F=F, HW=HW, c_latent=CL, ld=ld, cfg=True, guidance=8.0)
    calls = {"cfg_ddim_step": lambda: hip.cfg_ddim_step(pred, lat, ddim_coef, pred_type=1, clip_sample=False, **kw)}
    for order in (1, 2, 3):
        calls[f"cfg_solver_step order {order}"] = lambda o=order: hip.cfg_solver_step(pred, lat, coef, hist_out=hist[0], hist_1=hist[1], hist_2=hist[2], order=o, **kw)
    for name, fn in calls.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        us = sorted(1000.0 * a.elapsed_time(b) for a, b in ev)
        lat.copy_(hist[1])            # the in-place update of these repeated launches must not run the latents off to inf
        print(f"{name:28s} {launches} launches, device events: median {us[len(us) // 2]:.1f} us, min {us[0]:.1f} us, max {us[-1]:.1f} us")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    c = sub.add_parser("clip")
    c.add_argument("--solver-steps", type=int, required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--launches", type=int, default=20)
    args, rest = ap.parse_known_args()
    if args.mode == "clip":
        clip(args.solver_steps, rest)
    else:
        kernel(args.launches)
