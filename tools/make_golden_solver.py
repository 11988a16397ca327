"""Golden vectors of the DPM-Solver multistep scheduler, from the REAL reference class (build container only; needs the reference tree that
oracle/refshim.py resolves).

Run:  python tools/make_golden_solver.py

Writes tests/golden/dpm_solver.npz (the plain betas) and tests/golden/dpm_solver_zero_snr.npz (the zero-terminal-SNR betas, handed to the reference as
trained_betas; dpmsolver++ with v_prediction / sample only - everything else is NaN there): two files, because one would pass the size limit of a committed file.
  alpha_t, sigma_t, lambda_t      the reference's three f32 tables
  timesteps_n<n>                  set_timesteps(n) for n = 4, 10, 14, 15, 25
  orders_o<solver_order>_n<n>     which update the reference's step() called at every step (1 / 2 / 3), recorded by wrapping its three update methods
  <case key>                      [n, 2, 4, 3, 7] f32: prev_sample of every step (tests/solver_spec.py::golden_cases, case_key)
Inputs are not stored: tests/solver_spec.py::case_inputs draws the initial latents and one model output per step from a generator seeded by the case's name.  Every step is
taken from the reference's own previous output.  A first-order solver never reads solver_type: its heun run is checked to be the midpoint run's bits and stored once."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import solver_spec as SP                                                     # noqa: E402
from followyourclick_amd.engine.scheduler import rescale_zero_terminal_snr   # noqa: E402
from oracle import refshim                                                   # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
PLAN_COUNTS = (4, 10, 14, 15, 25)


def betas_kwargs(name):
    if name == "plain":
        return dict(SP.BETAS)
    b = SP.BETAS
    betas = rescale_zero_terminal_snr(torch.linspace(b["beta_start"], b["beta_end"], b["num_train_timesteps"], dtype=torch.float32))
    return dict(num_train_timesteps=b["num_train_timesteps"], trained_betas=betas.tolist())


def recorded_orders(sched, n):
    """the update step() calls at every step of an n-step run on zeros"""
    calls = []
    for order, name in ((1, "dpm_solver_first_order_update"), (2, "multistep_dpm_solver_second_order_update"), (3, "multistep_dpm_solver_third_order_update")):
        inner = getattr(sched, name)
        setattr(sched, name, lambda *a, _o=order, _f=inner, **k: (calls.append(_o), _f(*a, **k))[1])
    sched.set_timesteps(n)
    x = torch.ones(1, 1)
    for t in sched.timesteps:
        x = sched.step(torch.ones(1, 1), t, x).prev_sample
    return np.array(calls, dtype=np.int64)


def main():
    refshim.install()
    from diffusers.schedulers.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler
    files = {"plain": {}, "zsnr": {}}
    for name, out in files.items():
        s = DPMSolverMultistepScheduler(**betas_kwargs(name))
        out.update(alpha_t=s.alpha_t.numpy(), sigma_t=s.sigma_t.numpy(), lambda_t=s.lambda_t.numpy())
        for n in PLAN_COUNTS:
            s.set_timesteps(n)
            out[f"timesteps_n{n}"] = s.timesteps.numpy().astype(np.int64)
            for order in SP.ORDERS:
                out[f"orders_o{order}_n{n}"] = recorded_orders(DPMSolverMultistepScheduler(solver_order=order, **betas_kwargs(name)), n)
    for case in SP.golden_cases():
        sched = DPMSolverMultistepScheduler(**SP.family(case), **betas_kwargs(case.betas))
        sched.set_timesteps(case.n)
        x, vs = SP.case_inputs(case)
        prev = []
        for i, t in enumerate(sched.timesteps):
            x = sched.step(vs[i], t, x).prev_sample
            prev.append(x.numpy().copy())
        prev = np.stack(prev)
        assert np.isfinite(prev).all(), case
        out, key = files[case.betas], SP.case_key(case)
        if key in out:          # the first-order heun run (same array name, so the same inputs): stored once, because it IS the midpoint run
            assert np.array_equal(out[key], prev), case
            continue
        out[key] = prev
    for name, fname in (("plain", "dpm_solver.npz"), ("zsnr", "dpm_solver_zero_snr.npz")):
        path = os.path.join(OUT, fname)
        np.savez_compressed(path, **files[name])
        print(f"{path}: {len(files[name])} arrays, {os.path.getsize(path) >> 10} KiB")


if __name__ == "__main__":
    main()
