"""Golden vectors of the sigma-space schedulers - Euler, Euler ancestral, LMS - from the REAL reference classes (build container only; needs the reference tree
that oracle/refshim.py resolves, and scipy for the reference's LMS quadrature).

Run:  python tools/make_golden_sigma.py

Writes tests/golden/sigma_samplers.npz:
  <betas>/<kind>/sigmas_n<n>, timesteps_n<n>     set_timesteps(n) of the three classes for n = 4, 10, 25 (f32 / f64)
  <betas>/<kind>/init_noise_sigma
  <betas>/lms_coeffs_n<n>                          [n, 4] f64: what the reference's get_lms_coefficient returned at every step (newest derivative first, 0 beyond the order)
  <case key>                                       [n, 2, 4, 3, 7] f32: prev_sample of every step (tests/sigma_spec.py::golden_cases, case_key)
betas: linear, scaled_linear, zsnr.  zsnr is the zero-terminal-SNR table: the reference class gets the rescaled betas as trained_betas and its instance's
alphas_cumprod[-1] is set to 2^-24 before set_timesteps (a change of data; init_noise_sigma is re-derived from the patched table by the constructor's own lines).
Inputs are not stored: tests/sigma_spec.py::case_inputs draws the initial latents, one model output and one noise tensor per step from a generator seeded by the
case's name; the ancestral class is handed that noise by wrapping torch.randn for the call.  Every step is taken from the reference's own previous output, and every
stored result is checked to lie inside the specification's bound.

Writes tests/golden/pipeline_tiny_sigma.npz: one run per kind of the real AnimationPipeline on the tiny model of oracle/make_golden.py (same weights seed, inputs,
5 steps, CFG 8, mask + first-frame concat, fps / flow; linear betas, v_prediction; generator seed 33 for the step noise): the per-step latents."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sigma_spec as SP                                                      # noqa: E402
from followyourclick_amd.engine.scheduler import rescale_zero_terminal_snr   # noqa: E402
from oracle import functional as Fn                                          # noqa: E402
from oracle import make_golden as MG                                         # noqa: E402
from oracle import refshim, stubs                                            # noqa: E402
from oracle import weights as W                                              # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
PIPE_BETAS = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", prediction_type="v_prediction")
PIPE_SEED = 33


def classes():
    from diffusers.schedulers.scheduling_euler_ancestral_discrete import EulerAncestralDiscreteScheduler
    from diffusers.schedulers.scheduling_euler_discrete import EulerDiscreteScheduler
    from diffusers.schedulers.scheduling_lms_discrete import LMSDiscreteScheduler
    return {"euler": EulerDiscreteScheduler, "euler_ancestral": EulerAncestralDiscreteScheduler, "lms": LMSDiscreteScheduler}


def make(cls, betas, **kw):
    """the reference scheduler of a beta set; zsnr: rescaled betas as trained_betas, the table's last entry set to 2^-24"""
    b = SP.BETA_SETS[betas]
    if betas != "zsnr":
        return cls(**b, **kw)
    tb = rescale_zero_terminal_snr(torch.linspace(b["beta_start"], b["beta_end"], b["num_train_timesteps"], dtype=torch.float32))
    s = cls(num_train_timesteps=b["num_train_timesteps"], trained_betas=tb.tolist(), **kw)
    s.alphas_cumprod[-1] = 2.0 ** -24
    sig = np.array(((1 - s.alphas_cumprod) / s.alphas_cumprod) ** 0.5)
    s.sigmas = torch.from_numpy(np.concatenate([sig[::-1], [0.0]]).astype(np.float32))
    s.init_noise_sigma = s.sigmas.max()
    return s


def run_case(cls, case, out):
    sched = make(cls, case.betas, prediction_type=case.prediction_type)
    sched.set_timesteps(case.n)
    x, vs, noise = SP.case_inputs(case)
    x = x * sched.init_noise_sigma
    coeffs = np.zeros((case.n, 4))
    if case.kind == "lms":
        inner, seen = sched.get_lms_coefficient, []
        sched.get_lms_coefficient = lambda order, t, cur: (seen.append((t, cur, inner(order, t, cur))), seen[-1][2])[1]
    prev, randn = [], torch.randn
    for i, t in enumerate(sched.timesteps):
        sched.scale_model_input(x, t)
        torch.randn = lambda *a, _i=i, **k: noise[_i].clone()              # the ancestral step's noise (Euler draws and drops its own)
        try:
            x = sched.step(vs[i], t, x).prev_sample
        finally:
            torch.randn = randn
        prev.append(x.numpy().copy())
    prev = np.stack(prev)
    assert np.isfinite(prev).all() and prev.dtype == np.float32, case
    if case.kind == "lms":
        for t, cur, c in seen:
            coeffs[t, cur] = c
        key = f"{case.betas}/lms_coeffs_n{case.n}"
        assert key not in out or np.array_equal(out[key], coeffs), case          # the coefficients depend on the sigmas alone
        out[key] = coeffs
    # the reference's own f32 results against the specification
    sig = sched.sigmas
    xs = SP.case_samples(case, torch.from_numpy(prev), sched.init_noise_sigma)
    worst = 0.0
    for i in range(case.n):
        o = min(i + 1, 4)
        ref, S = SP.schedule_step(case.kind, case.prediction_type, sig, i, xs, vs, noise=noise[i], lms_coeffs=coeffs[i, :o])
        worst = max(worst, SP.inside(torch.from_numpy(prev[i]), ref, SP.gamma(SP.K_REFERENCE) * S, f"{case} step {i}"))
    out[SP.case_key(case)] = prev
    return worst


def pipeline_runs():
    from animatediff.pipelines.pipeline_animation import AnimationPipeline
    cfg = Fn.tiny_unet_config()
    unet = MG.ref_unet(cfg).eval()
    unet.load_state_dict(W.make_weights(W.unet_state_shapes(cfg), seed=0), strict=True)
    vcfg = Fn.VAEConfig(block_out_channels=(64, 128, 128, 128))
    vae = MG.ref_vae(vcfg).eval()
    vae.load_state_dict(W.make_weights(W.vae_decoder_state_shapes(vcfg), seed=3), strict=False)
    inp = W.seeded_inputs(cfg, 1, 4, 8, 8, seed=21)
    out = dict(latents=inp["latents"].numpy(), first_image_latents=inp["first_image_latents"].numpy(), first_images_mask=inp["first_images_mask"].numpy(),
               unet_weight_seed=np.int64(0), input_seed=np.int64(21), generator_seed=np.int64(PIPE_SEED))
    for kind, cls in classes().items():
        pipe = AnimationPipeline(vae=vae, text_encoder=stubs.StubTextEncoder(cfg.cross_attention_dim), tokenizer=stubs.FakeTokenizer(), unet=unet,
                                 scheduler=cls(**PIPE_BETAS))
        traj = []
        pipe("a corgi waving its tail", video_length=4, height=64, width=64, num_inference_steps=5, guidance_scale=8.0, negative_prompt="blurry",
             latents=inp["latents"].clone(), first_image_latents=inp["first_image_latents"], first_images_mask=inp["first_images_mask"],
             use_first_frame_mask_condition_concat=True, use_fps_condition=True, fps_tensor=torch.tensor([2]), flow_control=torch.tensor([4]),
             generator=torch.Generator().manual_seed(PIPE_SEED), callback=lambda i, t, l: traj.append(l.clone()), callback_steps=1)
        out[f"trajectory_{kind}"] = torch.stack(traj).numpy()
        assert np.isfinite(out[f"trajectory_{kind}"]).all(), kind
        if "text_embeddings" not in out:
            with torch.no_grad():
                out["text_embeddings"] = pipe._encode_prompt(["a corgi waving its tail"], "cpu", 1, True, ["blurry"]).numpy()
            out["init_noise_sigma"] = np.float32(pipe.scheduler.init_noise_sigma)
    return out


def main():
    refshim.install()
    out, worst = {}, 0.0
    for betas in SP.BETA_SETS:
        for kind, cls in classes().items():
            s = make(cls, betas)
            out[f"{betas}/{kind}/init_noise_sigma"] = np.float32(s.init_noise_sigma)
            for n in SP.STEP_COUNTS:
                s.set_timesteps(n)
                out[f"{betas}/{kind}/sigmas_n{n}"], out[f"{betas}/{kind}/timesteps_n{n}"] = s.sigmas.numpy().copy(), s.timesteps.numpy().copy()
    cases = SP.golden_cases()
    for case in cases:
        worst = max(worst, run_case(classes()[case.kind], case, out))
    assert sum(SP.case_key(c) in out for c in cases) == len(cases) == 54
    print(f"{len(cases)} cases: the reference's worst element at {worst:.3f} x its bound (K = {SP.K_REFERENCE})")
    for fname, arrays in (("sigma_samplers.npz", out), ("pipeline_tiny_sigma.npz", pipeline_runs())):
        path = os.path.join(OUT, fname)
        np.savez_compressed(path, **arrays)
        print(f"{path}: {len(arrays)} arrays, {os.path.getsize(path) >> 10} KiB")


if __name__ == "__main__":
    main()
