"""Golden vectors of the PNDM scheduler, PLMS mode (skip_prk_steps) and Runge-Kutta mode, from the REAL reference class (build container only; needs the reference
tree that oracle/refshim.py resolves).

Run:  python tools/make_golden_pndm.py

Writes tests/golden/pndm.npz:
  <betas>/<mode>/timesteps_n<n>, prk_timesteps_n<n>, plms_timesteps_n<n>     set_timesteps(n) for n = 4, 10, 25 (int64), steps_offset = 1
  <case key>                                                                 [n + 1 or n + 9, 2, 4, 3, 7] f32: prev_sample of every evaluation
                                                                             (tests/pndm_spec.py::golden_cases, case_key)
betas: linear, scaled_linear, zsnr; mode: plms, prk.  zsnr is the zero-terminal-SNR table: the reference class gets the rescaled betas as trained_betas; with its
leading spacing no schedule touches timestep 999, where formula (9) would divide by alphas_cumprod = 0.  Inputs are not stored: tests/pndm_spec.py::case_inputs draws
the initial latents and one model output per evaluation from a generator seeded by the case's name.  Every evaluation is taken from the reference's own previous
output, and every stored result is checked to be finite and to lie inside the specification's bound.

Writes tests/golden/pipeline_tiny_pndm.npz: one run per mode of the real AnimationPipeline on the tiny model of oracle/make_golden.py (same weights seed, inputs,
5 steps - 6 evaluations in PLMS mode, 14 in Runge-Kutta mode, the smallest schedule that reaches a PLMS step behind the twelve Runge-Kutta ones -, CFG 8, mask +
first-frame concat, fps / flow; linear betas, v_prediction): the latents after every evaluation (taken at the scheduler's step(): the reference's loop holds its
callback back over the len(timesteps) - num_inference_steps warm-up evaluations) and the indices its callback was called with."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pndm_spec as SP                                                       # noqa: E402
from followyourclick_amd.engine.scheduler import rescale_zero_terminal_snr   # noqa: E402
from oracle import functional as Fn                                          # noqa: E402
from oracle import make_golden as MG                                         # noqa: E402
from oracle import refshim, stubs                                            # noqa: E402
from oracle import weights as W                                              # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
PIPE_BETAS = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", prediction_type="v_prediction")


def make(betas, mode, **kw):
    """the reference scheduler of a beta set and mode; zsnr: the rescaled betas as trained_betas"""
    from diffusers.schedulers.scheduling_pndm import PNDMScheduler
    b = SP.BETA_SETS[betas]
    kw = dict(skip_prk_steps=mode == "plms", steps_offset=SP.STEPS_OFFSET, **kw)
    if betas != "zsnr":
        return PNDMScheduler(**b, **kw)
    tb = rescale_zero_terminal_snr(torch.linspace(b["beta_start"], b["beta_end"], b["num_train_timesteps"], dtype=torch.float32))
    return PNDMScheduler(num_train_timesteps=b["num_train_timesteps"], trained_betas=tb.tolist(), **kw)


def run_case(case, out):
    sched = make(case.betas, case.mode, prediction_type=case.prediction_type)
    sched.set_timesteps(case.n)
    assert len(sched.timesteps) == SP.evaluations(case), case
    x, vs = SP.case_inputs(case)
    prev = []
    for i, t in enumerate(sched.timesteps):
        x = sched.step(vs[i], t, sched.scale_model_input(x, t)).prev_sample
        prev.append(x.numpy().copy())
    prev = np.stack(prev)
    assert np.isfinite(prev).all() and prev.dtype == np.float32, case
    # the reference's own f32 results against the specification
    xs = SP.case_samples(case, torch.from_numpy(prev))
    worst = 0.0
    for i, ev in enumerate(SP.schedule(case.mode, case.n, offset=SP.STEPS_OFFSET)):
        ref, S = SP.schedule_eval(sched.alphas_cumprod, sched.final_alpha_cumprod, case.prediction_type, ev, xs, vs)
        worst = max(worst, SP.inside(torch.from_numpy(prev[i]), ref, SP.gamma(SP.K_REFERENCE) * S, f"{case} evaluation {i}"))
    out[SP.case_key(case)] = prev
    return worst


def pipeline_runs():
    from animatediff.pipelines.pipeline_animation import AnimationPipeline
    from diffusers.schedulers.scheduling_pndm import PNDMScheduler
    cfg = Fn.tiny_unet_config()
    unet = MG.ref_unet(cfg).eval()
    unet.load_state_dict(W.make_weights(W.unet_state_shapes(cfg), seed=0), strict=True)
    vcfg = Fn.VAEConfig(block_out_channels=(64, 128, 128, 128))
    vae = MG.ref_vae(vcfg).eval()
    vae.load_state_dict(W.make_weights(W.vae_decoder_state_shapes(vcfg), seed=3), strict=False)
    inp = W.seeded_inputs(cfg, 1, 4, 8, 8, seed=21)
    out = dict(latents=inp["latents"].numpy(), first_image_latents=inp["first_image_latents"].numpy(), first_images_mask=inp["first_images_mask"].numpy(),
               unet_weight_seed=np.int64(0), input_seed=np.int64(21))
    for mode in SP.MODES:
        pipe = AnimationPipeline(vae=vae, text_encoder=stubs.StubTextEncoder(cfg.cross_attention_dim), tokenizer=stubs.FakeTokenizer(), unet=unet,
                                 scheduler=PNDMScheduler(skip_prk_steps=mode == "plms", steps_offset=1, **PIPE_BETAS))
        traj, seen, called = [], [], []
        inner = pipe.scheduler.step

        def step(model_output, timestep, sample, **kw):          # every evaluation's result: the reference's loop holds its callback back over the warm-up evaluations
            o = inner(model_output, timestep, sample, **kw)
            traj.append(o.prev_sample.clone())
            seen.append(int(timestep))
            return o
        pipe.scheduler.step = step
        pipe("a corgi waving its tail", video_length=4, height=64, width=64, num_inference_steps=5, guidance_scale=8.0, negative_prompt="blurry",
             latents=inp["latents"].clone(), first_image_latents=inp["first_image_latents"], first_images_mask=inp["first_images_mask"],
             use_first_frame_mask_condition_concat=True, use_fps_condition=True, fps_tensor=torch.tensor([2]), flow_control=torch.tensor([4]),
             callback=lambda i, t, l: called.append(i), callback_steps=1)
        out[f"trajectory_{mode}"], out[f"timesteps_{mode}"] = torch.stack(traj).numpy(), np.array(seen, dtype=np.int64)
        out[f"callback_indices_{mode}"] = np.array(called, dtype=np.int64)          # (the evaluations behind the warm-up ones: 1 .. 5 and 9 .. 13)
        assert np.isfinite(out[f"trajectory_{mode}"]).all() and len(traj) == (6 if mode == "plms" else 14), mode
        if "text_embeddings" not in out:
            with torch.no_grad():
                out["text_embeddings"] = pipe._encode_prompt(["a corgi waving its tail"], "cpu", 1, True, ["blurry"]).numpy()
    return out


def main():
    refshim.install()
    out, worst = {}, 0.0
    for betas in SP.BETA_SETS:
        for mode in SP.MODES:
            s = make(betas, mode)
            for n in SP.STEP_COUNTS:
                s.set_timesteps(n)
                out[f"{betas}/{mode}/timesteps_n{n}"] = s.timesteps.numpy().copy()
                out[f"{betas}/{mode}/prk_timesteps_n{n}"] = np.asarray(s.prk_timesteps).astype(np.int64)
                out[f"{betas}/{mode}/plms_timesteps_n{n}"] = np.asarray(s.plms_timesteps).astype(np.int64)
    cases = SP.golden_cases()
    for case in cases:
        worst = max(worst, run_case(case, out))
    assert sum(SP.case_key(c) in out for c in cases) == len(cases) == 36
    print(f"{len(cases)} cases: the reference's worst element at {worst:.3f} x its bound (K = {SP.K_REFERENCE})")
    for fname, arrays in (("pndm.npz", out), ("pipeline_tiny_pndm.npz", pipeline_runs())):
        path = os.path.join(OUT, fname)
        np.savez_compressed(path, **arrays)
        print(f"{path}: {len(arrays)} arrays, {os.path.getsize(path) >> 10} KiB")


if __name__ == "__main__":
    main()
