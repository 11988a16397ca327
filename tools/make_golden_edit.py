"""Golden runs of the image-editing pipelines from the REAL reference classes (build container only; needs the reference tree that oracle/refshim.py
resolves): StableDiffusionImg2ImgPipeline, StableDiffusionInpaintPipeline and StableDiffusionInpaintPipelineLegacy of the vendored diffusers, on the tiny
2-D UNet / tiny VAE of oracle/make_golden_2d.py.

Run:  python tools/make_golden_edit.py

Writes tests/golden/pipeline_tiny_edit.npz.  Cases: tests/edit_spec.py::CASES - img2img at strength 0.6 of 5 steps (t_start = 2) with six schedulers, DDIM at
strength 1.0 and DDIM with eta = 0.5; the 9-channel inpainting pipeline and the legacy inpainting loop with DDIM, PNDM-PLMS and Euler.  64 x 64 images, CFG 8, a
negative prompt, a seeded CPU generator per call.  Per case <key> = edit_spec.case_key(case):
  <key>/noise_<k>        every tensor torch.randn returned during the call, in the order drawn
  <key>/trajectory       the latents after every evaluation (for the legacy loop: after its blend), [evaluations, 1, 4, 8, 8]
  <key>/timesteps        the timestep of every evaluation
  <key>/callbacks        the indices the caller's callback was called with
  <key>/images           the final images, (1, 64, 64, 3) f32 in [0, 1]
and once: image (1, 3, 64, 64) f32 in [-1, 1] and mask (1, 1, 64, 64) f32 in [0, 1] (img2img, inpaint), legacy_image (64, 64, 3) uint8 and legacy_mask (64, 64)
uint8 (handed to the legacy pipeline as PIL images), text_embeddings, the weight seeds.  Weights are re-derived from seeds by oracle/weights.py::make_weights.

While writing, the reference's own f32 results of the two formula kernels are checked against tests/edit_spec.py: the start latents of every img2img / legacy
case against posterior_latents (from the VAE moments and the two noises the call drew), the masked-image latents of every inpaint case, and every blend of every
legacy case against renoise_blend - the bounds are not tighter than the reference itself.  The inpaint cases' mask and masked image are compared bit for bit with
inpaint_prepare."""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import edit_spec as ES                                                       # noqa: E402
from followyourclick_amd.engine import DDIMConfig, PNDMConfig, SigmaConfig, SolverConfig      # noqa: E402
from followyourclick_amd.engine.scheduler import DDIMTables, PNDMTables, SigmaTables, SolverTables      # noqa: E402
from oracle import functional as Fn                                          # noqa: E402
from oracle import make_golden as MG                                         # noqa: E402
from oracle import make_golden_2d as MG2                                     # noqa: E402
from oracle import stubs                                                     # noqa: E402
from oracle import weights as W                                              # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SIGMA_KIND = {"euler": "euler", "euler_a": "euler_ancestral", "lms": "lms"}


def cfg_9ch():
    return Fn.tiny_unet_config(use_motion_module=False, use_fps_condition=False, use_first_frame_mask_condition_concat=True)


def vae_config():
    return Fn.VAEConfig(block_out_channels=(64, 128, 128, 128))


def vae_weights():
    vcfg = vae_config()
    sd = W.make_weights(W.vae_decoder_state_shapes(vcfg), seed=ES.VAE_SEED)
    sd.update(W.make_weights(W.vae_encoder_state_shapes(vcfg), seed=ES.VAE_SEED + 1))
    return sd


def inputs():
    """the seeded inputs of all cases"""
    g = torch.Generator().manual_seed(ES.INPUT_SEED)
    image = torch.rand(1, 3, 64, 64, generator=g) * 2.0 - 1.0
    mask = torch.zeros(1, 1, 64, 64)
    mask[:, :, 16:48, 8:40] = 1.0                                             # a square to repaint ...
    mask[:, :, 24:32, 40:56] = torch.rand(1, 1, 8, 16, generator=g)           # ... and a band of fractional values the binarisation decides
    legacy_image = torch.randint(0, 256, (64, 64, 3), generator=g, dtype=torch.uint8).numpy()
    legacy_mask = np.zeros((64, 64), np.uint8)
    legacy_mask[16:48, 8:40] = 255
    legacy_mask[24:32, 40:56] = torch.randint(0, 256, (8, 16), generator=g, dtype=torch.uint8).numpy()
    return dict(image=image, mask=mask, legacy_image=legacy_image, legacy_mask=legacy_mask)


def engine_tables(name):
    """the engine's table class of a scheduler of edit_spec.SCHEDULERS: its add_noise_coefficients are what the kernels get"""
    kw = dict(ES.SCHEDULERS[name][1])
    if name == "ddim":
        return DDIMTables(DDIMConfig(**kw))
    if name == "dpmpp2":
        return SolverTables(SolverConfig(**kw))
    if name == "plms":
        return PNDMTables(PNDMConfig(**kw))
    return SigmaTables(SigmaConfig(kind=SIGMA_KIND[name], **kw))


def run_case(case, pipes, schedulers, inp, out):
    import PIL.Image
    key = ES.case_key(case)
    cls_name, kw = ES.SCHEDULERS[case.scheduler]
    sched = schedulers[cls_name](**kw)
    pipe = pipes[case.pipeline](scheduler=sched)
    drawn, inputs_seen, stepped, seen_t, called, moments, decoded = [], [], [], [], [], [], []
    real_randn = torch.randn

    def randn(*a, **k):
        t = real_randn(*a, **k)
        drawn.append(t.clone())
        return t
    inner_scale, inner_step, inner_encode, inner_decode = sched.scale_model_input, sched.step, pipe.vae.encode, pipe.decode_latents

    def scale_model_input(sample, t):          # the input of every evaluation: the latents after the evaluation before (the legacy loop: after its blend)
        inputs_seen.append(sample[: sample.shape[0] // 2].clone())
        seen_t.append(float(t))
        return inner_scale(sample, t)

    @functools.wraps(inner_step)          # (the pipeline reads step()'s signature to decide whether eta and the generator are handed over)
    def step(model_output, timestep, sample, **k):
        o = inner_step(model_output, timestep, sample, **k)
        stepped.append(o.prev_sample.clone())
        return o

    def encode(x, *a, **k):
        o = inner_encode(x, *a, **k)
        moments.append((x.clone(), o.latent_dist.parameters.clone()))
        return o

    def decode_latents(latents):
        decoded.append(latents.clone())
        return inner_decode(latents)
    sched.scale_model_input, sched.step, pipe.vae.encode, pipe.decode_latents = scale_model_input, step, encode, decode_latents
    prepared, inner_prepare = [], pipe.prepare_latents

    def prepare_latents(*a, **k):          # (the legacy pipeline's returns the clean latents it blends back in)
        prepared.append(inner_prepare(*a, **k))
        return prepared[-1]
    pipe.prepare_latents = prepare_latents
    torch.randn = randn
    try:
        common = dict(num_inference_steps=ES.STEPS, guidance_scale=ES.GUIDANCE, negative_prompt=ES.NEGATIVE, eta=case.eta,
                      generator=torch.Generator().manual_seed(ES.CALL_SEED), output_type="np", callback=lambda i, t, l: called.append(i), callback_steps=1)
        if case.pipeline == "img2img":
            res = pipe(ES.PROMPT, image=inp["image"].clone(), strength=case.strength, **common)
        elif case.pipeline == "inpaint":
            res = pipe(ES.PROMPT, image=inp["image"].clone(), mask_image=inp["mask"].clone(), height=64, width=64, **common)
        else:
            res = pipe(ES.PROMPT, image=PIL.Image.fromarray(inp["legacy_image"]), mask_image=PIL.Image.fromarray(inp["legacy_mask"]), strength=case.strength,
                       **common)
    finally:
        torch.randn = real_randn
        pipe.vae.encode, pipe.decode_latents, pipe.prepare_latents = inner_encode, inner_decode, inner_prepare
    traj = torch.stack(inputs_seen[1:] + decoded)
    assert len(traj) == len(stepped) == len(seen_t) and torch.isfinite(traj).all(), key
    for k, t in enumerate(drawn):
        out[f"{key}/noise_{k}"] = t.numpy()
    out[f"{key}/trajectory"], out[f"{key}/timesteps"] = traj.numpy(), np.array(seen_t, dtype=np.float64)
    out[f"{key}/callbacks"], out[f"{key}/images"] = np.array(called, dtype=np.int64), np.asarray(res.images, dtype=np.float32)
    # ---- the reference's own f32 results against the specification of the formula kernels
    tables, worst = engine_tables(case.scheduler), {}
    if case.pipeline in ("img2img", "legacy"):
        c_x, c_n = tables.add_noise_coefficients(seen_t[0], ES.STEPS)
        ref = ES.posterior_latents(moments[0][1], noise_post=drawn[0], noise_add=drawn[1], c_x=c_x, c_n=c_n)["latents"]
        worst["start latents"] = ES.inside(inputs_seen[0], *ref, f"{key} start latents")
    if case.pipeline == "inpaint":
        masked, mask_lat = ES.inpaint_prepare(inp["image"], inp["mask"])
        assert torch.equal(moments[0][0], masked), key
        ref = ES.posterior_latents(moments[0][1], noise_post=drawn[1])["clean"]
        # (the pipeline keeps the masked-image latents to itself: the reference's f32 operations on the moments and the noise it drew, in its order)
        got = 0.18215 * (moments[0][1][:, :4] + torch.exp(0.5 * moments[0][1][:, 4:].clamp(-30.0, 20.0)) * drawn[1])
        worst["masked-image latents"] = ES.inside(got, *ref, f"{key} masked-image latents")
        out.setdefault("inpaint_mask_latent", mask_lat.numpy())
    if case.pipeline == "legacy":
        clean = prepared[0][1]
        worst["clean latents"] = ES.inside(clean, *ES.posterior_latents(moments[0][1], noise_post=drawn[0])["clean"], f"{key} clean latents")
        mask = torch.from_numpy(1 - np.tile(np.array(PIL.Image.fromarray(inp["legacy_mask"]).convert("L").resize((8, 8), resample=PIL.Image.NEAREST)).astype(np.float32) / 255.0,
                                            (4, 1, 1))[None])
        for i, t in enumerate(seen_t):
            c_x, c_n = tables.add_noise_coefficients(t, ES.STEPS)
            ref = ES.renoise_blend(stepped[i], clean, drawn[1], mask[:, :1], c_x=c_x, c_n=c_n, B=1, C=4, F=1, HW=64)
            worst[f"blend {i}"] = ES.inside(traj[i].reshape(1, 4, 1, 64), *ref, f"{key} blend {i}")
    return worst


def main():
    MG2.install_sd_pipeline()
    import transformers
    if not hasattr(transformers, "CLIPFeatureExtractor"):          # removed in transformers 5; only the safety checker, which is off, uses it
        transformers.CLIPFeatureExtractor = type("CLIPFeatureExtractor", (), {})
    from diffusers.models.unet_2d_condition import UNet2DConditionModel
    from diffusers.pipelines.stable_diffusion.pipeline_stable_diffusion_img2img import StableDiffusionImg2ImgPipeline
    from diffusers.pipelines.stable_diffusion.pipeline_stable_diffusion_inpaint import StableDiffusionInpaintPipeline
    from diffusers.pipelines.stable_diffusion.pipeline_stable_diffusion_inpaint_legacy import StableDiffusionInpaintPipelineLegacy
    import diffusers.schedulers as S
    schedulers = {n: getattr(S, n) for n, _ in ES.SCHEDULERS.values()}
    cfg = MG2.cfg_2d()
    unet = MG2.ref_unet2d(cfg).eval()
    unet.load_state_dict(W.make_weights(W.unet_state_shapes(cfg), seed=ES.UNET_SEED), strict=True)
    c9 = cfg_9ch()
    unet9 = UNet2DConditionModel(sample_size=c9.sample_size, in_channels=9, out_channels=c9.out_channels, block_out_channels=c9.block_out_channels,
                                 layers_per_block=c9.layers_per_block, cross_attention_dim=c9.cross_attention_dim, attention_head_dim=c9.attention_head_dim,
                                 norm_num_groups=c9.norm_num_groups, norm_eps=c9.norm_eps).eval()
    shapes9 = W.unet_state_shapes(c9)
    assert {k: tuple(v.shape) for k, v in unet9.state_dict().items()} == dict(shapes9), "the 9-channel reference module's state-dict shapes"
    unet9.load_state_dict(W.make_weights(shapes9, seed=ES.UNET9_SEED), strict=True)
    vae = MG.ref_vae(vae_config()).eval()
    vae.load_state_dict(vae_weights(), strict=True)
    parts = dict(vae=vae, text_encoder=stubs.StubTextEncoder(cfg.cross_attention_dim), tokenizer=stubs.FakeTokenizer(), safety_checker=None,
                 feature_extractor=None, requires_safety_checker=False)
    pipes = {"img2img": lambda scheduler: StableDiffusionImg2ImgPipeline(unet=unet, scheduler=scheduler, **parts),
             "inpaint": lambda scheduler: StableDiffusionInpaintPipeline(unet=unet9, scheduler=scheduler, **parts),
             "legacy": lambda scheduler: StableDiffusionInpaintPipelineLegacy(unet=unet, scheduler=scheduler, **parts)}
    inp = inputs()
    out = dict(image=inp["image"].numpy(), mask=inp["mask"].numpy(), legacy_image=inp["legacy_image"], legacy_mask=inp["legacy_mask"],
               unet_weight_seed=np.int64(ES.UNET_SEED), unet9_weight_seed=np.int64(ES.UNET9_SEED), vae_weight_seed=np.int64(ES.VAE_SEED))
    for case in ES.CASES:
        worst = run_case(case, pipes, schedulers, inp, out)
        print(f"{ES.case_key(case)}: {len(out[ES.case_key(case) + '/trajectory'])} evaluations, callbacks {out[ES.case_key(case) + '/callbacks'].tolist()}; "
              "the reference's worst element x its bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    # the reference schedulers' add_noise on unit inputs, at every entry of the 5-step list: column 0 = add_noise(1, 0, t), column 1 = add_noise(0, 1, t)
    one, zero = torch.ones(1, 1, 1, 1), torch.zeros(1, 1, 1, 1)
    for name, (cls_name, kw) in ES.SCHEDULERS.items():
        s = schedulers[cls_name](**kw)
        s.set_timesteps(ES.STEPS)
        out[f"add_noise/{name}"] = np.array([[float(s.add_noise(one, zero, t.reshape(1))), float(s.add_noise(zero, one, t.reshape(1)))] for t in s.timesteps],
                                            dtype=np.float32)
        out[f"add_noise_timesteps/{name}"] = s.timesteps.numpy().astype(np.float64)
    with torch.no_grad():
        out["text_embeddings"] = pipes["img2img"](schedulers["DDIMScheduler"](**ES.SCHEDULERS["ddim"][1]))._encode_prompt(ES.PROMPT, "cpu", 1, True, ES.NEGATIVE).numpy()
    path = os.path.join(OUT, "pipeline_tiny_edit.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path) >> 10} KiB")


if __name__ == "__main__":
    main()
