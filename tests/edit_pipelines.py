"""Building and running the drop-in image-editing pipelines on the tiny models of tests/golden/pipeline_tiny_edit.npz (a helper, not a test module; shared by
tests/test_edit.py on the emulator and tests/test_edit_gpu.py on the MI355X).  Nothing here reads the reference tree: the weights are re-derived from the seeds the
golden file names, the inputs and the expected results come from the file."""
import os

import numpy as np
import torch

import edit_spec as ES
from oracle import functional as Fn
from oracle import stubs
from oracle import weights as W

UNET_KW = dict(sample_size=8, block_out_channels=(64, 128, 256, 256), cross_attention_dim=64)


def load_golden(golden_dir):
    return {k: torch.from_numpy(v) if v.shape else v for k, v in np.load(os.path.join(golden_dir, "pipeline_tiny_edit.npz")).items()}


def cfg_2d(concat=False):
    return Fn.tiny_unet_config(use_motion_module=False, use_fps_condition=False, use_first_frame_mask_condition_concat=concat)


def vae_weights(seed):
    vcfg = Fn.VAEConfig(block_out_channels=(64, 128, 128, 128))
    sd = W.make_weights(W.vae_decoder_state_shapes(vcfg), seed=seed)
    sd.update(W.make_weights(W.vae_encoder_state_shapes(vcfg), seed=seed + 1))
    return sd


def build_models(g, dtype=torch.float32, device="cpu"):
    """-> dict(vae, unet, unet9) of drop-in modules with the golden file's weights (install_dropin() must be active)"""
    from diffusers import AutoencoderKL, UNet2DConditionModel
    vcfg = Fn.VAEConfig(block_out_channels=(64, 128, 128, 128))
    vae = AutoencoderKL(block_out_channels=vcfg.block_out_channels, layers_per_block=vcfg.layers_per_block, latent_channels=4, compute_dtype=dtype)
    vae.load_state_dict(vae_weights(int(g["vae_weight_seed"])), strict=True)
    unet = UNet2DConditionModel(**UNET_KW, compute_dtype=dtype)
    unet.load_state_dict(W.make_weights(W.unet_state_shapes(cfg_2d()), int(g["unet_weight_seed"])), strict=True)
    unet9 = UNet2DConditionModel(in_channels=9, **UNET_KW, compute_dtype=dtype)
    unet9.load_state_dict(W.make_weights(W.unet_state_shapes(cfg_2d(concat=True)), int(g["unet9_weight_seed"])), strict=True)
    return {k: m.to(device) for k, m in dict(vae=vae, unet=unet, unet9=unet9).items()}


def build_pipeline(case, models, device="cpu"):
    import diffusers
    cls_name, kw = ES.SCHEDULERS[case.scheduler]
    cls = dict(img2img=diffusers.StableDiffusionImg2ImgPipeline, inpaint=diffusers.StableDiffusionInpaintPipeline,
               legacy=diffusers.StableDiffusionInpaintPipelineLegacy)[case.pipeline]
    pipe = cls.from_pretrained("unused", vae=models["vae"], text_encoder=stubs.StubTextEncoder(64), tokenizer=stubs.FakeTokenizer(),
                               unet=models["unet9" if case.pipeline == "inpaint" else "unet"], scheduler=getattr(diffusers, cls_name)(**kw), safety_checker=None)
    return pipe.to(device)


class Run:
    """what one call left behind: traj [evaluations, 1, 4, 8, 8] (the latents after every evaluation, from the sampler's own callback: the pipeline holds the caller's back over
    the warm-up), timesteps, the indices the caller's callback saw, images, the tensors torch.randn returned in order"""


def run_case(case, g, pipe, monkeypatch):
    from PIL import Image
    from followyourclick_amd.engine import sampler as S
    run, traj, seen, called, drawn = Run(), [], [], [], []
    inner_sample, inner_randn = S.DDIMSampler.sample, torch.randn

    def sample(self, *a, callback=None, **k):
        def cb(i, t, lat):
            traj.append(lat[:, :, 0].detach().cpu().clone())
            seen.append(float(t))
            if callback is not None:
                callback(i, t, lat)
        return inner_sample(self, *a, callback=cb, **k)

    def randn(*a, **k):
        t = inner_randn(*a, **k)
        drawn.append(t.detach().cpu().clone())
        return t
    common = dict(num_inference_steps=ES.STEPS, guidance_scale=ES.GUIDANCE, negative_prompt=ES.NEGATIVE, eta=case.eta,
                  generator=torch.Generator().manual_seed(ES.CALL_SEED), output_type="np", callback=lambda i, t, l: called.append(i), callback_steps=1)
    with monkeypatch.context() as m:
        m.setattr(S.DDIMSampler, "sample", sample)
        m.setattr(torch, "randn", randn)
        if case.pipeline == "img2img":
            out = pipe(ES.PROMPT, image=g["image"].clone(), strength=case.strength, **common)
        elif case.pipeline == "inpaint":
            out = pipe(ES.PROMPT, image=g["image"].clone(), mask_image=g["mask"].clone(), height=64, width=64, **common)
        else:
            out = pipe(ES.PROMPT, image=Image.fromarray(g["legacy_image"].numpy()), mask_image=Image.fromarray(g["legacy_mask"].numpy()), strength=case.strength,
                       **common)
    run.traj, run.timesteps, run.callbacks, run.images, run.drawn = torch.stack(traj), seen, called, torch.from_numpy(np.asarray(out.images)), drawn
    return run


def trajectory_error(run, g, case):
    """per-evaluation relative L2 against the reference's trajectory"""
    ref = g[ES.case_key(case) + "/trajectory"]
    assert run.traj.shape == ref.shape, (ES.case_key(case), run.traj.shape, ref.shape)
    return (run.traj - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)
