"""`diffusers.StableDiffusionImg2ImgPipeline` on the MI355X engine: an encoded image, noised to the timestep `strength` selects, denoised
from there.

Call surface, defaults, argument checks and output type follow reference
diffusers/pipelines/stable_diffusion/pipeline_stable_diffusion_img2img.py:45-63 (`preprocess`), :380-455, :457-604 (`__call__`).  Prompt
encoding, decode and the callback warm-up rule are StableDiffusionPipeline's.  The image is encoded by the VAE encoder engine; its moments
become the start latents in ONE kernel (ops.posterior_latents: sample the posterior, `0.18215 *`, add_noise); the loop is the engine's sampler
started at entry t_start of the scheduler's timestep list.  Noise is drawn with torch.randn on the generator's device in the reference's shapes,
dtype and order (the posterior's, then add_noise's, then a stochastic scheduler's per step): a seeded CPU generator gives the reference's numbers.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Union

import numpy as np
import torch

from followyourclick_amd import ops as ops_mod
from followyourclick_amd.engine.sampler import make_sampler

from .pipeline_stable_diffusion import StableDiffusionPipeline

VAE_SCALE = 0.18215          # the literal of the reference's pipelines (`init_latents = 0.18215 * init_latents`)


def preprocess(image):
    """PIL image(s) -> (N, 3, H, W) f32 in [-1, 1], sizes rounded down to a multiple of 32 with lanczos; tensors pass (a list is concatenated)"""
    import PIL.Image
    if isinstance(image, torch.Tensor):
        return image
    if isinstance(image, PIL.Image.Image):
        image = [image]
    if isinstance(image[0], PIL.Image.Image):
        w, h = (x - x % 32 for x in image[0].size)
        lanczos = getattr(PIL.Image, "Resampling", PIL.Image).LANCZOS
        arr = np.concatenate([np.array(i.resize((w, h), resample=lanczos))[None, :] for i in image], axis=0)
        arr = np.array(arr).astype(np.float32) / 255.0
        return torch.from_numpy(2.0 * arr.transpose(0, 3, 1, 2) - 1.0)
    if isinstance(image[0], torch.Tensor):
        return torch.cat(image, dim=0)
    return image


def randn(shape, generator, dtype, device) -> torch.Tensor:
    """torch.randn(shape) from `generator` on ITS device (None: on `device`), a list of generators one sample each, as the reference draws"""
    if isinstance(generator, list):
        return torch.cat([torch.randn((1,) + tuple(shape[1:]), generator=g, device=g.device, dtype=dtype).to(device) for g in generator])
    gdev = device if generator is None else generator.device
    return torch.randn(tuple(shape), generator=generator, device=gdev, dtype=dtype).to(device)


class StableDiffusionImg2ImgPipeline(StableDiffusionPipeline):
    _optional_components = ["safety_checker"]

    def check_inputs(self, prompt, strength, callback_steps):
        if not isinstance(prompt, str) and not isinstance(prompt, list):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        if strength < 0 or strength > 1:
            raise ValueError(f"The value of strength should in [1.0, 1.0] but is {strength}")
        if (callback_steps is None) or (not isinstance(callback_steps, int) or callback_steps <= 0):
            raise ValueError(f"`callback_steps` has to be a positive integer but is {callback_steps} of type {type(callback_steps)}.")

    def get_timesteps(self, num_inference_steps, strength, device=None):
        """-> (the entries of scheduler.timesteps the run takes, the steps left, t_start) (reference :393-400).  A strength that leaves no step
        (int(n * strength) = 0: the reference goes on to an empty timestep list and fails inside add_noise) is refused"""
        init_timestep = min(int(num_inference_steps * strength), num_inference_steps)
        t_start = max(num_inference_steps - init_timestep, 0)
        if init_timestep < 1:
            raise ValueError(f"strength = {strength} leaves zero steps of {num_inference_steps} inference steps (int(num_inference_steps * strength) = 0): "
                             "nothing to denoise")
        return self.scheduler.timesteps[t_start:], num_inference_steps - t_start, t_start

    def start_latents(self, image, timestep, num_inference_steps, batch_size, dtype, device, generator, expand: str, keep_clean: bool = False):
        """image (n, 3, H, W) -> (noised start latents (batch, C, h, w) f32, the clean ones or None, the add_noise noise): VAE moments through
        ops.posterior_latents with the add_noise coefficients of `timestep`.  expand: how n images become `batch` latents - "img2img": duplicated
        when batch is a multiple of n (reference :422-438), "legacy": repeated batch times (pipeline_stable_diffusion_inpaint_legacy.py:413)"""
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                             f" size of {batch_size}. Make sure the batch size matches the length of the generators.")
        image = image.to(device=device, dtype=dtype)
        moments = self.vae.encode(image).latent_dist.parameters.to(torch.float32)
        n, c2 = moments.shape[:2]
        shape = (n, c2 // 2) + tuple(moments.shape[2:])
        noise_post = randn(shape, generator, torch.float32, device).to(dtype)       # DiagonalGaussianDistribution.sample: f32, then the parameters' dtype
        if expand == "legacy":
            times = batch_size
        elif batch_size > n and batch_size % n == 0:
            times = batch_size // n
        elif batch_size > n:
            raise ValueError(f"Cannot duplicate `image` of batch size {n} to {batch_size} text prompts.")
        else:
            times = 1
        if times > 1:
            moments, noise_post = torch.cat([moments] * times), torch.cat([noise_post] * times)
        shape = (moments.shape[0],) + shape[1:]
        noise = randn(shape, generator, dtype, device)
        tables = make_sampler(self.unet._get_engine(), self.scheduler.engine_config).tables
        c_x, c_n = tables.add_noise_coefficients(timestep, num_inference_steps)
        f32 = lambda t: t.to(torch.float32).contiguous()      # noqa: E731
        latents = torch.empty(shape, dtype=torch.float32, device=moments.device)
        clean = torch.empty_like(latents) if keep_clean else None
        ops_mod.get().posterior_latents(f32(moments), latents, noise_post=f32(noise_post), noise_add=f32(noise), clean_out=clean, scale=VAE_SCALE,
                                        c_x=c_x, c_n=c_n)
        return latents, clean, noise

    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str]], image=None, strength: float = 0.8, num_inference_steps: Optional[int] = 50,
                 guidance_scale: Optional[float] = 7.5, negative_prompt: Optional[Union[str, List[str]]] = None,
                 num_images_per_prompt: Optional[int] = 1, eta: Optional[float] = 0.0, generator=None, output_type: Optional[str] = "pil",
                 return_dict: bool = True, callback: Optional[Callable[[int, int, torch.Tensor], None]] = None,
                 callback_steps: Optional[int] = 1, **kwargs):
        image = kwargs.pop("init_image", None) or image          # (the reference's deprecated name)
        self.check_inputs(prompt, strength, callback_steps)
        self.check_scheduler()
        batch_size = 1 if isinstance(prompt, str) else len(prompt)
        device = self._execution_device
        cfg_on = guidance_scale > 1.0
        text_embeddings = self._encode_prompt(prompt, device, num_images_per_prompt, cfg_on, negative_prompt)
        image = preprocess(image)
        self.scheduler.set_timesteps(num_inference_steps, device=device)
        timesteps, _, t_start = self.get_timesteps(num_inference_steps, strength, device)
        latents, _, _ = self.start_latents(image, timesteps[0], num_inference_steps, batch_size * num_images_per_prompt, text_embeddings.dtype,
                                           device, generator, expand="img2img")
        out = self.run_sampler(latents, text_embeddings, num_inference_steps, guidance_scale, callback, callback_steps, start_index=t_start,
                               eta=float(eta), generator=generator, idle_step_noise=generator)
        return self.finish(out, output_type, return_dict)
