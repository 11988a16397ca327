"""`diffusers.StableDiffusionInpaintPipeline` on the MI355X engine: the 9-channel inpainting UNets (stable-diffusion-inpainting,
stable-diffusion-2-inpainting), whose input is latents | mask | masked-image latents.

Call surface, defaults, argument checks and output type follow reference
diffusers/pipelines/stable_diffusion/pipeline_stable_diffusion_inpaint.py:38-139 (`prepare_mask_and_masked_image`), :493-542, :545-735
(`__call__`).  Inputs are converted to tensors on the host as there; the binarised mask at the latents' size and the masked image are ONE kernel
(ops.inpaint_prepare) whose image output the VAE encoder engine takes as it is, the masked-image latents one more (ops.posterior_latents).  The
loop is the engine's sampler with the concat input build of a one-frame clip (fyc_unet_input mode 0: the same channel order); a sigma-space
scheduler's divisor reaches the latents only, as the reference scales before it concatenates (:699-703).
"""
from __future__ import annotations

from typing import Callable, List, Optional, Union

import numpy as np
import torch

from followyourclick_amd import ops as ops_mod

from .pipeline_stable_diffusion import StableDiffusionPipeline
from .pipeline_stable_diffusion_img2img import VAE_SCALE, randn


def image_and_mask_tensors(image, mask):
    """-> (image (N, 3, H, W) f32 in [-1, 1], mask (N, 1, H, W) f32 in [0, 1], not yet binarised): the conversions and checks of
    prepare_mask_and_masked_image (reference :66-135) up to the binarisation, which the kernel does"""
    import PIL.Image
    if isinstance(image, torch.Tensor):
        if not isinstance(mask, torch.Tensor):
            raise TypeError(f"`image` is a torch.Tensor but `mask` (type: {type(mask)} is not")
        if image.ndim == 3:
            assert image.shape[0] == 3, "Image outside a batch should be of shape (3, H, W)"
            image = image.unsqueeze(0)
        if mask.ndim == 2:
            mask = mask.unsqueeze(0).unsqueeze(0)
        if mask.ndim == 3:          # one mask with its channel axis, or a batch of masks without
            mask = mask.unsqueeze(0) if mask.shape[0] == 1 else mask.unsqueeze(1)
        assert image.ndim == 4 and mask.ndim == 4, "Image and Mask must have 4 dimensions"
        assert image.shape[-2:] == mask.shape[-2:], "Image and Mask must have the same spatial dimensions"
        assert image.shape[0] == mask.shape[0], "Image and Mask must have the same batch size"
        if image.min() < -1 or image.max() > 1:
            raise ValueError("Image should be in [-1, 1] range")
        if mask.min() < 0 or mask.max() > 1:
            raise ValueError("Mask should be in [0, 1] range")
        return image.to(dtype=torch.float32), mask.to(dtype=torch.float32)
    if isinstance(mask, torch.Tensor):
        raise TypeError(f"`mask` is a torch.Tensor but `image` (type: {type(image)} is not")
    if isinstance(image, (PIL.Image.Image, np.ndarray)):
        image = [image]
    if isinstance(image, list) and isinstance(image[0], PIL.Image.Image):
        image = np.concatenate([np.array(i.convert("RGB"))[None, :] for i in image], axis=0)
    elif isinstance(image, list) and isinstance(image[0], np.ndarray):
        image = np.concatenate([i[None, :] for i in image], axis=0)
    image = torch.from_numpy(image.transpose(0, 3, 1, 2)).to(dtype=torch.float32) / 127.5 - 1.0
    if isinstance(mask, (PIL.Image.Image, np.ndarray)):
        mask = [mask]
    if isinstance(mask, list) and isinstance(mask[0], PIL.Image.Image):
        mask = np.concatenate([np.array(m.convert("L"))[None, None, :] for m in mask], axis=0).astype(np.float32) / 255.0
    elif isinstance(mask, list) and isinstance(mask[0], np.ndarray):
        mask = np.concatenate([m[None, None, :] for m in mask], axis=0)
    return image, torch.from_numpy(np.ascontiguousarray(mask)).to(dtype=torch.float32)


class StableDiffusionInpaintPipeline(StableDiffusionPipeline):
    _optional_components = ["safety_checker"]

    def prepare_mask_latents(self, image, mask, batch_size, height, width, dtype, device, generator):
        """-> (mask at the latents' size (batch, 1, h, w), masked-image latents (batch, C, h, w)), both f32 (reference :493-542 without the CFG
        duplication: the sampler's input build repeats them for the two halves)"""
        o = ops_mod.get()
        image, mask = [t.to(device=device, dtype=torch.float32).contiguous() for t in (image, mask)]
        n = image.shape[0]
        if tuple(image.shape[2:]) != (height, width):
            raise ValueError(f"`image` and `mask_image` are {tuple(image.shape[2:])}, `height` and `width` are {(height, width)}")
        masked = torch.empty_like(image)
        mask_lat = torch.empty(n, 1, height // self.vae_scale_factor, width // self.vae_scale_factor, dtype=torch.float32, device=image.device)
        o.inpaint_prepare(image, mask, masked=masked, mask_latent=mask_lat)
        moments = self.vae.encode(masked.to(dtype)).latent_dist.parameters.to(torch.float32).contiguous()
        shape = (n, moments.shape[1] // 2) + tuple(moments.shape[2:])
        noise_post = randn(shape, generator, torch.float32, device).to(dtype).to(torch.float32).contiguous()
        masked_lat = torch.empty(shape, dtype=torch.float32, device=moments.device)
        o.posterior_latents(moments, masked_lat, noise_post=noise_post, scale=VAE_SCALE)
        for name, t in (("mask", mask_lat), ("images", masked_lat)):
            if t.shape[0] < batch_size and batch_size % t.shape[0] != 0:
                raise ValueError(f"The passed {name} and the required batch size don't match: {t.shape[0]} were passed for a total batch size of "
                                 f"{batch_size}, which they do not divide.")
        if n < batch_size:
            mask_lat, masked_lat = mask_lat.repeat(batch_size // n, 1, 1, 1), masked_lat.repeat(batch_size // n, 1, 1, 1)
        return mask_lat, masked_lat

    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str]], image=None, mask_image=None, height: Optional[int] = None, width: Optional[int] = None,
                 num_inference_steps: int = 50, guidance_scale: float = 7.5, negative_prompt: Optional[Union[str, List[str]]] = None,
                 num_images_per_prompt: Optional[int] = 1, eta: float = 0.0, generator=None, latents: Optional[torch.Tensor] = None,
                 output_type: Optional[str] = "pil", return_dict: bool = True,
                 callback: Optional[Callable[[int, int, torch.Tensor], None]] = None, callback_steps: Optional[int] = 1):
        height = height or self.unet.config.sample_size * self.vae_scale_factor
        width = width or self.unet.config.sample_size * self.vae_scale_factor
        self.check_inputs(prompt, height, width, callback_steps)
        self.check_scheduler()
        batch_size = 1 if isinstance(prompt, str) else len(prompt)
        device = self._execution_device
        cfg_on = guidance_scale > 1.0
        text_embeddings = self._encode_prompt(prompt, device, num_images_per_prompt, cfg_on, negative_prompt)
        image, mask = image_and_mask_tensors(image, mask_image)
        self.scheduler.set_timesteps(num_inference_steps, device=device)
        total = batch_size * num_images_per_prompt
        num_channels_latents = self.vae.config.latent_channels
        latents = self.prepare_latents(total, num_channels_latents, height, width, text_embeddings.dtype, device, generator, latents)
        mask_lat, masked_lat = self.prepare_mask_latents(image, mask, total, height, width, text_embeddings.dtype, device, generator)
        if num_channels_latents + mask_lat.shape[1] + masked_lat.shape[1] != self.unet.config.in_channels:
            raise ValueError(f"Incorrect configuration settings! The config of `pipeline.unet` expects {self.unet.config.in_channels} input channels but "
                             f"received `num_channels_latents`: {num_channels_latents} + `num_channels_mask`: {mask_lat.shape[1]} + "
                             f"`num_channels_masked_image`: {masked_lat.shape[1]}. Please verify the config of `pipeline.unet` or your `mask_image` "
                             "or `image` input.")
        out = self.run_sampler(latents, text_embeddings, num_inference_steps, guidance_scale, callback, callback_steps, eta=float(eta),
                               generator=generator, idle_step_noise=generator, first_image_latents=masked_lat, first_images_mask=mask_lat, scale_condition=False)
        return self.finish(out, output_type, return_dict)
