"""`diffusers.StableDiffusionInpaintPipelineLegacy` on the MI355X engine: inpainting with an ordinary 4-channel Stable Diffusion UNet - img2img
whose known region is re-imposed after every step.

Call surface, defaults, argument checks and output type follow reference
diffusers/pipelines/stable_diffusion/pipeline_stable_diffusion_inpaint_legacy.py:45-65 (`preprocess_image`, `preprocess_mask`), :406-420,
:423-596 (`__call__`).  Image and mask are prepared on the host with PIL, where they live: sizes rounded down to a multiple of 32, lanczos /
nearest, `1 - mask`, tiled to the latents' 4 channels.  The start latents and the clean ones come from one launch (ops.posterior_latents), and
after the step kernel of every entry of the timestep list one more (ops.renoise_blend) puts the original, noised to THAT entry's timestep, back
where the mask keeps it (:573-575).
"""
from __future__ import annotations

from typing import Callable, List, Optional, Union

import numpy as np
import torch

from .pipeline_stable_diffusion_img2img import StableDiffusionImg2ImgPipeline


def preprocess_image(image):
    """PIL image -> (1, 3, H, W) f32 in [-1, 1], sizes rounded down to a multiple of 32 with lanczos"""
    import PIL.Image
    w, h = (x - x % 32 for x in image.size)
    image = image.resize((w, h), resample=getattr(PIL.Image, "Resampling", PIL.Image).LANCZOS)
    arr = np.array(image).astype(np.float32) / 255.0
    return 2.0 * torch.from_numpy(arr[None].transpose(0, 3, 1, 2)) - 1.0


def preprocess_mask(mask, scale_factor=8):
    """PIL mask -> (1, 4, H/8, W/8) f32: luminance, nearest-resized to the latents' size, tiled over their channels; 1 = keep (black), 0 = repaint (white)"""
    import PIL.Image
    mask = mask.convert("L")
    w, h = (x - x % 32 for x in mask.size)
    mask = mask.resize((w // scale_factor, h // scale_factor), resample=getattr(PIL.Image, "Resampling", PIL.Image).NEAREST)
    arr = np.tile(np.array(mask).astype(np.float32) / 255.0, (4, 1, 1))[None]
    return torch.from_numpy(1 - arr)


class StableDiffusionInpaintPipelineLegacy(StableDiffusionImg2ImgPipeline):
    _optional_components = ["safety_checker"]

    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str]], image=None, mask_image=None, strength: float = 0.8, num_inference_steps: Optional[int] = 50,
                 guidance_scale: Optional[float] = 7.5, negative_prompt: Optional[Union[str, List[str]]] = None,
                 num_images_per_prompt: Optional[int] = 1, add_predicted_noise: Optional[bool] = False, eta: Optional[float] = 0.0, generator=None,
                 output_type: Optional[str] = "pil", return_dict: bool = True,
                 callback: Optional[Callable[[int, int, torch.Tensor], None]] = None, callback_steps: Optional[int] = 1, **kwargs):
        image = kwargs.pop("init_image", None) or image          # (the reference's deprecated name)
        self.check_inputs(prompt, strength, callback_steps)
        self.check_scheduler()
        if add_predicted_noise:
            raise NotImplementedError("StableDiffusionInpaintPipelineLegacy on the MI355X engine: add_predicted_noise=True (re-noising the original "
                                      "with the unconditional prediction) is not implemented; the blend kernel takes the drawn noise")
        batch_size = 1 if isinstance(prompt, str) else len(prompt)
        device = self._execution_device
        cfg_on = guidance_scale > 1.0
        text_embeddings = self._encode_prompt(prompt, device, num_images_per_prompt, cfg_on, negative_prompt)
        if not isinstance(image, torch.Tensor):
            image = preprocess_image(image)
        if not isinstance(mask_image, torch.Tensor):
            mask_image = preprocess_mask(mask_image, self.vae_scale_factor)
        self.scheduler.set_timesteps(num_inference_steps, device=device)
        timesteps, _, t_start = self.get_timesteps(num_inference_steps, strength, device)
        total = batch_size * num_images_per_prompt
        latents, clean, noise = self.start_latents(image, timesteps[0], num_inference_steps, total, text_embeddings.dtype, device, generator,
                                                   expand="legacy", keep_clean=True)
        mask = torch.cat([mask_image.to(device=device, dtype=latents.dtype)] * total)
        if mask.shape[0] != latents.shape[0] or mask.shape[2:] != latents.shape[2:]:
            raise ValueError(f"mask_image {tuple(mask.shape)} does not fit the latents {tuple(latents.shape)}")
        out = self.run_sampler(latents, text_embeddings, num_inference_steps, guidance_scale, callback, callback_steps, start_index=t_start,
                               eta=float(eta), generator=generator, idle_step_noise=generator, blend=(clean, noise, mask))
        return self.finish(out, output_type, return_dict)
