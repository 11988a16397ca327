"""The CPU op emulator with the three kernels of the image-editing front end (fyc_posterior_latents, fyc_inpaint_prepare, fyc_renoise_blend).  tests/emu_ops.py and the
emulators stacked on it stay as they are.  Everything is f32 in the order of the kernels (csrc/image_edit.hip), and - as there - an input a variant does not use is never
read and an output not handed over is never written."""
import torch

from emu_ops_pndm import PNDMEmuOps


class EditEmuOps(PNDMEmuOps):
    def posterior_latents(self, moments, latents, *, noise_post=None, noise_add=None, clean_out=None, scale, c_x=1.0, c_n=0.0):
        N, C2, H, W = moments.shape
        assert C2 % 2 == 0 and tuple(latents.shape) == (N, C2 // 2, H, W)
        assert all(t is None or (t.dtype == torch.float32 and t.is_contiguous()) for t in (moments, latents, noise_post, noise_add, clean_out))
        f32 = lambda s: float(torch.tensor(s, dtype=torch.float32))      # noqa: E731
        scale, c_x, c_n = f32(scale), f32(c_x), f32(c_n)
        mean = moments[:, : C2 // 2]
        if noise_post is not None:
            std = torch.exp(0.5 * moments[:, C2 // 2:].clamp(-30.0, 20.0))
            mean = mean + std * noise_post
        z = mean * scale
        lat = c_x * z
        if noise_add is not None:
            lat = lat + c_n * noise_add
        if clean_out is not None:
            clean_out.copy_(z)
        latents.copy_(lat)

    def inpaint_prepare(self, image, mask, *, masked=None, mask_latent=None):
        N, one, H, W = mask.shape
        assert one == 1 and H % 8 == 0 and W % 8 == 0 and (masked is not None or mask_latent is not None)
        if masked is not None:
            masked.copy_(image * (mask < 0.5).to(torch.float32))
        if mask_latent is not None:
            mask_latent.copy_(torch.where(mask[:, :, ::8, ::8] < 0.5, 0.0, 1.0))

    def renoise_blend(self, latents, orig, noise, mask, *, c_x, c_n, B, C_, F, HW):
        f32 = lambda s: float(torch.tensor(s, dtype=torch.float32))      # noqa: E731
        c_x, c_n = f32(c_x), f32(c_n)
        lat = latents.reshape(B, C_, F, HW)
        o, nz, m = orig.reshape(B, C_, -1, HW), noise.reshape(B, C_, -1, HW), mask.reshape(B, 1, 1, HW)
        assert o.shape == nz.shape and o.shape[2] in (1, F)
        lat.copy_((c_x * o + c_n * nz) * m + lat * (1.0 - m))
