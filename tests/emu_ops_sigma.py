"""The CPU op emulator with the fused guidance + sigma-space step (fyc_cfg_sigma_step) and the scaled UNet input (fyc_unet_input_scaled).  tests/emu_ops.py,
tests/emu_ops_sampling.py and tests/emu_ops_solver.py stay as they are.  The guided (and rescaled) prediction is SamplingEmuOps', everything else is f32 in the order
of the kernels (csrc/elementwise.hip::cfg_sigma_kernel, unet_input_scaled_kernel), and - as there - a history or noise buffer the call does not use is never read."""
import torch

from emu_ops import _flat
from emu_ops_solver import SolverEmuOps


class SigmaEmuOps(SolverEmuOps):
    def cfg_sigma_step(self, pred, latents, coef, *, hist_out=None, hist_1=None, hist_2=None, hist_3=None, order=1, noise=None, B, F, HW, c_latent, ld, cfg,
                       guidance, pred_single=None, video_scale=0.0, guidance_rescale=0.0):
        hists = (hist_1, hist_2, hist_3)
        assert order in (1, 2, 3, 4) and all(hists[k] is not None for k in range(order - 1)), order
        assert not 0.0 < guidance_rescale or cfg, "guidance rescale needs classifier-free guidance"
        assert pred_single is None or cfg
        for w in (hist_out, noise):
            for h in (latents, *hists, hist_out if w is noise else None):
                assert w is None or h is None or h.data_ptr() != w.data_ptr(), "hist_out / noise aliases another buffer"
        if guidance_rescale > 0:
            v, _ = self.guided_rescaled(pred, B=B, F=F, HW=HW, c_latent=c_latent, ld=ld, guidance=guidance, guidance_rescale=guidance_rescale,
                                        pred_single=pred_single, video_scale=video_scale)
        else:
            p = _flat(pred)[: (2 if cfg else 1) * B * F * HW * ld].reshape(-1, B, F, HW, ld)[..., :c_latent].float()
            v = p[0] + guidance * (p[1] - p[0]) if cfg else p[0]
            if pred_single is not None:
                s1 = _flat(pred_single)[: B * F * HW * ld].reshape(B, F, HW, ld)[..., :c_latent].float()
                v = s1 + video_scale * (p[0] - s1) + guidance * (p[1] - p[0])
        v = v.permute(0, 3, 1, 2)                                  # B C F HW
        shape = (B, c_latent, F, HW)
        x = latents.reshape(shape)
        ax, av, cx, c0, c1, c2, c3, cn = [float(c) for c in coef.reshape(-1)[:8]]
        d = ax * x + av * v
        nx = cx * x + c0 * d
        for k, c in ((2, c1), (3, c2), (4, c3)):
            if order >= k:
                nx = nx + c * hists[k - 2].reshape(shape)
        if noise is not None:
            nx = nx + cn * noise.reshape(shape)
        x.copy_(nx)
        if hist_out is not None:
            hist_out.reshape(shape).copy_(d)

    def unet_input_scaled(self, latents, mask, first, x, *, denom, scale_cond, B, F, HW, c_latent, c_pad, cfg_dup, mask_frames=1, mode=0):
        denom = float(torch.tensor(denom, dtype=torch.float32))
        assert denom >= 1.0 and denom < float("inf") and (mode == 0 or not scale_cond)
        cden = denom if scale_cond else 1.0
        out = torch.zeros(B, F, HW, c_pad)
        out[..., :c_latent] = latents.reshape(B, c_latent, F, HW).permute(0, 2, 3, 1) / denom
        if mode == 1:
            if first is not None:
                out[..., c_latent: 2 * c_latent] = first.reshape(B, 1, c_latent, HW).permute(0, 1, 3, 2)
        else:
            if mask is not None:
                m = mask.reshape(B, mask_frames, HW).clamp(0, 1) / cden
                out[..., c_latent] = m if mask_frames > 1 else m.expand(B, F, HW)
            else:
                out[:, 0, :, c_latent] = torch.tensor(1.0) / cden
            if first is not None:
                out[:, 0, :, c_latent + 1: 2 * c_latent + 1] = first.reshape(B, c_latent, HW).permute(0, 2, 1) / cden
        out = torch.cat([out] * cfg_dup, dim=0)
        _flat(x)[: out.numel()].reshape(out.shape).copy_(out.to(x.dtype))
