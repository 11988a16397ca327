"""The CPU op emulator with the guidance rescale of the fused DDIM step (fyc_cfg_ddim_step_rescaled).  tests/emu_ops.py stays as it is: plain EmuOps lacks the
method, and the sampler never asks for it while guidance_rescale is 0.  The moments are taken in f64 as the kernel takes them, the per-sample factor is formed in
f64 and rounded once to f32, and everything else is f32 in the order of the kernel (csrc/elementwise.hip::cfg_ddim_row)."""
import torch

from emu_ops import EmuOps, _flat


class SamplingEmuOps(EmuOps):
    @staticmethod
    def guided_rescaled(pred, *, B, F, HW, c_latent, ld, guidance, guidance_rescale, pred_single=None, video_scale=0.0):
        """-> (v' [B][F][HW][c_latent] f32: the guided prediction times the factor of its sample, factor [B] f32)"""
        p = _flat(pred)[: 2 * B * F * HW * ld].reshape(2, B, F, HW, ld)[..., :c_latent].float()
        v = p[0] + guidance * (p[1] - p[0])
        if pred_single is not None:
            s1 = _flat(pred_single)[: B * F * HW * ld].reshape(B, F, HW, ld)[..., :c_latent].float()
            v = s1 + video_scale * (p[0] - s1) + guidance * (p[1] - p[0])
        n = F * HW * c_latent

        def var(t):          # the kernel's one-pass form: f64 sums of the f32 values and of their (exact) squares
            t = t.double().reshape(B, -1)
            return ((t * t).sum(dim=1) - t.sum(dim=1) ** 2 / n).clamp_min(0.0) / (n - 1)
        var_c, var_v = var(p[1]), var(v)
        phi = float(torch.tensor(guidance_rescale, dtype=torch.float32))
        factor = torch.where(var_v > 0, phi * (var_c.sqrt() / var_v.sqrt()) + (1.0 - phi), torch.ones_like(var_v)).float()
        return v * factor.reshape(B, 1, 1, 1), factor

    def cfg_ddim_step_rescaled(self, pred, latents, coef, *, guidance_rescale, B, F, HW, c_latent, ld, cfg, guidance, pred_type, clip_sample,
                               pred_single=None, video_scale=0.0, variance_noise=None, sigma=0.0, clipped_model_output=False):
        kw = dict(B=B, F=F, HW=HW, c_latent=c_latent, ld=ld, guidance=guidance, pred_single=pred_single, video_scale=video_scale)
        if not 0.0 <= guidance_rescale <= 1.0:
            raise ValueError(f"guidance_rescale {guidance_rescale}")
        if guidance_rescale == 0.0:
            return self.cfg_ddim_step(pred, latents, coef, cfg=cfg, pred_type=pred_type, clip_sample=clip_sample, variance_noise=variance_noise, sigma=sigma,
                                      clipped_model_output=clipped_model_output, **kw)
        assert cfg, "guidance rescale needs classifier-free guidance"
        v, _ = self.guided_rescaled(pred, guidance_rescale=guidance_rescale, **kw)
        v = v.permute(0, 3, 1, 2)                                  # B C F HW
        x = latents.reshape(B, c_latent, F, HW)
        sa, sb, sap, sbp = [float(c) for c in coef.reshape(-1)[:4]]
        if pred_type == 1:
            x0, eps = sa * x - sb * v, sa * v + sb * x
        elif pred_type == 0:
            x0, eps = (x - sb * v) / sa, v
        else:
            x0, eps = v, v
        if clip_sample:
            x0 = x0.clamp(-1, 1)
        if clipped_model_output:
            eps = (x - sa * x0) / sb
        nx = sap * x0 + sbp * eps
        if variance_noise is not None:
            nx = nx + sigma * variance_noise.reshape(B, c_latent, F, HW).float()
        x.copy_(nx)
