"""The CPU op emulator with the fused guidance + DPM-Solver multistep step (fyc_cfg_solver_step).  tests/emu_ops.py and tests/emu_ops_sampling.py stay as they
are.  The guided (and rescaled) prediction is SamplingEmuOps', everything else is f32 in the order of the kernel (csrc/elementwise.hip::cfg_solver_kernel), and - as
there - a history buffer the order does not use is never read."""
import torch

from emu_ops import _flat
from emu_ops_sampling import SamplingEmuOps


class SolverEmuOps(SamplingEmuOps):
    def cfg_solver_step(self, pred, latents, coef, *, hist_out, hist_1=None, hist_2=None, order, B, F, HW, c_latent, ld, cfg, guidance, pred_single=None,
                        video_scale=0.0, guidance_rescale=0.0):
        assert order in (1, 2, 3) and (order < 2 or hist_1 is not None) and (order < 3 or hist_2 is not None), order
        assert not 0.0 < guidance_rescale or cfg, "guidance rescale needs classifier-free guidance"
        assert pred_single is None or cfg
        for h in (latents, hist_1, hist_2):
            assert h is None or h.data_ptr() != hist_out.data_ptr(), "hist_out aliases another buffer"
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
        x = latents.reshape(B, c_latent, F, HW)
        ax, av, cx, c0, c1, c2 = [float(c) for c in coef.reshape(-1)[:6]]
        m0 = ax * x + av * v
        nx = cx * x + c0 * m0
        if order >= 2:
            nx = nx + c1 * hist_1.reshape(B, c_latent, F, HW)
        if order == 3:
            nx = nx + c2 * hist_2.reshape(B, c_latent, F, HW)
        x.copy_(nx)
        hist_out.reshape(B, c_latent, F, HW).copy_(m0)
