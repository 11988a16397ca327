"""The CPU op emulator with the fused guidance + PNDM evaluation (fyc_cfg_pndm_step).  tests/emu_ops.py, tests/emu_ops_sampling.py, tests/emu_ops_solver.py and
tests/emu_ops_sigma.py stay as they are.  The guided (and rescaled) prediction is SamplingEmuOps', everything else is f32 in the order of the kernel
(csrc/elementwise.hip::cfg_pndm_kernel), and - as there - a buffer the call does not use is never read and an output not handed over is never written."""
import torch

from emu_ops import _flat
from emu_ops_sigma import SigmaEmuOps


class PNDMEmuOps(SigmaEmuOps):
    def cfg_pndm_step(self, pred, latents, coef, *, sample_in=None, sample_out=None, hist_out=None, hist_1=None, hist_2=None, hist_3=None, order=1, acc_in=None,
                      acc_out=None, B, F, HW, c_latent, ld, cfg, guidance, pred_single=None, video_scale=0.0, guidance_rescale=0.0):
        hists = (hist_1, hist_2, hist_3)
        assert order in (1, 2, 3, 4) and all(hists[k] is not None for k in range(order - 1)), order
        assert not 0.0 < guidance_rescale or cfg, "guidance rescale needs classifier-free guidance"
        assert pred_single is None or cfg
        assert sample_in is None or sample_in.data_ptr() != latents.data_ptr(), "sample_in aliases latents"
        outs = (sample_out, hist_out, acc_out)
        for k, w in enumerate(outs):
            for h in (latents, *hists, sample_in, acc_in, *outs[k + 1:]):
                assert w is None or h is None or h.data_ptr() != w.data_ptr() or (w is acc_out and h is acc_in), "an output aliases another buffer"
        if guidance_rescale > 0:
            g, _ = self.guided_rescaled(pred, B=B, F=F, HW=HW, c_latent=c_latent, ld=ld, guidance=guidance, guidance_rescale=guidance_rescale,
                                        pred_single=pred_single, video_scale=video_scale)
        else:
            p = _flat(pred)[: (2 if cfg else 1) * B * F * HW * ld].reshape(-1, B, F, HW, ld)[..., :c_latent].float()
            g = p[0] + guidance * (p[1] - p[0]) if cfg else p[0]
            if pred_single is not None:
                s1 = _flat(pred_single)[: B * F * HW * ld].reshape(B, F, HW, ld)[..., :c_latent].float()
                g = s1 + video_scale * (p[0] - s1) + guidance * (p[1] - p[0])
        g = g.permute(0, 3, 1, 2)                                  # B C F HW
        shape = (B, c_latent, F, HW)
        lat = latents.reshape(shape)
        if sample_out is not None:
            sample_out.reshape(shape).copy_(lat)
        x = lat if sample_in is None else sample_in.reshape(shape)
        cx, c0, c1, c2, c3, sg = [float(c) for c in coef.reshape(-1)[:6]]
        nx = cx * x + c0 * g
        for k, c in ((2, c1), (3, c2), (4, c3)):
            if order >= k:
                nx = nx + c * hists[k - 2].reshape(shape)
        lat.copy_(nx)
        if hist_out is not None:
            hist_out.reshape(shape).copy_(g)
        if acc_out is not None:
            acc_out.reshape(shape).copy_(sg * g if acc_in is None else acc_in.reshape(shape) + sg * g)
