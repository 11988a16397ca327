"""The f64 specification of the zero-SNR sampling additions (a helper, not a test module): timestep spacings as later diffusers computes them, diffusers'
rescale_noise_cfg, and the guided + rescaled DDIM step from the very inputs the kernel gets - with the bound its f32 evaluation is held to.

The bound.  guided_step() evaluates the step twice: in f64, and with every value replaced by its absolute value and every subtraction by an addition.  The
second result S is the sum of the absolute values of all terms of  sap x0 + sbp eps (+ sigma noise)  once x0, eps and the guided, rescaled prediction are
expanded down to the kernel's inputs.  An f32 evaluation whose longest path makes K roundings differs from the exact value by at most ((1 + 2^-24)^K - 1) S
(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; a clamp is 1-Lipschitz and adds nothing; the divisions are by the given coefficients).
K_ROUNDINGS counts the longest path of csrc/elementwise.hip::cfg_ddim_row.
"""
from collections import namedtuple

import numpy as np
import torch

SPACINGS = ("leading", "trailing", "linspace")


def timesteps(spacing, n, T=1000, offset=0):
    """-> int64 array, descending.  leading: diffusers 0.11.1 (the reference); trailing / linspace: later diffusers, no steps_offset"""
    if spacing == "leading":
        return (np.arange(0, n) * (T // n))[::-1].astype(np.int64) + offset
    if spacing == "trailing":
        return (np.round(np.arange(T, 0, -T / n)) - 1).astype(np.int64)
    if spacing == "linspace":
        return np.round(np.linspace(0, T - 1, n))[::-1].astype(np.int64)
    raise ValueError(spacing)


def rescale_noise_cfg(cond, guided, phi):
    """diffusers' rescale_noise_cfg (arXiv:2305.08891 section 3.4): unbiased std over all but the batch axis"""
    dims = tuple(range(1, cond.dim()))
    s_text, s_cfg = cond.std(dim=dims, keepdim=True), guided.std(dim=dims, keepdim=True)
    return phi * (guided * (s_text / s_cfg)) + (1 - phi) * guided


# The longest path of one output element through cfg_ddim_row, one f32 rounding each: u - s1, * video_scale, s1 + ., + guidance (c - u) [the sum; c - u and its product
# are a shorter parallel branch] = 4; * factor = 5, and the factor itself is a rounded number = 6; epsilon prediction: sb * v, x - ., / sa = 9; use_clipped_model_output:
# sa * x0, x - ., / sb = 12; sbp * eps, sap x0 + . = 14; + sigma * noise = 15.  Every other combination of options is a shorter path.
K_ROUNDINGS = 15


def _rows(pred, halves, B, F, HW, ld, c_latent):
    return pred.reshape(-1)[: halves * B * F * HW * ld].reshape(halves, B, F, HW, ld)[..., :c_latent].double()


def guided_step(pred, latents, coef, *, B, F, HW, c_latent, ld, guidance, pred_type, clip_sample, guidance_rescale, pred_single=None,
                video_scale=0.0, variance_noise=None, sigma=0.0, clipped_model_output=False):
    """-> (new latents [B][c_latent][F][HW] f64, bound of the same shape, guided rescaled prediction [B][c_latent][F][HW] f64).  pred: the stored predictions
    [2 B F HW][ld] (uncond half first), latents (B, c_latent, F, HW) f32, coef f32[4]; guidance, video_scale, guidance_rescale, sigma are taken at their f32 values"""
    f32 = lambda s: float(torch.tensor(s, dtype=torch.float32))      # noqa: E731
    g, vs, phi, sg = f32(guidance), f32(video_scale), f32(guidance_rescale), f32(sigma)
    p = _rows(pred, 2, B, F, HW, ld, c_latent)
    u, c = p[0], p[1]
    if pred_single is not None:
        s1 = _rows(pred_single, 1, B, F, HW, ld, c_latent)[0]
        v = s1 + vs * (u - s1) + g * (c - u)
        va = s1.abs() + abs(vs) * (u.abs() + s1.abs()) + abs(g) * (c.abs() + u.abs())
    else:
        v = u + g * (c - u)
        va = u.abs() + abs(g) * (c.abs() + u.abs())
    if phi > 0:
        va = va * (phi * c.std(dim=(1, 2, 3), keepdim=True) / v.std(dim=(1, 2, 3), keepdim=True) + (1 - phi))      # the per-sample factor
        v = rescale_noise_cfg(c, v, phi)
    v, va = v.permute(0, 3, 1, 2), va.permute(0, 3, 1, 2)                                  # B C F HW
    x = latents.reshape(B, c_latent, F, HW).double()
    xa = x.abs()
    sa, sb, sap, sbp = [float(t) for t in coef.reshape(-1)[:4]]
    if pred_type == 1:
        x0, eps = sa * x - sb * v, sa * v + sb * x
        x0a, epsa = sa * xa + sb * va, sa * va + sb * xa
    elif pred_type == 0:
        x0, eps = (x - sb * v) / sa, v
        x0a, epsa = (xa + sb * va) / sa, va
    else:
        x0, eps, x0a, epsa = v, v, va, va
    if clip_sample:
        x0 = x0.clamp(-1, 1)
    if clipped_model_output:
        eps, epsa = (x - sa * x0) / sb, (xa + sa * x0a) / sb
    nx, S = sap * x0 + sbp * eps, abs(sap) * x0a + abs(sbp) * epsa
    if variance_noise is not None:
        n = variance_noise.reshape(B, c_latent, F, HW).double()
        nx, S = nx + sg * n, S + abs(sg) * n.abs()
    return nx, ((1 + 2.0 ** -24) ** K_ROUNDINGS - 1) * S, v


# ---- the cases of the kernel tests (tests/test_sampling.py on the emulator, tests/test_sampling_gpu.py on the MI355X) --------------------------------
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
# (B, F, HW, c_latent, ld): one block covers a sample; rows no multiple of any block size and B = 1; a sample spans 17 partials of 1024 rows, a prime row count;
# three latent channels in rows of five: the scalar loads of the moments pass (the other shapes take one vector load per row)
SHAPES = [(2, 3, 20, 4, 8), (1, 5, 203, 4, 8), (2, 16, 1031, 4, 16), (2, 2, 37, 3, 5)]
PAD = 1.0e4            # what the pad channels of the ld-strided rows hold: a kernel that counts them is far off
Variant = namedtuple("Variant", ["pred_type", "phi", "single", "noise", "clip"])
VARIANTS = ([Variant(pt, phi, single, False, False) for pt in (0, 1, 2) for phi in (0.7, 1.0) for single in (False, True)]
            + [Variant(1, 0.7, False, True, False), Variant(0, 0.7, True, True, True)])      # eta > 0; the longest path: epsilon, single, clip + re-derived eps, noise
COEF = (0.6, 0.8, 0.8, 0.6)
GUIDANCE, VIDEO_SCALE, SIGMA = 8.0, 0.3, 0.25

_cache = {}


def operands(shape, dt):
    """seeded operands of a shape in a storage type, built once and shared (never written: every user clones the latents)"""
    key = (shape, dt)
    if key not in _cache:
        B, F, HW, CL, ld = shape
        g = torch.Generator().manual_seed(1000 * B + 10 * F + HW + ld)
        rows = B * F * HW
        pred = torch.full((2 * rows, ld), PAD)
        pred[:, :CL] = torch.randn(2 * rows, CL, generator=g)
        pred[rows:, :CL] = pred[:rows, :CL] + 0.2 * torch.randn(rows, CL, generator=g) + 0.05      # the conditional half: near the unconditional one, shifted
        single = torch.full((rows, ld), PAD)
        single[:, :CL] = torch.randn(rows, CL, generator=g)
        _cache[key] = dict(pred=pred.to(DT[dt]), single=single.to(DT[dt]), latents=torch.randn(B, CL, F, HW, generator=g),
                           noise=torch.randn(B, CL, F, HW, generator=g), coef=torch.tensor(COEF, dtype=torch.float32))
    return _cache[key]


def step_kwargs(shape, var):
    """keyword arguments of cfg_ddim_step(_rescaled) for a variant (without guidance_rescale)"""
    B, F, HW, CL, ld = shape
    return dict(B=B, F=F, HW=HW, c_latent=CL, ld=ld, cfg=True, guidance=GUIDANCE, pred_type=var.pred_type, clip_sample=var.clip,
                clipped_model_output=var.clip, video_scale=VIDEO_SCALE if var.single else 0.0, sigma=SIGMA if var.noise else 0.0)


def reference(shape, dt, var):
    """-> (latents after the step, bound), both [B c_latent][F HW] f64"""
    B, F, HW, CL, ld = shape
    o, kw = operands(shape, dt), step_kwargs(shape, var)
    del kw["cfg"]
    nx, bound, _ = guided_step(o["pred"], o["latents"], o["coef"], guidance_rescale=var.phi, pred_single=o["single"] if var.single else None,
                               variance_noise=o["noise"] if var.noise else None, **kw)
    return nx.reshape(B * CL, F * HW), bound.reshape(B * CL, F * HW)
