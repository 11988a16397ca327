"""The f64 specification of the sigma-space samplers - Euler, Euler ancestral, LMS (a helper, not a test module): the reference's formulas (diffusers 0.11.1,
scheduling_euler_discrete.py:195-253, scheduling_euler_ancestral_discrete.py:203-243, scheduling_lms_discrete.py:216-245) with every scalar taken at the f32 value
the reference forms - sigma^2 + 1, -sigma / (sigma^2 + 1) ** 0.5, dt, sigma_up, sigma_down in f32 tensor arithmetic, in its order; the LMS coefficients at the f64
values its quadrature returned (recorded in the golden file) - and every tensor in f64; and the kernel's form from the very inputs fyc_cfg_sigma_step gets.

The bound is solver_spec's: every function evaluates its formula twice, in f64 and with absolute values and additions (the pairs of P); an f32 evaluation whose
longest path makes K roundings differs from the exact value by at most gamma(K) S = ((1 + 2^-24)^K - 1) S.  The reference's epsilon derivative (x - (x - sigma v)) /
sigma cancels in f32: S holds |x| / sigma twice, and the collapsed form d = v, which does not cancel, sits inside the same bound.

LMS.  The engine integrates the Lagrange polynomials in closed form in f64; the reference's quadrature evaluates the integrand in f32 tensors - three factors of
four roundings each - so its coefficients sit up to LMS_COEF_UNITS x 2^-24 x max_k |c_k| from the exact ones (measured: at most 3.9).  That distance is held by its
own test; the trajectories are held to the plain gamma(K) S against the formula with the reference's coefficients.

The 2-D path.  The plain latents go through nchw_to_nhwc(scale = the f32 reciprocal of the denominator): the reciprocal is one rounding, the product another, against
the single rounding of the reference's division (K_PLAIN_INPUT, plain_input_reference below).
"""
import zlib
from collections import namedtuple

import numpy as np
import torch

import sampling_spec as SS
from solver_spec import P, gamma, inside  # noqa: F401

# The longest path of one output element through csrc/elementwise.hip::cfg_sigma_kernel, one f32 rounding each: guidance u - s1, * video_scale, s1 + ., + guidance (c - u)
# = 4 (sampling_spec.K_ROUNDINGS' first four); * factor = 5, the factor itself is a rounded number = 6; a_v is a rounded number = 7, a_v * v = 8, a_x x + . = 9.  For
# v_prediction the specification takes the reference's scalars: its f32 -sigma / (sigma^2 + 1) ** 0.5 carries three roundings (sigma^2 + 1, the root, the quotient;
# the square's is halved by the root) that the engine's a_v, formed in f64, does not share = 12 (its f32 sigma^2 + 1 under x is one rounding of a parallel, shorter
# branch).  This is d: K_D.  c_0 is a rounded number = 13, c_0 * d = 14, c_x x + . = 15, + c_1 d_1 = 16, + c_2 d_2 = 17, + c_3 d_3 = 18, + c_n noise = 19.  The drop-in's
# step() makes the same roundings without the guidance; a history entry it formed itself arrives with at most K_D roundings and leaves through a rounded c_k, its
# product and at most three sums: shorter.
K_KERNEL = 19
K_D = 12
# The same path where the coefficients are taken as given (kernel_step: the launches of the kernel tests hand over an f32 coef row, and the specification reads
# that row): the three roundings of the reference's v_prediction scalars do not occur, a_v and c_0 are still rounded numbers.  d = 9, x' = 16.
K_KERNEL_GIVEN = 16
K_D_GIVEN = 9
# nchw_to_nhwc with the f32 reciprocal: 1 / denom = 1, x * . = 2 (the rounding to a 16-bit storage type comes on top, as for the division)
K_PLAIN_INPUT = 2
# The reference's longest tensor path, LMS at order 4 with v_prediction: v * k_v = 1, + x / q = 2 (x0); x - x0 = 3, / sigma = 4 (the derivative); the coefficient, a
# python float, enters the f32 product rounded = 5, coeff * d = 6; sum() adds the four products (0 + . is exact) = 9; sample + . = 10.  The ancestral path (d = 4,
# d * dt = 5, x + . = 6, + noise * sigma_up = 7) and Euler's are shorter.
K_REFERENCE = 10
LMS_COEF_UNITS = 12

KINDS = ("euler", "euler_ancestral", "lms")
PREDICTIONS = ("epsilon", "v_prediction")


def timesteps(n, T=1000):
    return np.linspace(0, T - 1, n, dtype=float)[::-1].copy()


def derivative(pred, sigma, x, v):
    """(x - pred_original_sample) / sigma as the three step() methods form it -> P.  sigma: a 0-dim f32 tensor"""
    x, v = P(x), P(v)
    if pred == "epsilon":
        x0 = x - sigma * v
    else:
        x0 = (-sigma / (sigma ** 2 + 1) ** 0.5) * v + x.over(sigma ** 2 + 1)
    return (x - x0).over(sigma)


def schedule_step(kind, pred, sigmas, i, xs, vs, noise=None, lms_coeffs=None):
    """step i of a schedule from the samples xs[j] and model outputs vs[j] (f32) of the steps j <= i the order reaches back to -> (x' f64, S f64): the
    derivatives of the earlier steps are formed here in f64 from those steps' own inputs.  sigmas [n + 1] f32; noise: the ancestral step's; lms_coeffs: the
    reference's coefficients of this step (newest derivative first)"""
    x = P(xs[i])
    sg, sg_to = sigmas[i], sigmas[i + 1]
    d = derivative(pred, sg, xs[i], vs[i])
    if kind == "euler":
        out = x + (sg_to - sg) * d
        return out.v, out.a
    if kind == "euler_ancestral":
        sigma_up = (sg_to ** 2 * (sg ** 2 - sg_to ** 2) / sg ** 2) ** 0.5
        sigma_down = (sg_to ** 2 - sigma_up ** 2) ** 0.5
        out = x + (sigma_down - sg) * d + sigma_up * P(noise)
        return out.v, out.a
    ds = [d] + [derivative(pred, sigmas[i - k], xs[i - k], vs[i - k]) for k in range(1, len(lms_coeffs))]
    total = float(lms_coeffs[0]) * ds[0]
    for c, dk in zip(lms_coeffs[1:], ds[1:]):
        total = total + float(c) * dk
    out = x + total
    return out.v, out.a


# ---- the kernel's form: guidance, derivative and update from the very inputs fyc_cfg_sigma_step gets -------------------------------------------------------
def kernel_step(pred, latents, coef, *, B, F, HW, c_latent, ld, guidance, order=1, hist_1=None, hist_2=None, hist_3=None, noise=None, guidance_rescale=0.0,
                pred_single=None, video_scale=0.0, cfg=True):
    """-> (x' f64, its bound, d f64, its bound), all (B, c_latent, F, HW).  pred [cfg B F HW][ld] (uncond half first), latents / hist_* / noise (B, c_latent, F, HW)
    f32, coef f32[8] = {a_x, a_v, c_x, c_0, c_1, c_2, c_3, c_n} taken as given; guidance, video_scale, guidance_rescale at their f32 values"""
    f32 = lambda s: float(torch.tensor(s, dtype=torch.float32))      # noqa: E731
    g, vs, phi = f32(guidance), f32(video_scale), f32(guidance_rescale)
    p = SS._rows(pred, 2 if cfg else 1, B, F, HW, ld, c_latent)
    if not cfg:
        v = P(p[0])
    elif pred_single is not None:
        s1 = P(SS._rows(pred_single, 1, B, F, HW, ld, c_latent)[0])
        v = s1 + vs * (P(p[0]) - s1) + g * (P(p[1]) - P(p[0]))
    else:
        v = P(p[0]) + g * (P(p[1]) - P(p[0]))
    if phi > 0:
        factor = phi * p[1].std(dim=(1, 2, 3), keepdim=True) / v.v.std(dim=(1, 2, 3), keepdim=True) + (1 - phi)      # the per-sample factor
        v = P(SS.rescale_noise_cfg(p[1], v.v, phi), v.a * factor)
    v = P(v.v.permute(0, 3, 1, 2), v.a.permute(0, 3, 1, 2))                  # B C F HW
    shape = (B, c_latent, F, HW)
    x = P(latents.reshape(shape))
    ax, av, cx, c0, c1, c2, c3, cn = [float(t) for t in coef.reshape(-1)[:8]]
    d = ax * x + av * v
    out = cx * x + c0 * d
    for k, (c, h) in enumerate(((c1, hist_1), (c2, hist_2), (c3, hist_3)), start=2):
        if order >= k:
            out = out + c * P(h.reshape(shape))
    if noise is not None:
        out = out + cn * P(noise.reshape(shape))
    return out.v, gamma(K_KERNEL_GIVEN) * out.a, d.v, gamma(K_D_GIVEN) * d.a


# ---- the cases of the golden files (tools/make_golden_sigma.py writes them, tests/test_sigma.py reads them) ---------------------------------------------------
STEP_COUNTS = (4, 10, 25)
BETA_SETS = {"linear": dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear"),         # the shipped YAML's
             "scaled_linear": dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear"),      # Stable Diffusion's
             "zsnr": dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear")}          # + rescale_betas_zero_snr
LATENT_SHAPE = (2, 4, 3, 7)
Case = namedtuple("Case", ["betas", "kind", "prediction_type", "n"])


def golden_cases():
    return [Case(b, k, p, n) for b in BETA_SETS for k in KINDS for p in PREDICTIONS for n in STEP_COUNTS]


def case_key(case):
    return f"{case.betas}/{case.kind}/{case.prediction_type}/n{case.n}"


def case_inputs(case):
    """-> (initial latents LATENT_SHAPE f32 - unit noise, to be multiplied by init_noise_sigma -, one model output per step [n, *LATENT_SHAPE] f32, one noise tensor per
    step of the same shape (the ancestral kind's)), seeded by the case's array name"""
    g = torch.Generator().manual_seed(zlib.crc32(case_key(case).encode()))
    return torch.randn(LATENT_SHAPE, generator=g), torch.randn((case.n,) + LATENT_SHAPE, generator=g), torch.randn((case.n,) + LATENT_SHAPE, generator=g)


def case_samples(case, prev_samples, init_noise_sigma):
    """the sample of every step: the initial latents, then the reference's own previous output (nothing an implementation computes is carried along)"""
    x0 = case_inputs(case)[0] * init_noise_sigma
    return [x0] + [prev_samples[i] for i in range(case.n - 1)]


# ---- the cases of the kernel tests (tests/test_sigma.py on the emulator, tests/test_sigma_gpu.py on the MI355X) -----------------------------------------------
SHAPES = SS.SHAPES
SIGMA = 2.5                                                                                                  # a_x, a_v of the two prediction types at sigma = 2.5
CONVERT = {"epsilon": (0.0, 1.0), "v_prediction": (SIGMA / (SIGMA ** 2 + 1), 1 / (SIGMA ** 2 + 1) ** 0.5)}
UPDATE = (1.0, -1.31, 1.47, -0.93, 0.22, 0.71)                                                              # c_x, c_0 .. c_3, c_n: the magnitudes of a fourth-order LMS step, a mid-schedule sigma_up
ORDERS = (1, 2, 3, 4)
Variant = namedtuple("Variant", ["order", "noise", "single", "phi", "pred"])
VARIANTS = [Variant(o, n, s, phi, p) for o in ORDERS for n in (False, True) for s in (False, True) for phi in (0.0, 0.7) for p in PREDICTIONS]
GUIDANCE, VIDEO_SCALE = SS.GUIDANCE, SS.VIDEO_SCALE
_hist = {}


def coef_of(pred):
    return torch.tensor([*CONVERT[pred], *UPDATE], dtype=torch.float64).float()


def operands(shape, dt):
    """sampling_spec's seeded operands of a shape (its `noise` is the ancestral noise here) plus three history tensors (never written: every user clones what a
    launch writes)"""
    o = dict(SS.operands(shape, dt))
    if shape not in _hist:
        B, F, HW, CL, ld = shape
        g = torch.Generator().manual_seed(91 + 1000 * B + 10 * F + HW + ld)
        _hist[shape] = tuple(torch.randn(B, CL, F, HW, generator=g) for _ in range(3))
    o["hist_1"], o["hist_2"], o["hist_3"] = _hist[shape]
    return o


def step_kwargs(shape, var):
    """keyword arguments of cfg_sigma_step for a variant (without the tensors)"""
    B, F, HW, CL, ld = shape
    return dict(B=B, F=F, HW=HW, c_latent=CL, ld=ld, cfg=True, guidance=GUIDANCE, order=var.order, video_scale=VIDEO_SCALE if var.single else 0.0,
                guidance_rescale=var.phi)


def reference(shape, dt, var, coef=None):
    """-> (x', its bound, d, its bound), each [B c_latent][F HW] f64"""
    B, F, HW, CL, ld = shape
    o = operands(shape, dt)
    out = kernel_step(o["pred"], o["latents"], coef_of(var.pred) if coef is None else coef, hist_1=o["hist_1"], hist_2=o["hist_2"], hist_3=o["hist_3"],
                      noise=o["noise"] if var.noise else None, pred_single=o["single"] if var.single else None, **step_kwargs(shape, var))
    return tuple(t.reshape(B * CL, F * HW) for t in out)


def run_step(ops, shape, dt, var, *, on=lambda t: t, coef=None, hist=None, noise=None, store=True, pred=None):
    """one launch of cfg_sigma_step on clones of the shared operands -> (latents, hist_out), each [B c_latent][F HW]; hist_out starts full of NaN (store=False: it is
    not handed over and comes back as it was).  hist: what to hand over as (hist_1, hist_2, hist_3) instead of the operands' - the histories an order does not read are
    always handed over: the kernel must not touch them; noise: what to hand over as the noise of a variant WITHOUT noise (None = nothing)"""
    B, F, HW, CL, ld = shape
    o = operands(shape, dt)
    lat, out = on(o["latents"].clone()), on(torch.full((B, CL, F, HW), float("nan")))
    h = (o["hist_1"], o["hist_2"], o["hist_3"]) if hist is None else hist
    nz = o["noise"] if var.noise else noise
    ops.cfg_sigma_step(on(o["pred"] if pred is None else pred), lat, on(coef_of(var.pred) if coef is None else coef), hist_out=out if store else None,
                       hist_1=on(h[0]), hist_2=on(h[1]), hist_3=on(h[2]), noise=None if nz is None else on(nz),
                       pred_single=on(o["single"]) if var.single else None, **step_kwargs(shape, var))
    return lat.reshape(B * CL, F * HW), out.reshape(B * CL, F * HW)


# ---- fyc_unet_input_scaled -----------------------------------------------------------------------------------------------------------------------------------
INPUT_DENOM = 5.413011074066162          # sqrt(sigma^2 + 1) of a mid-schedule step, an f32 value
InputCase = namedtuple("InputCase", ["mode", "scale_cond", "cfg_dup", "with_mask"])
INPUT_CASES = [InputCase(0, 1, 2, True), InputCase(0, 0, 1, True), InputCase(0, 1, 1, False), InputCase(1, 0, 2, False)]
INPUT_SHAPES = [(2, 3, 20, 4, 16), (1, 5, 203, 4, 16), (2, 2, 37, 3, 8)]          # (B, F, HW, c_latent, c_pad): one block; rows no multiple of the block; three latent channels


def input_operands(shape):
    B, F, HW, CL, cp = shape
    g = torch.Generator().manual_seed(5 + 1000 * B + 10 * F + HW + cp)
    return dict(latents=torch.randn(B, CL, F, HW, generator=g) * 7.0, mask=torch.rand(B, 1, HW, generator=g) * 1.4 - 0.2, first=torch.randn(B, CL, HW, generator=g))


def input_reference(shape, case, denom):
    """the scaled UNet input in f64, [cfg_dup B F][HW][c_pad]: latents / denom; mode 0: the clamped mask and the first-frame block at frame 0, divided when scale_cond;
    mode 1: the first-frame latents beside every frame, never divided; pads 0.  One f32 division and one rounding to the storage type: |got - ref| <= (2^-24 + u) |ref|
    with u the storage type's unit roundoff (0 for f32 beyond the division's)"""
    B, F, HW, CL, cp = shape
    o = input_operands(shape)
    out = torch.zeros(B, F, HW, cp, dtype=torch.float64)
    out[..., :CL] = o["latents"].double().permute(0, 2, 3, 1) / denom
    cden = denom if case.scale_cond else 1.0
    if case.mode == 1:
        out[..., CL:2 * CL] = o["first"].double().reshape(B, 1, CL, HW).permute(0, 1, 3, 2)
    else:
        if case.with_mask:
            out[..., CL] = (o["mask"].double().reshape(B, 1, HW).clamp(0, 1) / cden).expand(B, F, HW)
        else:
            out[:, 0, :, CL] = 1.0 / cden
        out[:, 0, :, CL + 1:2 * CL + 1] = o["first"].double().permute(0, 2, 1) / cden
    return torch.cat([out] * case.cfg_dup, dim=0).reshape(case.cfg_dup * B * F, HW, cp)


def run_input(ops, shape, case, dtype, denom, *, on=lambda t: t, scaled=True):
    """one launch of unet_input_scaled (scaled=False: of unet_input) into a NaN-filled buffer -> x [cfg_dup B F][HW][c_pad]"""
    B, F, HW, CL, cp = shape
    o = input_operands(shape)
    x = on(torch.full((case.cfg_dup * B * F * HW, cp), float("nan"), dtype=dtype))
    kw = dict(B=B, F=F, HW=HW, c_latent=CL, c_pad=cp, cfg_dup=case.cfg_dup, mask_frames=1, mode=case.mode)
    mask = on(o["mask"]) if case.with_mask and case.mode == 0 else None
    if scaled:
        ops.unet_input_scaled(on(o["latents"]), mask, on(o["first"]), x, denom=denom, scale_cond=bool(case.scale_cond), **kw)
    else:
        ops.unet_input(on(o["latents"]), mask, on(o["first"]), x, **kw)
    return x.reshape(case.cfg_dup * B * F, HW, cp)


def plain_input_reference(shape, denom):
    """the 2-D path's UNet input in f64, [B F][HW][c_pad]: the plain latents / denom, pads 0.  An implementation that multiplies by the f32 reciprocal is held to
    (gamma(K_PLAIN_INPUT) + u) |ref| with u the storage type's unit roundoff"""
    B, F, HW, CL, cp = shape
    out = torch.zeros(B * F, HW, cp, dtype=torch.float64)
    out[..., :CL] = input_operands(shape)["latents"].double().permute(0, 2, 3, 1).reshape(B * F, HW, CL) / denom
    return out


def run_plain_input(ops, shape, dtype, denom, *, on=lambda t: t):
    """the launch DDIMSampler.predict makes for plain latents under a sigma-space scheduler: nchw_to_nhwc with scale = 1 / denom formed in f32 -> x [B F][HW][c_pad]"""
    B, F, HW, CL, cp = shape
    frames = input_operands(shape)["latents"].permute(0, 2, 1, 3).reshape(B * F, CL, HW).contiguous()
    x = on(torch.full((B * F * HW, cp), float("nan"), dtype=dtype))
    scale = float(torch.tensor(1.0) / torch.tensor(denom, dtype=torch.float32))
    ops.nchw_to_nhwc(on(frames), x, N=B * F, C_=CL, HW=HW, c_pad=cp, scale=scale)
    return x.reshape(B * F, HW, cp)
