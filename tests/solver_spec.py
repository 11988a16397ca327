"""The f64 specification of the DPM-Solver multistep scheduler (a helper, not a test module): the reference's formulas (diffusers 0.11.1,
scheduling_dpmsolver_multistep.py:234-280 convert_model_output, :304-426 the three updates, :462-489 the order rules) with every scalar taken at the
f32 value the reference forms - h, r0, exp(-h) - 1, (exp(-h) - 1) / h + 1, ... in f32 tensor arithmetic, in its order - and every tensor in f64.
With f64 scalars instead the reference itself sits up to 183 x 2^-24 S away: its f32 (exp(-h) - 1) / h + 1 cancels.

The bound.  Every function evaluates its formula twice: in f64, and with every value replaced by its absolute value and every subtraction by an
addition (the pairs of P below).  The second result S is the sum of the absolute values of all terms once D1, D2, the converted outputs and the
guided prediction are expanded down to the inputs.  An f32 evaluation whose longest path makes K roundings differs from the exact value by at
most ((1 + 2^-24)^K - 1) S (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; the divisions are by given scalars).
"""
import zlib
from collections import namedtuple

import torch

import sampling_spec as SS

# The longest path of one output element through csrc/elementwise.hip::cfg_solver_kernel, one f32 rounding each: guidance u - s1, * video_scale, s1 + ., + guidance (c - u) = 4
# (sampling_spec.K_ROUNDINGS); * factor = 5, and the factor itself is a rounded number = 6; a_v is a rounded number = 7, a_v * v = 8, a_x x + . = 9 (this is m0: K_M0);
# c_0 is a rounded number = 10, c_0 * m0 = 11, c_x x + . = 12, + c_1 m1 = 13, + c_2 m2 = 14.  The drop-in's step() makes the same roundings without the guidance; a history
# entry it formed itself arrives with 3 roundings and leaves through a rounded c_1, its product and at most two sums: shorter.
K_KERNEL = 14
K_M0 = 9
# The reference's longest tensor path, third order with epsilon prediction: conversion sigma_t * v, x - ., / alpha_t = 3; m0 - m1 = 4, (1 / r0) * . = 5 (D1_0; D1_1 in parallel);
# D1_0 - D1_1 = 6, (r0 / (r0 + r1)) * . = 7, D1_0 + . = 8 (D1); factor * D1 = 9; the sum ((c_x x - . D0) + . D1) = 10, - . D2 = 11.  The scalars are taken at their f32 values
# and cost nothing.  Every other family is a shorter path.
K_REFERENCE = 11


def gamma(k):
    return (1 + 2.0 ** -24) ** k - 1


class P:
    """a value in f64 together with the sum of the absolute values of the terms it was formed from"""

    def __init__(self, v, a=None):
        self.v = v.double()
        self.a = self.v.abs() if a is None else a

    def __add__(self, o):
        return P(self.v + o.v, self.a + o.a)

    def __sub__(self, o):
        return P(self.v - o.v, self.a + o.a)

    def __rmul__(self, c):          # c: a python float or a 0-dim tensor, taken at its value as f64
        c = float(c)
        return P(c * self.v, abs(c) * self.a)

    def over(self, c):
        c = float(c)
        return P(self.v / c, self.a / abs(c))


def timesteps(n, T=1000):
    import numpy as np
    return np.linspace(0, T - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)


def plan(n, solver_order, lower_order_final=True):
    """the order the reference's step() takes at every step (:462-489), replayed with its own variables"""
    orders, lower_order_nums = [], 0
    for step_index in range(n):
        final = (step_index == n - 1) and lower_order_final and n < 15
        second = (step_index == n - 2) and lower_order_final and n < 15
        if solver_order == 1 or lower_order_nums < 1 or final:
            orders.append(1)
        elif solver_order == 2 or lower_order_nums < 2 or second:
            orders.append(2)
        else:
            orders.append(3)
        if lower_order_nums < solver_order:
            lower_order_nums += 1
    return orders


def convert(tables, fam, t, x, v):
    """convert_model_output (:234-280) -> P"""
    a, s = tables["alpha_t"][t], tables["sigma_t"][t]
    x, v = P(x), P(v)
    if fam["algorithm_type"] == "dpmsolver++":
        return {"epsilon": lambda: (x - s * v).over(a), "sample": lambda: v, "v_prediction": lambda: a * x - s * v}[fam["prediction_type"]]()
    return {"epsilon": lambda: v, "sample": lambda: (x - a * v).over(s), "v_prediction": lambda: a * v + s * x}[fam["prediction_type"]]()


def update(tables, fam, ts, i, order, x, m):
    """the first / second / third order update (:304-426) of step i from the sample x (f32 tensor) and the converted outputs m = [m0, m1, m2] (P, newest first)
    -> P.  The scalars are 0-dim f32 tensors formed exactly as the reference's lines form them."""
    lam, al, sg = tables["lambda_t"], tables["alpha_t"], tables["sigma_t"]
    t, s0 = (0 if i == len(ts) - 1 else ts[i + 1]), ts[i]
    plus, heun = fam["algorithm_type"] == "dpmsolver++", fam["solver_type"] == "heun"
    x = P(x)
    lambda_t, lambda_s0 = lam[t], lam[s0]
    alpha_t, alpha_s0, sigma_t, sigma_s0 = al[t], al[s0], sg[t], sg[s0]
    h = lambda_t - lambda_s0
    if order == 1:
        if plus:
            return (sigma_t / sigma_s0) * x - (alpha_t * (torch.exp(-h) - 1.0)) * m[0]
        return (alpha_t / alpha_s0) * x - (sigma_t * (torch.exp(h) - 1.0)) * m[0]
    h_0 = lambda_s0 - lam[ts[i - 1]]
    r0 = h_0 / h
    if order == 2:
        D0, D1 = m[0], (1.0 / r0) * (m[0] - m[1])
        if plus and not heun:
            return (sigma_t / sigma_s0) * x - (alpha_t * (torch.exp(-h) - 1.0)) * D0 - (0.5 * (alpha_t * (torch.exp(-h) - 1.0))) * D1
        if plus:
            return (sigma_t / sigma_s0) * x - (alpha_t * (torch.exp(-h) - 1.0)) * D0 + (alpha_t * ((torch.exp(-h) - 1.0) / h + 1.0)) * D1
        if not heun:
            return (alpha_t / alpha_s0) * x - (sigma_t * (torch.exp(h) - 1.0)) * D0 - (0.5 * (sigma_t * (torch.exp(h) - 1.0))) * D1
        return (alpha_t / alpha_s0) * x - (sigma_t * (torch.exp(h) - 1.0)) * D0 - (sigma_t * ((torch.exp(h) - 1.0) / h - 1.0)) * D1
    h_1 = lam[ts[i - 1]] - lam[ts[i - 2]]
    r1 = h_1 / h
    D0 = m[0]
    D1_0, D1_1 = (1.0 / r0) * (m[0] - m[1]), (1.0 / r1) * (m[1] - m[2])
    D1 = D1_0 + (r0 / (r0 + r1)) * (D1_0 - D1_1)
    D2 = (1.0 / (r0 + r1)) * (D1_0 - D1_1)
    if plus:
        return ((sigma_t / sigma_s0) * x - (alpha_t * (torch.exp(-h) - 1.0)) * D0 + (alpha_t * ((torch.exp(-h) - 1.0) / h + 1.0)) * D1
                - (alpha_t * ((torch.exp(-h) - 1.0 + h) / h ** 2 - 0.5)) * D2)
    return ((alpha_t / alpha_s0) * x - (sigma_t * (torch.exp(h) - 1.0)) * D0 - (sigma_t * ((torch.exp(h) - 1.0) / h - 1.0)) * D1
            - (sigma_t * ((torch.exp(h) - 1.0 - h) / h ** 2 - 0.5)) * D2)


def schedule_step(tables, fam, ts, i, order, xs, vs):
    """step i of a schedule from the samples xs[j] and model outputs vs[j] (f32) of the steps j <= i that the order reaches back to -> (x' f64, S f64): the converted
    outputs of the earlier steps are formed here in f64 from those steps' own inputs, so a history an f32 implementation kept in f32 is part of the judged path"""
    m = [convert(tables, fam, ts[i - k], xs[i - k], vs[i - k]) for k in range(order)]
    out = update(tables, fam, ts, i, order, xs[i], m)
    return out.v, out.a


# ---- the kernel's form: guidance, conversion and update from the very inputs fyc_cfg_solver_step gets ---------------------------------------------------
def kernel_step(pred, latents, coef, *, B, F, HW, c_latent, ld, guidance, order, hist_1=None, hist_2=None, guidance_rescale=0.0, pred_single=None,
                video_scale=0.0, cfg=True):
    """-> (x' f64, its bound, m0 f64, its bound), all (B, c_latent, F, HW).  pred [cfg B F HW][ld] (uncond half first), latents / hist_* (B, c_latent, F, HW) f32,
    coef f32[8] = {a_x, a_v, c_x, c_0, c_1, c_2, -, -} taken as given; guidance, video_scale, guidance_rescale at their f32 values"""
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
    x = P(latents.reshape(B, c_latent, F, HW))
    ax, av, cx, c0, c1, c2 = [float(t) for t in coef.reshape(-1)[:6]]
    m0 = ax * x + av * v
    out = cx * x + c0 * m0
    if order >= 2:
        out = out + c1 * P(hist_1.reshape(B, c_latent, F, HW))
    if order == 3:
        out = out + c2 * P(hist_2.reshape(B, c_latent, F, HW))
    return out.v, gamma(K_KERNEL) * out.a, m0.v, gamma(K_M0) * m0.a


# ---- the cases of the golden file (tools/make_golden_solver.py writes it, tests/test_solver.py reads it) --------------------------------------------
ALGORITHMS, ORDERS, SOLVER_TYPES = ("dpmsolver++", "dpmsolver"), (1, 2, 3), ("midpoint", "heun")
PREDICTIONS, STEP_COUNTS = ("epsilon", "v_prediction", "sample"), (4, 10, 25)
BETAS = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear")      # the shipped YAML's
LATENT_SHAPE = (2, 4, 3, 7)
Case = namedtuple("Case", ["betas", "algorithm_type", "solver_order", "solver_type", "prediction_type", "n"])


def golden_cases():
    """every family x n on the plain betas, then dpmsolver++ with v_prediction / sample on the zero-terminal-SNR betas (the rest is NaN there, in the reference too)"""
    plain = [Case("plain", a, o, s, p, n) for a in ALGORITHMS for o in ORDERS for s in SOLVER_TYPES for p in PREDICTIONS for n in STEP_COUNTS]
    return plain + [Case("zsnr", "dpmsolver++", o, s, p, n) for o in ORDERS for s in SOLVER_TYPES for p in ("v_prediction", "sample") for n in STEP_COUNTS]


def family(case):
    return dict(algorithm_type=case.algorithm_type, solver_order=case.solver_order, solver_type=case.solver_type, prediction_type=case.prediction_type)


def case_key(case):
    """the array name of a case in the golden file.  A first-order solver never reads solver_type: the generator checks that the reference's heun and midpoint
    runs are the same bits and stores them once, under midpoint"""
    stype = "midpoint" if case.solver_order == 1 else case.solver_type
    return f"{case.betas}/{case.algorithm_type}/o{case.solver_order}/{stype}/{case.prediction_type}/n{case.n}"


def case_inputs(case):
    """-> (initial latents LATENT_SHAPE f32, one model output per step [n, *LATENT_SHAPE] f32), seeded by the case's array name"""
    g = torch.Generator().manual_seed(zlib.crc32(case_key(case).encode()))
    return torch.randn(LATENT_SHAPE, generator=g), torch.randn((case.n,) + LATENT_SHAPE, generator=g)


def case_samples(case, prev_samples):
    """the sample of every step: the initial latents, then the reference's own previous output (nothing an implementation computes is carried along)"""
    x0, _ = case_inputs(case)
    return [x0] + [prev_samples[i] for i in range(case.n - 1)]


# ---- the cases of the kernel tests (tests/test_solver.py on the emulator, tests/test_solver_gpu.py on the MI355X) ------------------------------------
SHAPES = SS.SHAPES
ALPHA, SIGMA = 0.6, 0.8                                                                                    # a_x, a_v of the three prediction types at alpha_t = 0.6 (dpmsolver++)
CONVERT = {"epsilon": (1 / ALPHA, -SIGMA / ALPHA), "v_prediction": (ALPHA, -SIGMA), "sample": (0.0, 1.0)}
UPDATE = (0.83, 0.47, -0.21, 0.06)                                                                         # c_x, c_0, c_1, c_2: the magnitudes of a third-order step of a 25-step schedule
Variant = namedtuple("Variant", ["order", "single", "phi", "pred"])
VARIANTS = [Variant(o, s, phi, PREDICTIONS[k % 3]) for k, (o, s, phi) in
            enumerate((o, s, phi) for o in ORDERS for s in (False, True) for phi in (0.0, 0.7))]
GUIDANCE, VIDEO_SCALE = SS.GUIDANCE, SS.VIDEO_SCALE
_hist = {}


def coef_of(pred):
    return torch.tensor([*CONVERT[pred], *UPDATE, 0.0, 0.0], dtype=torch.float64).float()


def operands(shape, dt):
    """sampling_spec's seeded operands of a shape plus two history tensors (never written: every user clones what a launch writes)"""
    o = dict(SS.operands(shape, dt))
    if shape not in _hist:
        B, F, HW, CL, ld = shape
        g = torch.Generator().manual_seed(77 + 1000 * B + 10 * F + HW + ld)
        _hist[shape] = (torch.randn(B, CL, F, HW, generator=g), torch.randn(B, CL, F, HW, generator=g))
    o["hist_1"], o["hist_2"] = _hist[shape]
    return o


def step_kwargs(shape, var):
    """keyword arguments of cfg_solver_step for a variant (without the tensors)"""
    B, F, HW, CL, ld = shape
    return dict(B=B, F=F, HW=HW, c_latent=CL, ld=ld, cfg=True, guidance=GUIDANCE, order=var.order, video_scale=VIDEO_SCALE if var.single else 0.0,
                guidance_rescale=var.phi)


def reference(shape, dt, var, coef=None):
    """-> (x', its bound, m0, its bound), each [B c_latent][F HW] f64"""
    B, F, HW, CL, ld = shape
    o = operands(shape, dt)
    out = kernel_step(o["pred"], o["latents"], coef_of(var.pred) if coef is None else coef, hist_1=o["hist_1"], hist_2=o["hist_2"],
                      pred_single=o["single"] if var.single else None, **step_kwargs(shape, var))
    return tuple(t.reshape(B * CL, F * HW) for t in out)


def run_step(ops, shape, dt, var, *, on=lambda t: t, coef=None, hist=None, phi=None):
    """one launch of cfg_solver_step on clones of the shared operands -> (latents, hist_out), each [B c_latent][F HW].  hist: what to hand over as (hist_1, hist_2)
    instead of the operands' (the histories an order does not read are always handed over: the kernel must not touch them)"""
    B, F, HW, CL, ld = shape
    o = operands(shape, dt)
    lat, out = on(o["latents"].clone()), on(torch.full((B, CL, F, HW), float("nan")))
    h1, h2 = (o["hist_1"], o["hist_2"]) if hist is None else hist
    kw = step_kwargs(shape, var)
    if phi is not None:
        kw["guidance_rescale"] = phi
    ops.cfg_solver_step(on(o["pred"]), lat, on(coef_of(var.pred) if coef is None else coef), hist_out=out, hist_1=on(h1), hist_2=on(h2),
                        pred_single=on(o["single"]) if var.single else None, **kw)
    return lat.reshape(B * CL, F * HW), out.reshape(B * CL, F * HW)


def inside(got, ref, bound, tag):
    """asserts finite and every element within its bound -> the worst |got - ref| / bound"""
    g = got.detach().cpu().double()
    assert torch.isfinite(g).all(), f"{tag}: non-finite values"
    ratio = (g - ref).abs() / bound
    worst = ratio.max().item()
    assert worst <= 1.0, f"{tag}: element {int(ratio.argmax())} is {worst:.3f} x its bound ({g.reshape(-1)[ratio.argmax()]} vs {ref.reshape(-1)[ratio.argmax()]})"
    return worst
