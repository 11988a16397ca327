"""The f64 specification of the PNDM scheduler, PLMS mode (skip_prk_steps) and Runge-Kutta mode (a helper, not a test module): the reference's formulas (diffusers 0.11.1,
scheduling_pndm.py:153-187 set_timesteps, :223-276 step_prk, :278-343 step_plms, :358-399 _get_prev_sample) with every scalar taken at the f32 value the reference
forms - 1 - alpha_prod, alpha_prod ** 0.5, (alpha_prod_t_prev / alpha_prod_t) ** 0.5, the denominator of formula (9), alpha_prod_t_prev - alpha_prod_t in f32 tensor
arithmetic, in its order - and every tensor in f64; and the kernel's form from the very inputs fyc_cfg_pndm_step gets.

The bound is solver_spec's: every function evaluates its formula twice, in f64 and with absolute values and additions (the pairs of P); an f32 evaluation whose
longest path makes K roundings differs from the exact value by at most gamma(K) S = ((1 + 2^-24)^K - 1) S.

The schedule here is restated from the reference's state machine on its own (counter, ets, cur_sample, cur_model_output as indices of evaluations), not taken from
engine/scheduler.py::PNDMTables.plan: the two are compared in tests/test_pndm.py.
"""
import zlib
from collections import namedtuple

import numpy as np
import torch

import sampling_spec as SS
from solver_spec import P, gamma, inside  # noqa: F401

# ---- rounding counts, one f32 rounding each --------------------------------------------------------------------------------------------------------------
# The reference's longest tensor path, a fourth-order PLMS step with v_prediction: 55 e_1 = 1, - 59 e_2 = 2 (its product is a parallel branch), + 37 e_3 = 3, - 9 e_4
# = 4; the python scalar 1 / 24 enters the f32 product rounded = 5, (1 / 24) * . = 6; the conversion alpha ** 0.5 * e' = 7, + beta ** 0.5 * x = 8 (the scalars are
# taken at their f32 values and cost nothing); (alpha_prev - alpha) * . = 9, / denominator = 10, sample_coeff * x - . = 11.  The last Runge-Kutta evaluation is
# shorter: 1 / 6 rounded = 1, * e = 2, + 1/3 e_2 = 3, + 1/3 e_3 = 4, + 1/6 e_4 = 5, then the same six.
K_REFERENCE = 11
# The scalars of formula (9) the reference forms in f32 and the engine, collapsing in f64 from the same f32 table entries, does not share.  On the model-output term:
# alpha_prev - alpha = 1; the denominator alpha sqrt(beta_prev) + sqrt(alpha beta alpha_prev): beta_prev = 1, its root = 2 (the root halves what it is handed: 1.5),
# alpha * . = 3 beside beta = 1, alpha beta = 2, * alpha_prev = 3, the root = 3 (2.5), and the sum of the two positive terms = 4; v_prediction's alpha ** 0.5 = 1: SCALARS_E
# = 6.  On the sample term: sample_coeff = quotient and root = 2; v_prediction adds k sqrt(beta) x with the first five above and beta = 1, its root = 2: SCALARS_X = 7.
K_SCALARS_E = 6
K_SCALARS_X = 7
# The longest path of one output element through csrc/elementwise.hip::cfg_pndm_kernel against the reference's formulas.  Guidance u - s1, * video_scale, s1 + ., + guidance
# (c - u) = 4 (sampling_spec.K_ROUNDINGS' first four); * factor = 5, the factor itself is a rounded number = 6: this is g, K_G.
# A PLMS evaluation: c_0 stands for scalars that carry K_SCALARS_E = 12, is itself a rounded number = 13, c_0 * g = 14; c_x x (K_SCALARS_X, rounded, product = 9) is the
# shorter branch; c_x x + . = 15, + c_1 h_1 = 16, + c_2 h_2 = 17, + c_3 h_3 = 18.
# The last Runge-Kutta evaluation reads the accumulator as h_1: g = 6, s_g is a rounded number = 7, s_g g = 8 (0 + . is exact), + s_g g of the second evaluation = 9, of
# the third = 10; c_1 stands for K_SCALARS_E = 16, is a rounded number = 17, c_1 * acc = 18, the last sum = 19.  This is the longest: K_KERNEL.
# The drop-in's step() makes the same roundings without the guidance.
K_G = 6
K_KERNEL = 19
# The same paths where the coefficient row is taken as given (kernel_step: the launches of the kernel tests hand over an f32 coef row and the specification reads that
# very row, so no coefficient is a rounded number): g = 6, c_0 g = 7, c_x x + . = 8, + c_1 h_1 = 9, + c_2 h_2 = 10, + c_3 h_3 = 11; the accumulator: s_g g = 7, acc_in + . = 8.
K_KERNEL_GIVEN = 11
K_ACC_GIVEN = 8

MODES = ("plms", "prk")
PREDICTIONS = ("epsilon", "v_prediction")

# one evaluation as the reference's step() sees it: kind (below), the pair (timestep, prev_timestep) handed to _get_prev_sample, src = the evaluation whose INPUT sample
# is stepped from, terms = the evaluations whose model outputs are combined, in the order of the reference's formula
Eval = namedtuple("Eval", ["kind", "timestep", "prev_timestep", "src", "terms"])


def split_timesteps(mode, n, T=1000, offset=0):
    """set_timesteps (:162-185) -> (prk_timesteps, plms_timesteps)"""
    base = (np.arange(0, n) * (T // n)).round()
    base += offset
    if mode == "plms":
        return np.array([]), np.concatenate([base[:-1], base[-2:-1], base[-1:]])[::-1].copy()
    prk = np.array(base[-4:]).repeat(2) + np.tile(np.array([0, T // n // 2]), 4)
    return (prk[:-1].repeat(2)[1:-1])[::-1].copy(), base[:-3][::-1].copy()


def timesteps(mode, n, T=1000, offset=0):
    return np.concatenate(split_timesteps(mode, n, T, offset)).astype(np.int64)


def schedule(mode, n, T=1000, offset=0):
    """step() / step_prk() / step_plms() run over the timestep list with evaluation indices in place of tensors -> [Eval]"""
    prk, _ = split_timesteps(mode, n, T, offset)
    ts, ratio = timesteps(mode, n, T, offset).tolist(), T // n
    ets, cur, out = [], None, []
    for counter, t in enumerate(ts):
        if counter < len(prk) and mode == "prk":
            prev_t, t = t - (0 if counter % 2 else ratio // 2), int(prk[counter // 4 * 4])
            if counter % 4 == 0:
                ets.append(counter)
                cur = counter
            if counter % 4 == 3:
                out.append(Eval("prk_last", t, prev_t, cur, (counter - 3, counter - 2, counter - 1, counter)))
            else:
                out.append(Eval("single", t, prev_t, cur, (counter,)))
            continue
        prev_t = t - ratio
        if counter != 1:
            ets = ets[-3:] + [counter]
        else:
            prev_t, t = t, t + ratio
        if len(ets) == 1 and counter == 0:
            cur = counter
            out.append(Eval("single", t, prev_t, counter, (counter,)))
        elif len(ets) == 1 and counter == 1:
            out.append(Eval("redo", t, prev_t, cur, (counter, ets[-1])))
            cur = None
        else:
            out.append(Eval(f"plms{len(ets)}", t, prev_t, counter, tuple(ets[::-1])))
    return out


def prev_sample(alphas_cumprod, final_alpha_cumprod, pred, x, t, prev_t, m):
    """_get_prev_sample (:371-397) on pairs.  alphas_cumprod: the f32 table, indexed as the reference indexes it (0-dim f32 tensors)"""
    a_t = alphas_cumprod[t]
    a_p = alphas_cumprod[prev_t] if prev_t >= 0 else final_alpha_cumprod
    b_t, b_p = 1 - a_t, 1 - a_p
    if pred == "v_prediction":
        m = (a_t ** 0.5) * m + (b_t ** 0.5) * x
    sample_coeff = (a_p / a_t) ** 0.5
    denom = a_t * b_p ** 0.5 + (a_t * b_t * a_p) ** 0.5
    return sample_coeff * x - ((a_p - a_t) * m).over(denom)


def schedule_eval(alphas_cumprod, final_alpha_cumprod, pred, ev, xs, vs):
    """one evaluation from the input samples xs[j] and the model outputs vs[j] (f32) of the evaluations it reaches back to -> (x' f64, S f64)"""
    x, e = P(xs[ev.src]), [P(vs[j]) for j in ev.terms]
    if ev.kind == "single":
        m = e[0]
    elif ev.kind == "redo":
        m = (e[0] + e[1]).over(2)
    elif ev.kind == "plms2":
        m = (3 * e[0] - e[1]).over(2)
    elif ev.kind == "plms3":
        m = (23 * e[0] - 16 * e[1] + 5 * e[2]).over(12)
    elif ev.kind == "plms4":
        m = (1 / 24) * (55 * e[0] - 59 * e[1] + 37 * e[2] - 9 * e[3])
    else:               # cur_model_output = 1/6 e_1 + 1/3 e_2 + 1/3 e_3, then + 1/6 e_4
        m = (1 / 6) * e[0] + (1 / 3) * e[1] + (1 / 3) * e[2] + (1 / 6) * e[3]
    out = prev_sample(alphas_cumprod, final_alpha_cumprod, pred, x, ev.timestep, ev.prev_timestep, m)
    return out.v, out.a


# ---- the kernel's form: guidance and update from the very inputs fyc_cfg_pndm_step gets ------------------------------------------------------------------------
_guided = {}


def guided(pred, *, B, F, HW, c_latent, ld, guidance, guidance_rescale=0.0, pred_single=None, video_scale=0.0, cfg=True, key=None):
    """the guided (and rescaled) prediction -> P (B, c_latent, F, HW); key: cache the result under it (the operands of the kernel cases are shared)"""
    if key is not None and key in _guided:
        return _guided[key]
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
    if key is not None:
        _guided[key] = v
    return v


def kernel_step(pred, latents, coef, *, B, F, HW, c_latent, ld, guidance, order=1, sample_in=None, hist_1=None, hist_2=None, hist_3=None, acc_in=None,
                guidance_rescale=0.0, pred_single=None, video_scale=0.0, cfg=True, key=None):
    """-> dict of (value f64, bound) pairs, all (B, c_latent, F, HW): lat (x'), hist (g), acc (acc_in + s_g g; acc_in None = 0); sample_out is a copy of the latents as
    they were and is compared bit for bit.  pred [cfg B F HW][ld] (uncond half first), the other tensors (B, c_latent, F, HW) f32, coef f32[6] = {c_x, c_0, c_1, c_2, c_3, s_g} taken as given"""
    g = guided(pred, B=B, F=F, HW=HW, c_latent=c_latent, ld=ld, guidance=guidance, guidance_rescale=guidance_rescale, pred_single=pred_single,
               video_scale=video_scale, cfg=cfg, key=key)
    shape = (B, c_latent, F, HW)
    x = P((latents if sample_in is None else sample_in).reshape(shape))
    cx, c0, c1, c2, c3, sg = [float(t) for t in coef.reshape(-1)[:6]]
    out = cx * x + c0 * g
    for k, (c, h) in enumerate(((c1, hist_1), (c2, hist_2), (c3, hist_3)), start=2):
        if order >= k:
            out = out + c * P(h.reshape(shape))
    acc = sg * g if acc_in is None else P(acc_in.reshape(shape)) + sg * g
    return dict(lat=(out.v, gamma(K_KERNEL_GIVEN) * out.a), hist=(g.v, gamma(K_G) * g.a), acc=(acc.v, gamma(K_ACC_GIVEN) * acc.a))


# ---- the cases of the golden files (tools/make_golden_pndm.py writes them, tests/test_pndm.py reads them) ------------------------------------------------------
STEP_COUNTS = (4, 10, 25)
STEPS_OFFSET = 1                # Stable Diffusion's, and what both pipelines patch an outdated config to
BETA_SETS = {"linear": dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear"),         # the shipped YAML's
             "scaled_linear": dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear"),      # Stable Diffusion's
             "zsnr": dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear")}          # + rescale_betas_zero_snr
LATENT_SHAPE = (2, 4, 3, 7)
Case = namedtuple("Case", ["betas", "mode", "prediction_type", "n"])


def golden_cases():
    return [Case(b, m, p, n) for b in BETA_SETS for m in MODES for p in PREDICTIONS for n in STEP_COUNTS]


def case_key(case):
    return f"{case.betas}/{case.mode}/{case.prediction_type}/n{case.n}"


def evaluations(case):
    return case.n + (1 if case.mode == "plms" else 9)


def case_inputs(case):
    """-> (initial latents LATENT_SHAPE f32, one model output per evaluation [n + 1 or n + 9, *LATENT_SHAPE] f32), seeded by the case's array name"""
    g = torch.Generator().manual_seed(zlib.crc32(case_key(case).encode()))
    return torch.randn(LATENT_SHAPE, generator=g), torch.randn((evaluations(case),) + LATENT_SHAPE, generator=g)


def case_samples(case, prev_samples):
    """the input sample of every evaluation: the initial latents, then the reference's own previous output (nothing an implementation computes is carried along)"""
    return [case_inputs(case)[0]] + [prev_samples[i] for i in range(evaluations(case) - 1)]


# ---- the cases of the kernel tests (tests/test_pndm.py on the emulator, tests/test_pndm_gpu.py on the MI355X) -------------------------------------------------
SHAPES = SS.SHAPES
UPDATE = (1.1521, -1.2198, 1.3085, -0.8206, 0.1996, 1 / 3)               # c_x, c_0 .. c_3, s_g: a fourth-order PLMS step of a 5-step schedule, a middle Runge-Kutta weight
ORDERS = (1, 2, 3, 4)
ACC_MODES = ("none", "write", "read_write", "in_place")                  # no accumulator; acc_out alone; acc_in and another acc_out; acc_in == acc_out
Variant = namedtuple("Variant", ["order", "sample_in", "acc", "single", "phi"])
VARIANTS = [Variant(o, s, a, sg, phi) for o in ORDERS for s in (False, True) for a in ACC_MODES for sg in (False, True) for phi in (0.0, 0.7)]
GUIDANCE, VIDEO_SCALE = SS.GUIDANCE, SS.VIDEO_SCALE
OUTPUTS = ("lat", "hist", "sample", "acc")
_extra = {}


def coef_row():
    return torch.tensor(UPDATE, dtype=torch.float64).float()


def operands(shape, dt):
    """sampling_spec's seeded operands of a shape plus three histories, a saved sample and an accumulator (never written: every user clones what a launch writes)"""
    o = dict(SS.operands(shape, dt))
    if shape not in _extra:
        B, F, HW, CL, ld = shape
        g = torch.Generator().manual_seed(57 + 1000 * B + 10 * F + HW + ld)
        _extra[shape] = tuple(torch.randn(B, CL, F, HW, generator=g) for _ in range(5))
    o["hist_1"], o["hist_2"], o["hist_3"], o["sample"], o["acc"] = _extra[shape]
    return o


def step_kwargs(shape, var):
    """keyword arguments of cfg_pndm_step for a variant (without the tensors)"""
    B, F, HW, CL, ld = shape
    return dict(B=B, F=F, HW=HW, c_latent=CL, ld=ld, cfg=True, guidance=GUIDANCE, order=var.order, video_scale=VIDEO_SCALE if var.single else 0.0,
                guidance_rescale=var.phi)


def reference(shape, dt, var):
    """-> {output: (value, bound)}, each [B c_latent][F HW] f64; `acc` is absent for a variant without an accumulator"""
    B, F, HW, CL, ld = shape
    o = operands(shape, dt)
    out = kernel_step(o["pred"], o["latents"], coef_row(), sample_in=o["sample"] if var.sample_in else None, hist_1=o["hist_1"], hist_2=o["hist_2"],
                      hist_3=o["hist_3"], acc_in=o["acc"] if var.acc in ("read_write", "in_place") else None,
                      pred_single=o["single"] if var.single else None, key=(shape, dt, var.single, var.phi), **step_kwargs(shape, var))
    if var.acc == "none":
        del out["acc"]
    return {k: tuple(t.reshape(B * CL, F * HW) for t in pair) for k, pair in out.items()}


def run_step(ops, shape, dt, var, *, on=lambda t: t, hist=None, latents=None, store=True, save=None, pred=None):
    """one launch of cfg_pndm_step on clones of the shared operands -> {lat, hist, sample, acc}, each [B c_latent][F HW].  The output buffers start full of NaN; store=False:
    hist_out and sample_out are not handed over and come back as they were, like the accumulator of a variant without one (save: the same for sample_out alone).  hist: what to hand over as (hist_1, hist_2,
    hist_3) instead of the operands' - the histories an order does not read are always handed over: the kernel must not touch them; latents: what to hand over as the latents"""
    B, F, HW, CL, ld = shape
    o = operands(shape, dt)
    nan = lambda: on(torch.full((B, CL, F, HW), float("nan")))      # noqa: E731
    lat, hout, sout, aout = on((o["latents"] if latents is None else latents).clone()), nan(), nan(), nan()
    h = (o["hist_1"], o["hist_2"], o["hist_3"]) if hist is None else hist
    acc_in = None
    if var.acc == "read_write":
        acc_in = on(o["acc"])
    elif var.acc == "in_place":
        acc_in = aout = on(o["acc"].clone())
    ops.cfg_pndm_step(on(o["pred"] if pred is None else pred), lat, on(coef_row()), sample_in=on(o["sample"]) if var.sample_in else None,
                      sample_out=sout if (store if save is None else save) else None, hist_out=hout if store else None, hist_1=on(h[0]), hist_2=on(h[1]), hist_3=on(h[2]),
                      acc_in=acc_in, acc_out=None if var.acc == "none" else aout, pred_single=on(o["single"]) if var.single else None, **step_kwargs(shape, var))
    return {k: t.reshape(B * CL, F * HW) for k, t in (("lat", lat), ("hist", hout), ("sample", sout), ("acc", aout))}


# ---- driving an ops object through a schedule by the engine's plan (the buffers PNDMSampler keeps) --------------------------------------------------------------
class Buffers:
    def __init__(self, like, on=lambda t: t):
        nan = lambda: on(torch.full(like.shape, float("nan")))      # noqa: E731
        self.hist, self.sample, self.acc = [nan() for _ in range(4)], nan(), nan()

    def kwargs(self, ev):
        """the buffer arguments of cfg_pndm_step for a plan entry (engine/scheduler.py::PNDMEval)"""
        slot = lambda s: self.acc if s == "acc" else self.hist[s]      # noqa: E731
        hs = [slot(s) for s in ev.hist] + [None] * (4 - ev.order)
        return dict(order=ev.order, sample_in=self.sample if ev.sample_in else None, sample_out=self.sample if ev.sample_out else None,
                    hist_out=None if ev.hist_out is None else self.hist[ev.hist_out], hist_1=hs[0], hist_2=hs[1], hist_3=hs[2],
                    acc_in=self.acc if ev.acc_in else None, acc_out=self.acc if ev.acc_out else None)
