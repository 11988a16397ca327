"""DDIM tables on the host (reference diffusers/schedulers/scheduling_ddim.py, patched with
zero-terminal-SNR rescaling and v-prediction).

The reference indexes a CPU `alphas_cumprod` table with a device tensor inside `step()` (a GPU->CPU sync
every step, scheduling_ddim.py:308-312).  Here everything that depends only on (t, n) is precomputed in
f32 with the same op sequence as the reference (bit-identical table), and each step's four coefficients
{sqrt(abar_t), sqrt(1-abar_t), sqrt(abar_prev), sqrt(1-abar_prev)} are uploaded once per clip; the
update itself is the fused guidance+DDIM kernel (fyc_cfg_ddim_step).
"""
from __future__ import annotations

from collections import namedtuple
from typing import List

import numpy as np
import torch

from .config import DDIMConfig, PNDMConfig, SigmaConfig, SolverConfig

PRED_TYPES = {"epsilon": 0, "v_prediction": 1, "sample": 2}


def rescale_zero_terminal_snr(betas: torch.Tensor) -> torch.Tensor:
    """Algorithm 1 of arXiv:2305.08891 as the reference applies it (scheduling_ddim.py:78-111)."""
    abar_sqrt = torch.cumprod(1.0 - betas, dim=0).sqrt()
    a0, aT = abar_sqrt[0].clone(), abar_sqrt[-1].clone()
    abar_sqrt = abar_sqrt - aT
    abar_sqrt = abar_sqrt * (a0 / (a0 - aT))
    abar = abar_sqrt ** 2
    alphas = torch.cat([abar[0:1], abar[1:] / abar[:-1]])
    return 1 - alphas


def alpha_add_noise_coefficients(alphas_cumprod: torch.Tensor, t) -> tuple:
    """(sqrt(abar_t), sqrt(1 - abar_t)) as the reference's add_noise forms them (scheduling_ddim.py:388-393): f32 tensor arithmetic on the
    table entry -> python floats holding those f32 values"""
    t = int(t)
    if not 0 <= t < len(alphas_cumprod):
        raise ValueError(f"timestep {t} lies outside the {len(alphas_cumprod)} training timesteps")
    a_t = alphas_cumprod[t]
    return float(a_t ** 0.5), float((1 - a_t) ** 0.5)


def betas_from_config(cfg, who: str) -> torch.Tensor:
    """the f32 betas of a scheduler config: trained_betas, or the linear / scaled_linear schedule, then the zero-terminal-SNR rescale if asked
    for.  who: the tables class, named where the schedule is refused"""
    n = cfg.num_train_timesteps
    if cfg.trained_betas is not None:
        betas = torch.tensor(cfg.trained_betas, dtype=torch.float32)
    elif cfg.beta_schedule == "linear":
        betas = torch.linspace(cfg.beta_start, cfg.beta_end, n, dtype=torch.float32)
    elif cfg.beta_schedule == "scaled_linear":
        betas = torch.linspace(cfg.beta_start ** 0.5, cfg.beta_end ** 0.5, n, dtype=torch.float32) ** 2
    else:
        raise NotImplementedError(f"{cfg.beta_schedule} is not implemented for {who}")
    return rescale_zero_terminal_snr(betas) if cfg.rescale_betas_zero_snr else betas


class AlphaAddNoise:
    """add_noise of the schedulers whose latents live in alpha space (DDIM, DPM-Solver, PNDM), from their alphas_cumprod table"""

    def add_noise_coefficients(self, t, num_inference_steps: int = None) -> tuple:
        """(c_x, c_n) of add_noise at timestep t: x_t = c_x x_0 + c_n noise"""
        return alpha_add_noise_coefficients(self.alphas_cumprod, t)


def check_start_index(start_index, entries: int) -> int:
    """the first entry of the scheduler's timestep list a sliced run takes (what `strength` selects): 0 .. entries - 1"""
    k = int(start_index)
    if not 0 <= k < entries:
        raise ValueError(f"start_index = {start_index} leaves no step of a schedule of {entries} entries (0 .. {entries - 1})")
    return k


class DDIMTables(AlphaAddNoise):
    def __init__(self, cfg: DDIMConfig):
        self.cfg = cfg
        betas = betas_from_config(cfg, "DDIMTables")
        self.betas = betas
        self.alphas = 1.0 - betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if cfg.set_alpha_to_one else self.alphas_cumprod[0]
        if cfg.prediction_type not in PRED_TYPES:
            raise ValueError(f"prediction_type given as {cfg.prediction_type} must be one of `epsilon`, `sample`, or `v_prediction`")
        self.pred_type = PRED_TYPES[cfg.prediction_type]

    def timesteps(self, num_inference_steps: int) -> torch.Tensor:
        """set_timesteps (scheduling_ddim.py:238-252): arange(n) * (T // n), reversed, + steps_offset ("leading", the reference's only
        spacing).  "trailing" and "linspace" are those of later diffusers (arXiv:2305.08891 section 3.3), without steps_offset as there."""
        spacing, T, n = self.cfg.timestep_spacing, self.cfg.num_train_timesteps, num_inference_steps
        if spacing == "leading":
            ratio = self.cfg.num_train_timesteps // num_inference_steps
            return (torch.arange(0, num_inference_steps, dtype=torch.int64) * ratio).flip(0) + self.cfg.steps_offset
        if spacing == "trailing":
            ts = np.round(np.arange(T, 0, -T / n)) - 1
        elif spacing == "linspace":
            ts = np.round(np.linspace(0, T - 1, n))[::-1]
        else:
            raise ValueError(f"timestep_spacing given as {spacing!r} must be one of 'leading', 'trailing' or 'linspace'")
        ts = ts.astype(np.int64)
        # the float step of the trailing arange yields n + 1 entries ending in -1 for some n (61, 103, 121, ... with T = 1000): refused,
        # not truncated - a schedule one entry short or long is another schedule
        if len(ts) != n or (ts < 0).any():
            raise ValueError(f"timestep_spacing {spacing!r} gives no valid schedule for num_inference_steps n = {n} with {T} training "
                             f"timesteps ({len(ts)} entries, smallest {int(ts.min()) if len(ts) else None}): choose another n")
        return torch.from_numpy(ts.copy())

    def check_step(self, t: int, use_clipped_model_output: bool = False) -> None:
        """A step at alphas_cumprod[t] = 0 (the first trailing step of a zero-terminal-SNR table) is x0 = sa x - sb v, eps = sa v + sb x
        for v_prediction and x0 = v for sample: no division.  Epsilon prediction divides by sqrt(abar_t) = 0, and use_clipped_model_output
        re-derives the direction as (x - sqrt(abar_t) x0) / sqrt(1 - abar_t), which no longer sees the clipped x0 at abar_t = 0 and divides
        by zero at abar_t = 1: both are refused at such a timestep."""
        a_t = float(self.alphas_cumprod[t])
        if a_t == 0.0 and self.pred_type == PRED_TYPES["epsilon"]:
            raise ValueError(f"timestep {t}: alphas_cumprod is 0 there (zero terminal SNR) and epsilon prediction divides by its square "
                             "root; such a step needs prediction_type 'v_prediction' or 'sample'")
        if use_clipped_model_output and (a_t == 0.0 or 1.0 - a_t == 0.0):
            raise ValueError(f"timestep {t}: use_clipped_model_output cannot re-derive the noise direction where alphas_cumprod is "
                             f"{a_t:g} ((x - sqrt(abar) x0) / sqrt(1 - abar))")

    def step_coefficients(self, t: int, num_inference_steps: int, eta: float = 0.0) -> List[float]:
        """{sqrt(abar_t), sqrt(1 - abar_t), sqrt(abar_prev), sqrt(1 - abar_prev - sigma^2), sigma} with sigma = eta * sqrt(variance_t)
        (scheduling_ddim.py:229-236 `_get_variance`, :336-349): the same f32 tensor arithmetic as the reference, eta = 0 gives sigma = 0"""
        prev_t = t - self.cfg.num_train_timesteps // num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        variance = ((1 - a_prev) / (1 - a_t)) * (1 - a_t / a_prev)
        std = eta * variance ** 0.5
        return [float(a_t ** 0.5), float((1 - a_t) ** 0.5), float(a_prev ** 0.5), float((1 - a_prev - std ** 2) ** 0.5), float(std)]

    def coefficient_table(self, num_inference_steps: int, eta: float = 0.0) -> torch.Tensor:
        ts = self.timesteps(num_inference_steps).tolist()
        return torch.tensor([self.step_coefficients(t, num_inference_steps, eta) for t in ts], dtype=torch.float32)


class SolverTables(AlphaAddNoise):
    """DPM-Solver multistep on the host (reference diffusers/schedulers/scheduling_dpmsolver_multistep.py; arXiv:2206.00927, arXiv:2211.01095).

    alpha_t, sigma_t and lambda_t are the reference's f32 op sequence (:165-170), bit-identical tables.  Every update of the family is linear in
    the current latents x, the (guided) prediction v and the stored converted outputs m1, m2, so a step collapses to six numbers:

        m0 = a_x x + a_v v                          (convert_model_output, :234-280)
        x' = c_x x + c_0 m0 + c_1 m1 + c_2 m2       (:304-426 with D1, D2 expanded)

    The scalars the reference forms (h, r0, r1, exp(-+h) - 1, the heun and third-order factors) are formed in f32 tensor arithmetic in its order
    - its (exp(-h) - 1) / h + 1 cancels in f32, and a step computed from f64 scalars would sit two hundred ulps from it -, then collapsed in f64
    and rounded once each to f32; the update itself is the fused guidance + solver kernel (fyc_cfg_solver_step)."""

    def __init__(self, cfg: SolverConfig):
        self.cfg = cfg
        if cfg.thresholding:
            raise NotImplementedError("thresholding=True (dynamic thresholding, a per-sample quantile of x0) is not implemented for SolverTables")
        betas = betas_from_config(cfg, "SolverTables")
        if cfg.algorithm_type not in ("dpmsolver", "dpmsolver++"):
            raise NotImplementedError(f"{cfg.algorithm_type} is not implemented for SolverTables")
        if cfg.solver_type not in ("midpoint", "heun"):
            raise NotImplementedError(f"{cfg.solver_type} is not implemented for SolverTables")
        if cfg.solver_order not in (1, 2, 3):
            raise ValueError(f"solver_order given as {cfg.solver_order} must be 1, 2 or 3")
        if cfg.prediction_type not in PRED_TYPES:
            raise ValueError(f"prediction_type given as {cfg.prediction_type} must be one of `epsilon`, `sample`, or `v_prediction`")
        self.betas = betas
        self.alphas = 1.0 - betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.alpha_t = torch.sqrt(self.alphas_cumprod)
        self.sigma_t = torch.sqrt(1 - self.alphas_cumprod)
        self.lambda_t = torch.log(self.alpha_t) - torch.log(self.sigma_t)
        self.pred_type = PRED_TYPES[cfg.prediction_type]
        self.plus = cfg.algorithm_type == "dpmsolver++"

    def timesteps(self, num_inference_steps: int) -> torch.Tensor:
        """set_timesteps (:199-204): linspace(0, T - 1, n + 1).round()[::-1][:-1].  An n that rounds two entries to the same timestep is refused:
        the reference's step() finds its place by `timesteps == t`, and a zero-length step has h = 0"""
        T, n = self.cfg.num_train_timesteps, int(num_inference_steps)
        if n < 1:
            raise ValueError(f"num_inference_steps = {num_inference_steps} must be at least 1")
        ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        if len(np.unique(ts)) != n:
            raise ValueError(f"num_inference_steps n = {n} gives duplicate timesteps with {T} training timesteps: choose n < {T}")
        return torch.from_numpy(ts)

    def next_order(self, step_index: int, num_steps: int, lower_order_nums: int) -> int:
        """the order step() takes at a step (:463-489) after `lower_order_nums` earlier steps (counted up to solver_order)"""
        short = self.cfg.lower_order_final and num_steps < 15
        if self.cfg.solver_order == 1 or lower_order_nums < 1 or (short and step_index == num_steps - 1):
            return 1
        if self.cfg.solver_order == 2 or lower_order_nums < 2 or (short and step_index == num_steps - 2):
            return 2
        return 3

    def plan(self, num_inference_steps: int, start_index: int = 0) -> List[int]:
        """per step, the order actually used: the warm-up from first order and the lower-order final steps of a schedule shorter than 15.
        start_index > 0: the steps start_index .. n - 1 of a sliced run - the warm-up starts over (the scheduler's history is empty), the
        lower-order final steps are found by the place in the full list, as the reference's step() finds them"""
        orders, low = [], 0
        for i in range(check_start_index(start_index, num_inference_steps), num_inference_steps):
            orders.append(self.next_order(i, num_inference_steps, low))
            low = min(low + 1, self.cfg.solver_order)
        return orders

    def check_step(self, t: int) -> None:
        """At alphas_cumprod[t] = 0 (the first step of a zero-terminal-SNR table) lambda_t is -inf.  dpmsolver++ with v_prediction or sample stays
        finite there, as in the reference: the first step degenerates to sigma_prev x + alpha_prev x0 and the next step's 1 / r0 is 0.  Epsilon
        prediction divides by alpha_t = 0 and dpmsolver multiplies by exp(h) = inf: both are refused at such a timestep."""
        if float(self.alphas_cumprod[t]) != 0.0:
            return
        if not self.plus:
            raise ValueError(f"timestep {t}: alphas_cumprod is 0 there (zero terminal SNR, lambda = -inf) and algorithm_type 'dpmsolver' "
                             "integrates exp(h) = inf over it; such a step needs algorithm_type 'dpmsolver++'")
        if self.pred_type == PRED_TYPES["epsilon"]:
            raise ValueError(f"timestep {t}: alphas_cumprod is 0 there (zero terminal SNR) and epsilon prediction divides by its square "
                             "root; such a step needs prediction_type 'v_prediction' or 'sample'")

    def convert_coefficients(self, t: int) -> List[float]:
        """(a_x, a_v) of m0 = a_x x + a_v v (:234-280): x0 for dpmsolver++, eps for dpmsolver, from the f32 table entries, in f64"""
        a, s = float(self.alpha_t[t]), float(self.sigma_t[t])
        pred = self.cfg.prediction_type
        if self.plus:
            if pred == "epsilon":           # x0 = (x - sigma_t v) / alpha_t; alpha_t = 0 is refused by check_step
                return [1.0 / a, -s / a] if a != 0.0 else [float("nan"), float("nan")]
            return [a, -s] if pred == "v_prediction" else [0.0, 1.0]            # x0 = alpha_t x - sigma_t v;  x0 = v
        if pred == "sample":                # eps = (x - alpha_t v) / sigma_t
            return [1.0 / s, -a / s] if s != 0.0 else [float("nan"), float("nan")]
        return [s, a] if pred == "v_prediction" else [0.0, 1.0]                 # eps = alpha_t v + sigma_t x;  eps = v

    def step_scalars(self, ts: List[int], i: int, order: int) -> dict:
        """the scalars of step i of the schedule `ts` at an order, each formed as the reference forms it (f32 tensor arithmetic, its order of
        operations) -> python floats holding those f32 values: cx (the factor of the sample), k0, k1, k2 (the signed factors of D0, D1, D2),
        inv_r0 = 1 / r0, inv_r1 = 1 / r1, w = r0 / (r0 + r1), u = 1 / (r0 + r1).  Only what the order uses is formed: at an infinite h (the first
        step from lambda = -inf) the higher-order factors are inf / inf."""
        lam, al, sg = self.lambda_t, self.alpha_t, self.sigma_t
        t, s0 = (0 if i == len(ts) - 1 else ts[i + 1]), ts[i]
        h = lam[t] - lam[s0]
        if self.plus:
            cx, lead, e, hh = sg[t] / sg[s0], al[t], torch.exp(-h) - 1.0, h
        else:
            cx, lead, e, hh = al[t] / al[s0], sg[t], torch.exp(h) - 1.0, -h
        out = dict(cx=cx, k0=-(lead * e))
        if order == 2 and self.cfg.solver_type == "midpoint":
            out["k1"] = -(0.5 * (lead * e))
        elif order >= 2:
            # dpmsolver++: + alpha_t ((exp(-h) - 1) / h + 1);  dpmsolver: - sigma_t ((exp(h) - 1) / h - 1)
            out["k1"] = lead * (e / h + 1.0) if self.plus else -(lead * (e / h - 1.0))
        if order == 3:
            # dpmsolver++: (exp(-h) - 1 + h) / h^2 - 0.5;  dpmsolver: (exp(h) - 1 - h) / h^2 - 0.5
            out["k2"] = -(lead * ((e + hh) / h ** 2 - 0.5))
        if order >= 2:
            r0 = (lam[s0] - lam[ts[i - 1]]) / h
            out["inv_r0"] = 1.0 / r0
        if order == 3:
            r1 = (lam[ts[i - 1]] - lam[ts[i - 2]]) / h
            out["inv_r1"], out["w"], out["u"] = 1.0 / r1, r0 / (r0 + r1), 1.0 / (r0 + r1)
        return {k: float(v) for k, v in out.items()}

    def step_coefficients(self, ts: List[int], i: int, order: int) -> List[float]:
        """{a_x, a_v, c_x, c_0, c_1, c_2, 0, 0} of step i: the f32 scalars collapsed in f64.  An infinite h_0 or h_1 (a history entry taken at
        lambda = -inf) enters only through 1 / r0, 1 / r1, w and u, which the f32 arithmetic has already turned into 0: the products below are of
        finite numbers, never inf * 0."""
        s = self.step_scalars(ts, i, order)
        c0, c1, c2 = s["k0"], 0.0, 0.0
        if order == 2:          # D1 = (1 / r0) (m0 - m1)
            d = s["k1"] * s["inv_r0"]
            c0, c1 = c0 + d, -d
        elif order == 3:        # D1_0 = (m0 - m1) / r0, D1_1 = (m1 - m2) / r1, D1 = D1_0 + w (D1_0 - D1_1), D2 = u (D1_0 - D1_1)
            g0 = (s["k1"] * (1.0 + s["w"]) + s["k2"] * s["u"]) * s["inv_r0"]        # the factor of m0 - m1
            g1 = -(s["k1"] * s["w"] + s["k2"] * s["u"]) * s["inv_r1"]               # the factor of m1 - m2
            c0, c1, c2 = c0 + g0, g1 - g0, -g1
        return [*self.convert_coefficients(ts[i]), s["cx"], c0, c1, c2, 0.0, 0.0]

    def coefficient_table(self, num_inference_steps: int, start_index: int = 0) -> torch.Tensor:
        """[n - start_index][8] f32, each entry rounded once, for the orders of plan(n, start_index)"""
        ts = self.timesteps(num_inference_steps).tolist()
        for t in ts[start_index:]:
            self.check_step(t)
        return torch.tensor([self.step_coefficients(ts, start_index + j, o) for j, o in enumerate(self.plan(num_inference_steps, start_index))],
                            dtype=torch.float64).float()


SIGMA_KINDS = ("euler", "euler_ancestral", "lms")


class SigmaTables:
    """The sigma-space (k-diffusion) samplers on the host: Euler, Euler ancestral and LMS (reference diffusers/schedulers/
    scheduling_euler_discrete.py, scheduling_euler_ancestral_discrete.py, scheduling_lms_discrete.py).

    sigma = sqrt((1 - abar) / abar) is the reference's f32 op sequence, interpolated in f64 at the fractional timesteps
    linspace(0, T - 1, n)[::-1] and cast to f32 (bit-identical tables).  The latents live in sigma space (x = x0 + sigma noise, started at
    init_noise_sigma), the UNet sees x / sqrt(sigma^2 + 1), and every update of the three is linear in the latents x, the (guided) prediction
    v, up to three stored derivatives and a noise tensor, so a step collapses to eight numbers:

        d  = a_x x + a_v v                                                  (the derivative (x - x0) / sigma)
        x' = c_x x + c_0 d + c_1 d_1 + c_2 d_2 + c_3 d_3 + c_n noise

    The scalars the reference forms (dt, sigma_up, sigma_down) are formed in f32 tensor arithmetic in its order, the rest in f64 from the f32
    sigmas, each coefficient rounded once to f32; the update itself is the fused guidance + step kernel (fyc_cfg_sigma_step).  The LMS
    coefficients are the integrals of the Lagrange basis polynomials in closed form (the reference integrates them numerically)."""

    def __init__(self, cfg: SigmaConfig):
        self.cfg = cfg
        if cfg.kind not in SIGMA_KINDS:
            raise ValueError(f"kind given as {cfg.kind!r} must be one of {SIGMA_KINDS}")
        betas = betas_from_config(cfg, "SigmaTables")
        if cfg.prediction_type not in ("epsilon", "v_prediction"):
            raise ValueError(f"prediction_type given as {cfg.prediction_type} must be one of `epsilon`, or `v_prediction`")
        self.betas = betas
        self.alphas = 1.0 - betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        if cfg.rescale_betas_zero_snr:
            self.alphas_cumprod[-1] = 2.0 ** -24          # sigma_max = sqrt(2^24 - 1) ~ 4096 instead of infinity
        self.pred_type = PRED_TYPES[cfg.prediction_type]
        self.train_sigmas = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()            # f32 [T], ascending
        # (the reference's constructor: the reversed table with 0 appended, cast to f32, its maximum)
        self.init_noise_sigma = float(np.concatenate([self.train_sigmas[::-1], [0.0]]).astype(np.float32).max())

    def timesteps(self, num_inference_steps: int) -> torch.Tensor:
        """set_timesteps: linspace(0, T - 1, n)[::-1] in float64 - fractional (957.375 at n = 25); the UNet's embedding gets them as they are"""
        n = int(num_inference_steps)
        if n < 1:
            raise ValueError(f"num_inference_steps = {num_inference_steps} must be at least 1")
        return torch.from_numpy(np.linspace(0, self.cfg.num_train_timesteps - 1, n, dtype=float)[::-1].copy())

    def sigmas(self, num_inference_steps: int) -> torch.Tensor:
        """[n + 1] f32: the training sigmas interpolated at the timesteps, then 0.  A schedule that touches a timestep where alphas_cumprod is 0
        (sigma = inf; the reference goes on to inf / NaN latents) is refused."""
        ts = self.timesteps(num_inference_steps).numpy()
        sig = np.interp(ts, np.arange(0, len(self.train_sigmas)), self.train_sigmas)
        if not np.isfinite(sig).all():
            t = ts[~np.isfinite(sig)][0]
            raise ValueError(f"timestep {t:g}: alphas_cumprod is 0 there (zero terminal SNR), so sigma is infinite; a sigma-space scheduler "
                             "needs rescale_betas_zero_snr=True, which rescales the betas itself and ends the table at alphas_cumprod = 2^-24")
        return torch.from_numpy(np.concatenate([sig, [0.0]]).astype(np.float32))

    def input_denominators(self, num_inference_steps: int) -> List[float]:
        """per step, the f32 value (sigma^2 + 1) ^ 0.5 that scale_model_input divides the UNet's input by, formed as the reference forms it"""
        return [float((s ** 2 + 1) ** 0.5) for s in self.sigmas(num_inference_steps)[:-1]]

    def order(self, i: int, max_order: int = 4) -> int:
        """how many derivatives step i uses: 1 for the Euler samplers, min(i + 1, order) for LMS (scheduling_lms_discrete.py:239)"""
        return min(i + 1, max_order) if self.cfg.kind == "lms" else 1

    @staticmethod
    def lms_coefficients(sigmas: torch.Tensor, i: int, order: int) -> List[float]:
        """c_k = integral from sigmas[i] to sigmas[i + 1] of l_k, the Lagrange basis polynomial on sigmas[i], .., sigmas[i - order + 1]
        (get_lms_coefficient, :136-156), in closed form in f64 from the f32 sigmas.  In u = tau - sigmas[i] the antiderivative vanishes at the
        lower limit, so nothing cancels between the two ends."""
        from numpy.polynomial import polynomial as Poly
        s = [float(v) for v in sigmas]
        h = s[i + 1] - s[i]
        out = []
        for k in range(order):
            p = np.array([1.0])
            for j in range(order):
                if j != k:
                    p = Poly.polymul(p, np.array([-(s[i - j] - s[i]), 1.0]) / (s[i - k] - s[i - j]))
            out.append(float(Poly.polyval(h, Poly.polyint(p))))
        return out

    def step_coefficients(self, sigmas: torch.Tensor, i: int, order: int = None, stored: int = None) -> List[float]:
        """{a_x, a_v, c_x, c_0, c_1, c_2, c_3, c_n} of step i of the schedule `sigmas` ([n + 1] f32), in f64.  order: how many derivatives an LMS
        step uses (None = self.order(i)).  stored (None = order): how many derivatives the scheduler holds at that step - fewer than `order` in
        a run that starts at a later entry of the list: the reference takes its order from the step's place in the list, integrates the
        Lagrange basis of that order and zips the coefficients with the derivatives it has, which drops the last ones (scheduling_lms_discrete.py
        :239-248)"""
        kind = self.cfg.kind
        order = self.order(i) if order is None else order
        stored = order if stored is None else min(int(stored), order)
        sg, sg_to = sigmas[i], sigmas[i + 1]                # 0-dim f32 tensors: the reference's operands
        s = float(sg)
        if self.cfg.prediction_type == "epsilon":           # x0 = x - s v: d = v
            ax, av = 0.0, 1.0
        else:                                               # x0 = -s / sqrt(s^2 + 1) v + x / (s^2 + 1): d = s / (s^2 + 1) x + v / sqrt(s^2 + 1)
            ax, av = s / (s * s + 1.0), 1.0 / (s * s + 1.0) ** 0.5
        c = [0.0, 0.0, 0.0, 0.0]
        cn = 0.0
        if kind == "euler":
            c[0] = float(sg_to - sg)                                                        # dt (:251, gamma = 0)
        elif kind == "euler_ancestral":
            sigma_up = (sg_to ** 2 * (sg ** 2 - sg_to ** 2) / sg ** 2) ** 0.5               # (:220-228)
            sigma_down = (sg_to ** 2 - sigma_up ** 2) ** 0.5
            c[0], cn = float(sigma_down - sg), float(sigma_up)
        else:
            c[:stored] = self.lms_coefficients(sigmas, i, order)[:stored]
        return [ax, av, 1.0, *c, cn]

    def plan(self, num_inference_steps: int, start_index: int = 0) -> List[int]:
        """per step of a run over the entries start_index .. n - 1, how many derivatives the update reads: 1 for the Euler samplers; for LMS
        the order of the step's place in the list, cut to the derivatives stored since the run began"""
        k = check_start_index(start_index, num_inference_steps)
        return [min(self.order(i), i - k + 1) for i in range(k, num_inference_steps)]

    def coefficient_table(self, num_inference_steps: int, start_index: int = 0) -> torch.Tensor:
        """[n - start_index][8] f32, each entry rounded once"""
        sig = self.sigmas(num_inference_steps)
        k = check_start_index(start_index, num_inference_steps)
        tab = torch.tensor([self.step_coefficients(sig, i, stored=i - k + 1) for i in range(k, num_inference_steps)], dtype=torch.float64).float()
        if not torch.isfinite(tab).all():
            raise ValueError(f"the {self.cfg.kind} schedule of {num_inference_steps} steps has a non-finite coefficient (sigmas {sig.tolist()})")
        return tab

    def add_noise_coefficients(self, t, num_inference_steps: int = None) -> tuple:
        """(1, sigma_t) of add_noise at an entry t of the schedule of n steps: x_t = x_0 + sigma_t noise, sigma looked up by `timesteps == t`
        as the reference's add_noise does (scheduling_euler_discrete.py:276-279)"""
        if num_inference_steps is None:
            raise ValueError("a sigma-space add_noise looks the timestep up in a schedule: num_inference_steps is needed")
        hit = (self.timesteps(num_inference_steps) == float(t)).nonzero()
        if hit.numel() != 1:
            raise ValueError(f"timestep {t} is not an entry of the schedule of {num_inference_steps} steps")
        return 1.0, float(self.sigmas(num_inference_steps)[int(hit)])


# one evaluation of a PNDM schedule: what _get_prev_sample sees (timestep, prev_timestep), the weights of the combined model output on
# (g, h_1, h_2, h_3), which buffers the launch reads and writes.  hist: the slot of h_1 .. h_{order-1} - 0..3 a history buffer, "acc" the
# Runge-Kutta accumulator; hist_out: the slot that receives g (None: not stored); s_g: the weight of g in the accumulator (0: none)
PNDMEval = namedtuple("PNDMEval", ["counter", "timestep", "prev_timestep", "order", "weights", "hist", "hist_out", "sample_in", "sample_out",
                                   "acc_in", "acc_out", "s_g"])
PLMS_WEIGHTS = {1: (1.0,), 2: (3 / 2, -1 / 2), 3: (23 / 12, -16 / 12, 5 / 12), 4: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}      # Adams-Bashforth (:323-335)


class PNDMTables(AlphaAddNoise):
    """PNDM on the host, PLMS mode (skip_prk_steps, what Stable Diffusion 1.x ships) and Runge-Kutta mode (reference diffusers/schedulers/
    scheduling_pndm.py; arXiv:2202.09778).

    The timestep list has n + 1 entries in PLMS mode (the second one repeated) and n + 9 in Runge-Kutta mode (twelve PRK evaluations on
    half steps, then PLMS).  Some evaluations update not the latents they were handed but a sample saved earlier (PLMS: counter == 1; PRK:
    the three later evaluations of each group of four), PRK sums e/6 + e/3 + e/3 + e/6 over a group, and the v-prediction conversion is
    applied to the COMBINED model output with the current sample and timestep (:376-377) - so the history holds raw (guided) predictions.
    All of it is linear, and an evaluation collapses to six numbers:

        x' = c_x x_src + c_0 g + c_1 h_1 + c_2 h_2 + c_3 h_3,      acc' = acc + s_g g

    with g the guided prediction, h_k the stored predictions (or the PRK accumulator) and x_src the latents or the saved sample.  Formula (9)
    (_get_prev_sample, :358-399) gives x' = sc x - k m with sc = sqrt(a_prev / a_t), k = (a_prev - a_t) / (a_t sqrt(1 - a_prev) +
    sqrt(a_t (1 - a_t) a_prev)); m = sum w_i h_i for epsilon prediction, sqrt(a_t) sum w_i h_i + sqrt(1 - a_t) x for v_prediction.  The
    coefficients are collapsed in f64 from the f32 alphas_cumprod entries the reference indexes and rounded once each to f32; the update
    itself is the fused guidance + step kernel (fyc_cfg_pndm_step)."""

    PRK_EVALUATIONS = 12          # three groups of four on the schedule's first three steps (pndm_order = 4; :178-185)

    def __init__(self, cfg: PNDMConfig):
        self.cfg = cfg
        betas = betas_from_config(cfg, "PNDMTables")
        if cfg.prediction_type not in ("epsilon", "v_prediction"):
            raise ValueError(f"prediction_type given as {cfg.prediction_type} must be one of `epsilon` or `v_prediction`")
        self.betas = betas
        self.alphas = 1.0 - betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if cfg.set_alpha_to_one else self.alphas_cumprod[0]
        self.pred_type = PRED_TYPES[cfg.prediction_type]

    def split_timesteps(self, num_inference_steps: int):
        """set_timesteps (:153-187) -> (prk_timesteps, plms_timesteps), numpy arrays as the reference keeps them.  steps_offset and
        skip_prk_steps are read from the config at every call: the pipelines patch steps_offset after construction, as the reference's do."""
        n, T = int(num_inference_steps), self.cfg.num_train_timesteps
        if not 1 <= n <= T:
            raise ValueError(f"num_inference_steps = {num_inference_steps} must lie in 1 .. {T}")
        base = (np.arange(0, n) * (T // n)).round()
        base += self.cfg.steps_offset
        if self.cfg.skip_prk_steps:
            return np.array([]), np.concatenate([base[:-1], base[-2:-1], base[-1:]])[::-1].copy()
        if n < 4:       # the reference dies in a numpy broadcast (the last four timesteps against a tile of eight)
            raise ValueError(f"num_inference_steps = {n}: the Runge-Kutta mode (skip_prk_steps=False) needs at least 4 inference steps")
        prk = np.array(base[-4:]).repeat(2) + np.tile(np.array([0, T // n // 2]), 4)
        return (prk[:-1].repeat(2)[1:-1])[::-1].copy(), base[:-3][::-1].copy()

    def timesteps(self, num_inference_steps: int) -> torch.Tensor:
        """[n + 1] (PLMS) or [n + 9] (Runge-Kutta) int64: one entry per UNet evaluation"""
        return torch.from_numpy(np.concatenate(self.split_timesteps(num_inference_steps)).astype(np.int64))

    def plan(self, num_inference_steps: int, start_index: int = 0) -> List[PNDMEval]:
        """the reference's state machine (step / step_prk / step_plms: counter, ets, cur_sample, cur_model_output) run over the timestep
        list, with buffer slots in place of tensors.  Four history slots are enough: step_plms keeps ets[-3:] before it appends.
        start_index > 0 (PLMS mode only): the machine runs over the entries start_index .. with its counter at zero, as the reference's
        does when a pipeline slices the list - its second evaluation redoes its first step whatever timestep that entry carries."""
        ts = self.timesteps(num_inference_steps).tolist()
        start_index = check_start_index(start_index, len(ts))
        if start_index > 0 and not self.cfg.skip_prk_steps:
            raise ValueError(f"start_index = {start_index}: a PNDM schedule in Runge-Kutta mode (skip_prk_steps=False) cannot start part-way - "
                             "the slice cuts into a group of four evaluations that share one step; use skip_prk_steps=True (PLMS)")
        ts = ts[start_index:]
        ratio = self.cfg.num_train_timesteps // int(num_inference_steps)
        n_prk = 0 if self.cfg.skip_prk_steps else self.PRK_EVALUATIONS
        ets, plan = [], []

        def store():
            ets.append(next(s for s in range(4) if s not in ets))
            return ets[-1]
        for counter, t in enumerate(ts):
            if counter < n_prk:         # step_prk (:251-270): every evaluation of a group steps from the sample saved at its first one
                prev_t, t_group, r = t - (0 if counter % 2 else ratio // 2), ts[counter // 4 * 4], counter % 4
                if r == 0:
                    ev = PNDMEval(counter, t_group, prev_t, 1, (1.0,), (), store(), False, True, False, True, 1 / 6)
                elif r < 3:
                    ev = PNDMEval(counter, t_group, prev_t, 1, (1.0,), (), None, True, False, True, True, 1 / 3)
                else:                   # e' = acc + e / 6: the accumulator is the second term
                    ev = PNDMEval(counter, t_group, prev_t, 2, (1 / 6, 1.0), ("acc",), None, True, False, False, False, 0.0)
            elif counter == 1:          # step_plms (:316-329): the second evaluation redoes step 0 from the saved sample with (e + e_0) / 2
                ev = PNDMEval(counter, t + ratio, t, 2, (0.5, 0.5), (ets[-1],), None, True, False, False, False, 0.0)
            else:
                del ets[:-3]
                slot = store()
                order = len(ets)
                ev = PNDMEval(counter, t, t - ratio, order, PLMS_WEIGHTS[order], tuple(ets[-2::-1]), slot, False, counter == 0, False, False, 0.0)
            plan.append(ev)
        return plan

    def check_step(self, t: int) -> None:
        """formula (9) divides by alphas_cumprod[t]: a step where it is 0 (timestep T - 1 of a zero-terminal-SNR table; the reference goes on to
        NaN) is refused, as is a timestep outside the table (a steps_offset that pushes the first step past it)"""
        if not 0 <= t < len(self.alphas_cumprod):
            raise ValueError(f"timestep {t} lies outside the {len(self.alphas_cumprod)} training timesteps (steps_offset = {self.cfg.steps_offset})")
        if float(self.alphas_cumprod[t]) == 0.0:
            raise ValueError(f"timestep {t}: alphas_cumprod is 0 there (zero terminal SNR) and PNDM's formula (9) divides by it; choose a "
                             "schedule that does not start there (leading spacing with steps_offset = 1 never does)")

    def step_coefficients(self, ev: PNDMEval) -> List[float]:
        """{c_x, c_0, c_1, c_2, c_3, s_g} of one evaluation, in f64 from the f32 table entries"""
        self.check_step(ev.timestep)
        a_t = float(self.alphas_cumprod[ev.timestep])
        a_p = float(self.alphas_cumprod[ev.prev_timestep] if ev.prev_timestep >= 0 else self.final_alpha_cumprod)
        sc = (a_p / a_t) ** 0.5
        k = (a_p - a_t) / (a_t * (1 - a_p) ** 0.5 + (a_t * (1 - a_t) * a_p) ** 0.5)
        if self.cfg.prediction_type == "v_prediction":          # m = sqrt(a_t) e' + sqrt(1 - a_t) x
            cx, w = sc - k * (1 - a_t) ** 0.5, -k * a_t ** 0.5
        else:
            cx, w = sc, -k
        c = [w * wi for wi in ev.weights] + [0.0] * (4 - ev.order)
        return [cx, *c, ev.s_g]

    def coefficient_table(self, num_inference_steps: int, start_index: int = 0) -> torch.Tensor:
        """[evaluations][6] f32, each entry rounded once"""
        tab = torch.tensor([self.step_coefficients(ev) for ev in self.plan(num_inference_steps, start_index)], dtype=torch.float64).float()
        if not torch.isfinite(tab).all():
            raise ValueError(f"the PNDM schedule of {num_inference_steps} steps has a non-finite coefficient")
        return tab
