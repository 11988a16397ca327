"""`diffusers.DPMSolverMultistepScheduler` surface (reference diffusers/schedulers/scheduling_dpmsolver_multistep.py:36-534) on the
engine's host-side tables.  AnimationPipeline does NOT call `step()` in its loop - guidance, the conversion of the model output and
the multistep update are one fused kernel there (fyc_cfg_solver_step) - but the method is kept for scripts that drive a scheduler by hand:
stateful as the reference's (model_outputs, lower_order_nums, both reset by set_timesteps), on the same collapsed coefficients."""
from __future__ import annotations

import inspect
import json
import os
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Union

import numpy as np
import torch

from followyourclick_amd.engine import SolverConfig
from followyourclick_amd.engine.scheduler import SolverTables


@dataclass
class SchedulerOutput:
    prev_sample: torch.Tensor


class DPMSolverMultistepScheduler:
    order = 1

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02, beta_schedule: str = "linear",
                 trained_betas=None, solver_order: int = 2, prediction_type: str = "epsilon", thresholding: bool = False,
                 dynamic_thresholding_ratio: float = 0.995, sample_max_value: float = 1.0, algorithm_type: str = "dpmsolver++",
                 solver_type: str = "midpoint", lower_order_final: bool = True, rescale_betas_zero_snr: bool = False, **kwargs):
        if thresholding:
            raise NotImplementedError("DPMSolverMultistepScheduler on the MI355X engine: thresholding=True (a per-sample quantile of x0, which the "
                                      "reference calls unsuitable for latent-space diffusion models) is not implemented")
        self.engine_config = SolverConfig(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                          beta_schedule=beta_schedule, trained_betas=trained_betas, solver_order=solver_order,
                                          prediction_type=prediction_type, thresholding=thresholding, algorithm_type=algorithm_type,
                                          solver_type=solver_type, lower_order_final=lower_order_final,
                                          rescale_betas_zero_snr=rescale_betas_zero_snr)
        self.config = SimpleNamespace(**vars(self.engine_config), dynamic_thresholding_ratio=dynamic_thresholding_ratio,
                                      sample_max_value=sample_max_value)
        self.tables = SolverTables(self.engine_config)
        self.betas, self.alphas, self.alphas_cumprod = self.tables.betas, self.tables.alphas, self.tables.alphas_cumprod
        self.alpha_t, self.sigma_t, self.lambda_t = self.tables.alpha_t, self.tables.sigma_t, self.tables.lambda_t
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.linspace(0, num_train_timesteps - 1, num_train_timesteps, dtype=np.float32)[::-1].copy())
        self.model_outputs = [None] * solver_order
        self.lower_order_nums = 0

    @classmethod
    def from_config(cls, config: dict, **kwargs):
        """Keeps the keys this scheduler's constructor knows and drops the rest (reference configuration_utils.py:189-226)."""
        known = set(inspect.signature(cls.__init__).parameters) - {"self", "kwargs"}
        cfg = {k: v for k, v in dict(config).items() if k in known}
        cfg.update({k: v for k, v in kwargs.items() if k in known})
        return cls(**cfg)

    @classmethod
    def from_pretrained(cls, pretrained_model_path, subfolder=None, **kwargs):
        """`from_pretrained(path, subfolder="scheduler")`: local directory only."""
        if subfolder is not None:
            pretrained_model_path = os.path.join(pretrained_model_path, subfolder)
        config_file = os.path.join(pretrained_model_path, "scheduler_config.json")
        if not os.path.isfile(config_file):
            raise EnvironmentError(f"Error no file named scheduler_config.json found in directory {pretrained_model_path}.")
        with open(config_file) as f:
            return cls.from_config(json.load(f), **kwargs)

    def scale_model_input(self, sample: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        return sample

    def set_timesteps(self, num_inference_steps: int, device: Union[str, torch.device, None] = None) -> None:
        self.num_inference_steps = num_inference_steps
        self.timesteps = self.tables.timesteps(num_inference_steps).to(device)
        self._ts = self.timesteps.tolist()
        self.model_outputs = [None] * self.config.solver_order
        self.lower_order_nums = 0

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, return_dict: bool = True):
        """one multistep update (reference :428-494): the step's place by `timesteps == timestep` (the last step when absent, as there), the order
        from lower_order_nums and the lower-order-final rules, then  m0 = a_x x + a_v v,  x' = c_x x + c_0 m0 + c_1 m1 + c_2 m2  in the
        tensors' dtype, summed in the kernel's order"""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        ts, t = self._ts, int(timestep)
        i = ts.index(t) if t in ts else len(ts) - 1
        self.tables.check_step(ts[i])
        order = self.tables.next_order(i, len(ts), self.lower_order_nums)
        ax, av, cx, c0, c1, c2 = torch.tensor(self.tables.step_coefficients(ts, i, order)[:6], dtype=torch.float64).float().tolist()
        m0 = ax * sample + av * model_output
        self.model_outputs = self.model_outputs[1:] + [m0]
        prev = cx * sample + c0 * m0
        if order >= 2:
            prev = prev + c1 * self.model_outputs[-2]
        if order == 3:
            prev = prev + c2 * self.model_outputs[-3]
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1
        if not return_dict:
            return (prev,)
        return SchedulerOutput(prev_sample=prev)

    def add_noise(self, original_samples: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor) -> torch.Tensor:
        abar = self.alphas_cumprod.to(device=original_samples.device, dtype=original_samples.dtype)[timesteps.to(original_samples.device)]
        shape = (-1,) + (1,) * (original_samples.dim() - 1)
        return (abar ** 0.5).reshape(shape) * original_samples + ((1 - abar) ** 0.5).reshape(shape) * noise

    def __len__(self):
        return self.config.num_train_timesteps
