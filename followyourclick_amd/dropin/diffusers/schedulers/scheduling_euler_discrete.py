"""`diffusers.EulerDiscreteScheduler` surface (reference diffusers/schedulers/scheduling_euler_discrete.py:48-287) on the engine's
host-side tables, and the base the other two sigma-space schedulers (Euler ancestral, LMS) share.  AnimationPipeline does NOT call
`step()` or `scale_model_input()` in its loop - the scaled UNet input is one kernel there (fyc_unet_input_scaled) and guidance, the
derivative and the update another (fyc_cfg_sigma_step) - but both methods are kept for scripts that drive a scheduler by hand, on the
same collapsed coefficients."""
from __future__ import annotations

import inspect
import json
import os
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional, Union

import numpy as np
import torch

from followyourclick_amd.engine import SigmaConfig
from followyourclick_amd.engine.scheduler import SigmaTables


@dataclass
class SigmaSchedulerOutput:
    prev_sample: torch.Tensor
    pred_original_sample: Optional[torch.Tensor] = None


class SigmaSchedulerBase:
    """what the three share: the constructor, the tables, scale_model_input, set_timesteps, add_noise and the collapsed update"""
    order = 1
    kind = "euler"

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02, beta_schedule: str = "linear",
                 trained_betas=None, prediction_type: str = "epsilon", rescale_betas_zero_snr: bool = False, **kwargs):
        self.engine_config = SigmaConfig(kind=self.kind, num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                         beta_schedule=beta_schedule, trained_betas=trained_betas, prediction_type=prediction_type,
                                         rescale_betas_zero_snr=rescale_betas_zero_snr)
        cfg = dict(vars(self.engine_config))
        cfg.pop("kind")
        self.config = SimpleNamespace(**cfg)
        self.tables = SigmaTables(self.engine_config)
        self.betas, self.alphas, self.alphas_cumprod = self.tables.betas, self.tables.alphas, self.tables.alphas_cumprod
        self.sigmas = torch.from_numpy(np.concatenate([self.tables.train_sigmas[::-1], [0.0]]).astype(np.float32))
        self.init_noise_sigma = self.sigmas.max()            # standard deviation of the initial noise, a 0-dim tensor as in the reference
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.linspace(0, num_train_timesteps - 1, num_train_timesteps, dtype=float)[::-1].copy())
        self.is_scale_input_called = False

    @classmethod
    def from_config(cls, config: dict, **kwargs):
        """Keeps the keys this scheduler's constructor knows and drops the rest (reference configuration_utils.py:189-226)."""
        known = set(inspect.signature(SigmaSchedulerBase.__init__).parameters) - {"self", "kwargs"}
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

    def _index(self, timestep) -> int:
        """the step's place by `timesteps == timestep`, as the reference finds it (an absent or repeated timestep is an error there too)"""
        if isinstance(timestep, torch.Tensor):
            timestep = timestep.to(self.timesteps.device)
        return (self.timesteps == timestep).nonzero().item()

    def scale_model_input(self, sample: torch.Tensor, timestep) -> torch.Tensor:
        sigma = self.sigmas[self._index(timestep)]
        self.is_scale_input_called = True
        return sample / ((sigma ** 2 + 1) ** 0.5)

    def set_timesteps(self, num_inference_steps: int, device: Union[str, torch.device, None] = None) -> None:
        sigmas = self.tables.sigmas(num_inference_steps)          # (refuses a schedule over an infinite sigma)
        self.num_inference_steps = num_inference_steps
        self.sigmas = sigmas.to(device=device)
        self._sigmas_host = sigmas
        self.timesteps = self.tables.timesteps(num_inference_steps).to(device=device)
        self.derivatives = []

    @staticmethod
    def _refuse_integer(timestep, name) -> None:
        if isinstance(timestep, int) or isinstance(timestep, torch.IntTensor) or isinstance(timestep, torch.LongTensor):
            raise ValueError("Passing integer indices (e.g. from `enumerate(timesteps)`) as timesteps to"
                             f" `{name}.step()` is not supported. Make sure to pass one of the `scheduler.timesteps` as a timestep.")

    def _require_schedule(self) -> None:
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")

    def _update(self, i: int, order: int, model_output, sample, history=(), noise=None, return_dict=True):
        """d = a_x x + a_v v,  x' = c_x x + c_0 d + c_1 d_1 + c_2 d_2 + c_3 d_3 + c_n noise  in the tensors' dtype, summed in the kernel's order
        -> (the output, d)"""
        co = torch.tensor(self.tables.step_coefficients(self._sigmas_host, i, order), dtype=torch.float64).float().tolist()
        ax, av, cx, c, cn = co[0], co[1], co[2], co[3:7], co[7]
        d = ax * sample + av * model_output
        prev = cx * sample + c[0] * d
        for k in range(1, order):
            prev = prev + c[k] * history[k - 1]
        if noise is not None:
            prev = prev + cn * noise
        sigma = float(self._sigmas_host[i])
        x0 = sample - sigma * d                 # (x - x0) / sigma = d
        return ((prev,) if not return_dict else SigmaSchedulerOutput(prev_sample=prev, pred_original_sample=x0)), d

    def add_noise(self, original_samples: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor) -> torch.Tensor:
        sigmas = self.sigmas.to(device=original_samples.device, dtype=original_samples.dtype)
        schedule = self.timesteps.to(original_samples.device)
        timesteps = timesteps.to(original_samples.device)
        sigma = sigmas[[(schedule == t).nonzero().item() for t in timesteps]].flatten()
        while len(sigma.shape) < len(original_samples.shape):
            sigma = sigma.unsqueeze(-1)
        return original_samples + noise * sigma

    def __len__(self):
        return self.config.num_train_timesteps


class EulerDiscreteScheduler(SigmaSchedulerBase):
    kind = "euler"

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, s_churn: float = 0.0, s_tmin: float = 0.0,
             s_tmax: float = float("inf"), s_noise: float = 1.0, generator: Optional[torch.Generator] = None, return_dict: bool = True):
        """one Euler step (reference :160-258).  Without churn (the only way the reference's pipeline can call it: its loop forwards eta and
        generator alone) it is the collapsed update of the fused kernel.  With s_churn > 0 inside [s_tmin, s_tmax] the sample is first
        raised to sigma_hat = sigma (gamma + 1) with fresh noise, in torch as the reference writes it.  The noise is drawn from `generator` on every
        call, used or not, as the reference draws it: a generator shared with other code advances as it does there."""
        self._refuse_integer(timestep, "EulerDiscreteScheduler")
        self._require_schedule()
        i = self._index(timestep)
        sigma = self.sigmas[i]
        gamma = min(s_churn / (len(self.sigmas) - 1), 2 ** 0.5 - 1) if s_tmin <= sigma <= s_tmax else 0.0
        noise = torch.randn(model_output.shape, dtype=model_output.dtype, device=model_output.device, generator=generator)
        if gamma <= 0:
            return self._update(i, 1, model_output, sample, return_dict=return_dict)[0]
        sigma_hat = sigma * (gamma + 1)
        sample = sample + (noise * s_noise) * (sigma_hat ** 2 - sigma ** 2) ** 0.5
        if self.config.prediction_type == "epsilon":
            x0 = sample - sigma_hat * model_output
        else:
            x0 = model_output * (-sigma / (sigma ** 2 + 1) ** 0.5) + (sample / (sigma ** 2 + 1))
        prev = sample + ((sample - x0) / sigma_hat) * (self.sigmas[i + 1] - sigma_hat)
        return (prev,) if not return_dict else SigmaSchedulerOutput(prev_sample=prev, pred_original_sample=x0)
