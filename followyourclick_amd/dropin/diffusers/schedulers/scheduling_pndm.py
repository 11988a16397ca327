"""`diffusers.PNDMScheduler` surface (reference diffusers/schedulers/scheduling_pndm.py:57-425) on the engine's host-side tables: the
scheduler Stable Diffusion 1.x checkpoints name in scheduler/scheduler_config.json (skip_prk_steps = true, steps_offset = 1: PLMS), and its
Runge-Kutta mode (skip_prk_steps = false, the class default).  The pipelines do NOT call `step()` in their loops - guidance, the combination
of the stored predictions, formula (9) and the saved sample are one fused kernel there (fyc_cfg_pndm_step) - but the method is kept for
scripts that drive a scheduler by hand: stateful as the reference's (counter, ets, cur_sample, cur_model_output; set_timesteps resets
counter and ets), on the same collapsed coefficients, summed in the kernel's order."""
from __future__ import annotations

import inspect
import json
import os
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Union

import numpy as np
import torch

from followyourclick_amd.engine import PNDMConfig
from followyourclick_amd.engine.scheduler import PLMS_WEIGHTS, PNDMEval, PNDMTables


@dataclass
class SchedulerOutput:
    prev_sample: torch.Tensor


class PNDMScheduler:
    order = 1

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02, beta_schedule: str = "linear",
                 trained_betas=None, skip_prk_steps: bool = False, set_alpha_to_one: bool = False, prediction_type: str = "epsilon",
                 steps_offset: int = 0, rescale_betas_zero_snr: bool = False, **kwargs):
        self.engine_config = PNDMConfig(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                        beta_schedule=beta_schedule, trained_betas=trained_betas, skip_prk_steps=skip_prk_steps,
                                        set_alpha_to_one=set_alpha_to_one, prediction_type=prediction_type, steps_offset=steps_offset,
                                        rescale_betas_zero_snr=rescale_betas_zero_snr)
        self.config = SimpleNamespace(**vars(self.engine_config))
        self.tables = PNDMTables(self.engine_config)
        self.betas, self.alphas, self.alphas_cumprod = self.tables.betas, self.tables.alphas, self.tables.alphas_cumprod
        self.final_alpha_cumprod = self.tables.final_alpha_cumprod
        self.init_noise_sigma = 1.0
        self.pndm_order = 4
        # running values
        self.cur_model_output = 0
        self.counter = 0
        self.cur_sample = None
        self.ets = []
        # setable values
        self.num_inference_steps = None
        self._timesteps = np.arange(0, num_train_timesteps)[::-1].copy()
        self.prk_timesteps = None
        self.plms_timesteps = None
        self.timesteps = None

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
        self.prk_timesteps, self.plms_timesteps = self.tables.split_timesteps(num_inference_steps)
        self.num_inference_steps = num_inference_steps
        self.timesteps = self.tables.timesteps(num_inference_steps).to(device)
        self.ets = []
        self.counter = 0

    def _prev_sample(self, ev: PNDMEval, sample: torch.Tensor, terms) -> torch.Tensor:
        """x' = c_x x + c_0 g + c_1 h_1 + ...  in the tensors' dtype, summed left to right as the kernel sums.  ev carries the pair of timesteps and the weights;
        the tensors are held here, so its buffer fields stay empty"""
        co = torch.tensor(self.tables.step_coefficients(ev), dtype=torch.float64).float().tolist()
        prev = co[0] * sample
        for c, h in zip(co[1:5], terms):
            prev = prev + c * h
        return prev

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, return_dict: bool = True):
        """one evaluation (reference :192-221): step_prk while the Runge-Kutta list lasts, step_plms after it"""
        if self.prk_timesteps is not None and self.counter < len(self.prk_timesteps) and not self.config.skip_prk_steps:
            return self.step_prk(model_output=model_output, timestep=timestep, sample=sample, return_dict=return_dict)
        return self.step_plms(model_output=model_output, timestep=timestep, sample=sample, return_dict=return_dict)

    def _require_schedule(self) -> None:
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")

    def step_prk(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, return_dict: bool = True):
        """one Runge-Kutta evaluation (reference :223-276): four of them approximate one step, all from the sample saved at the first"""
        self._require_schedule()
        half = self.config.num_train_timesteps // self.num_inference_steps // 2
        prev_timestep = int(timestep) - (0 if self.counter % 2 else half)
        group_timestep = int(self.prk_timesteps[self.counter // 4 * 4])
        r = self.counter % 4
        if r == 0:
            self.cur_model_output = self.cur_model_output + (1 / 6) * model_output
            self.ets.append(model_output)
            self.cur_sample = sample
        elif r < 3:
            self.cur_model_output = self.cur_model_output + (1 / 3) * model_output
        cur_sample = self.cur_sample if self.cur_sample is not None else sample
        if r == 3:
            ev = PNDMEval(self.counter, group_timestep, prev_timestep, 2, (1 / 6, 1.0), (), None, False, False, False, False, 0.0)
            prev = self._prev_sample(ev, cur_sample, (model_output, self.cur_model_output))
            self.cur_model_output = 0
        else:
            ev = PNDMEval(self.counter, group_timestep, prev_timestep, 1, (1.0,), (), None, False, False, False, False, 0.0)
            prev = self._prev_sample(ev, cur_sample, (model_output,))
        self.counter += 1
        return (prev,) if not return_dict else SchedulerOutput(prev_sample=prev)

    def step_plms(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, return_dict: bool = True):
        """one linear multistep evaluation (reference :278-343)"""
        self._require_schedule()
        if not self.config.skip_prk_steps and len(self.ets) < 3:
            raise ValueError(f"{self.__class__} can only be run AFTER scheduler has been run in 'prk' mode for at least 12 iterations "
                             "See: https://github.com/huggingface/diffusers/blob/main/src/diffusers/pipelines/pipeline_pndm.py "
                             "for more information.")
        ratio = self.config.num_train_timesteps // self.num_inference_steps
        timestep = int(timestep)
        prev_timestep = timestep - ratio
        if self.counter != 1:
            self.ets = self.ets[-3:]
            self.ets.append(model_output)
        else:
            prev_timestep, timestep = timestep, timestep + ratio
        if len(self.ets) == 1 and self.counter == 0:
            self.cur_sample = sample
            weights, terms = PLMS_WEIGHTS[1], (model_output,)
        elif len(self.ets) == 1 and self.counter == 1:
            sample, self.cur_sample = self.cur_sample, None
            weights, terms = (0.5, 0.5), (model_output, self.ets[-1])
        else:
            weights, terms = PLMS_WEIGHTS[len(self.ets)], tuple(self.ets[::-1])
        ev = PNDMEval(self.counter, timestep, prev_timestep, len(weights), weights, (), None, False, False, False, False, 0.0)
        prev = self._prev_sample(ev, sample, terms)
        self.counter += 1
        return (prev,) if not return_dict else SchedulerOutput(prev_sample=prev)

    def add_noise(self, original_samples: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor) -> torch.Tensor:
        abar = self.alphas_cumprod.to(device=original_samples.device, dtype=original_samples.dtype)[timesteps.to(original_samples.device)]
        shape = (-1,) + (1,) * (original_samples.dim() - 1)
        return (abar ** 0.5).reshape(shape) * original_samples + ((1 - abar) ** 0.5).reshape(shape) * noise

    def __len__(self):
        return self.config.num_train_timesteps
