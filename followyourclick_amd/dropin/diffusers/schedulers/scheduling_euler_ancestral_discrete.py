"""`diffusers.EulerAncestralDiscreteScheduler` surface (reference diffusers/schedulers/scheduling_euler_ancestral_discrete.py:48-280) on
the engine's host-side tables; see scheduling_euler_discrete.py for what the pipeline uses of it."""
from __future__ import annotations

from typing import Optional

import torch

from .scheduling_euler_discrete import SigmaSchedulerBase


class EulerAncestralDiscreteScheduler(SigmaSchedulerBase):
    kind = "euler_ancestral"

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator: Optional[torch.Generator] = None,
             return_dict: bool = True):
        """one ancestral step (reference :159-250): down to sigma_down along the derivative, then sigma_up of fresh noise, drawn as the
        reference draws it (the model output's shape, dtype and device, from `generator`)"""
        self._refuse_integer(timestep, "EulerAncestralDiscreteScheduler")
        self._require_schedule()
        i = self._index(timestep)
        noise = torch.randn(model_output.shape, dtype=model_output.dtype, device=model_output.device, generator=generator)
        return self._update(i, 1, model_output, sample, noise=noise, return_dict=return_dict)[0]
