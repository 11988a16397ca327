"""`diffusers.LMSDiscreteScheduler` surface (reference diffusers/schedulers/scheduling_lms_discrete.py:47-278) on the engine's host-side
tables; see scheduling_euler_discrete.py for what the pipeline uses of it.  The linear multistep coefficients are the closed-form
integrals of the Lagrange basis polynomials (engine/scheduler.py::SigmaTables.lms_coefficients): no scipy."""
from __future__ import annotations

import torch

from .scheduling_euler_discrete import SigmaSchedulerBase


class LMSDiscreteScheduler(SigmaSchedulerBase):
    kind = "lms"

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.derivatives = []

    def get_lms_coefficient(self, order, t, current_order):
        """the integral of the Lagrange basis polynomial `current_order` of an `order`-point step at schedule index t (reference :136-156)"""
        return self.tables.lms_coefficients(self._sigmas_host, t, order)[current_order]

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, order: int = 4, return_dict: bool = True):
        """one linear multistep update (reference :184-250): stateful as there (`derivatives`, reset by set_timesteps), up to `order` of them"""
        self._refuse_integer(timestep, "LMSDiscreteScheduler")
        self._require_schedule()
        if order not in (1, 2, 3, 4):
            raise ValueError(f"order given as {order} must be 1, 2, 3 or 4")
        i = self._index(timestep)
        used = min(i + 1, order, len(self.derivatives) + 1)
        out, d = self._update(i, used, model_output, sample, history=self.derivatives[::-1], return_dict=return_dict)
        self.derivatives.append(d)
        if len(self.derivatives) > order:
            self.derivatives.pop(0)
        return out
