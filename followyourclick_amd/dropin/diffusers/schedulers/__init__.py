from .scheduling_ddim import DDIMScheduler  # noqa: F401
from .scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler  # noqa: F401
