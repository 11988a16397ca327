from .scheduling_ddim import DDIMScheduler  # noqa: F401
from .scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler  # noqa: F401
from .scheduling_euler_ancestral_discrete import EulerAncestralDiscreteScheduler  # noqa: F401
from .scheduling_euler_discrete import EulerDiscreteScheduler  # noqa: F401
from .scheduling_lms_discrete import LMSDiscreteScheduler  # noqa: F401
from .scheduling_pndm import PNDMScheduler  # noqa: F401
