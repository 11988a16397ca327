from .pipeline_stable_diffusion import StableDiffusionPipeline, StableDiffusionPipelineOutput  # noqa: F401
from .pipeline_stable_diffusion_img2img import StableDiffusionImg2ImgPipeline  # noqa: F401
from .pipeline_stable_diffusion_inpaint import StableDiffusionInpaintPipeline  # noqa: F401
from .pipeline_stable_diffusion_inpaint_legacy import StableDiffusionInpaintPipelineLegacy  # noqa: F401
