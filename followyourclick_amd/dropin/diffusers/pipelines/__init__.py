from .stable_diffusion import (StableDiffusionImg2ImgPipeline, StableDiffusionInpaintPipeline, StableDiffusionInpaintPipelineLegacy,  # noqa: F401
                               StableDiffusionPipeline)
