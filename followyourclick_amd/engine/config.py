"""Hyper-parameters of the hot path, named after the reference constructor arguments they mirror."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple, Union


@dataclass
class UNet3DConfig:
    """UNet3DConditionModel.__init__ (reference animatediff/models/unet.py:43-104) restricted to the
    options the shipped inference YAMLs exercise (configs/inference/*.yaml)."""
    sample_size: int = 64
    in_channels: int = 4
    out_channels: int = 4
    block_out_channels: Tuple[int, ...] = (320, 640, 1280, 1280)
    layers_per_block: int = 2
    cross_attention_dim: int = 768
    # = number of heads (reference unet_blocks.py:437-440); a tuple holds one count per down block (SD-2.1: (5, 10, 20, 20)): entry i in down
    # block i, the last entry in the mid block, the reversed tuple in the up blocks (reference unet.py:190-191, 212, 250, 282, 312)
    attention_head_dim: Union[int, Tuple[int, ...]] = 8
    # proj_in / proj_out of the spatial transformers are Linear (C, C) instead of 1x1 Conv2d (C, C, 1, 1) (reference attention.py:179-182,
    # 212-215, 270-300): the same arithmetic on token rows, another state-dict shape
    use_linear_projection: bool = False
    norm_num_groups: int = 32
    norm_eps: float = 1e-5
    down_block_types: Tuple[str, ...] = ("CrossAttnDownBlock3D", "CrossAttnDownBlock3D", "CrossAttnDownBlock3D", "DownBlock3D")
    up_block_types: Tuple[str, ...] = ("UpBlock3D", "CrossAttnUpBlock3D", "CrossAttnUpBlock3D", "CrossAttnUpBlock3D")
    use_motion_module: bool = True
    motion_module_resolutions: Tuple[int, ...] = (1, 2, 4, 8)
    motion_module_mid_block: bool = False
    motion_num_attention_heads: int = 8
    motion_num_transformer_block: int = 1
    motion_attention_blocks: int = 2
    temporal_position_encoding: bool = True
    temporal_position_encoding_max_len: int = 24
    # motion_module_kwargs.use_rope_postion_encoding / video_length / train_video_length (reference motion_module.py:335-353, rope.py:120-173):
    # q and k of the temporal attention are rotated per frame instead of adding the sinusoidal table to the tokens; the queries of a model
    # built for rope_video_length > rope_train_video_length carry the factor ln(train) / ln(video)
    use_rope_position_encoding: bool = False
    rope_video_length: int = 16
    rope_train_video_length: int = 16
    use_fps_condition: bool = True
    use_camera_motion_condition: bool = False      # camera_motion_embedding added to the time embedding (reference unet.py:134-137, 538-544)
    use_first_frame_mask_condition_concat: bool = True
    use_first_frame_condition_concat: bool = False
    # use_inflated_groupnorm (reference resnet.py:9-17, 237-263, unet.py:342-343): norm1 / norm2 of every ResNet and conv_norm_out take their
    # statistics per frame instead of per clip; use_temporal_conv (resnet.py:29-68, 288-294, 339-340): a TemporalConvBlock behind every ResNet
    use_inflated_groupnorm: bool = False
    use_temporal_conv: bool = False
    use_ip_cross_attention: bool = False
    ip_scale: float = 1.0
    ip_num_tokens: int = 4

    @property
    def conv_in_channels(self) -> int:
        if self.use_first_frame_condition_concat:
            return self.in_channels * 2
        if self.use_first_frame_mask_condition_concat:
            return self.in_channels * 2 + 1
        return self.in_channels

    @property
    def time_embed_dim(self) -> int:
        return self.block_out_channels[0] * 4

    def _heads(self) -> Tuple[int, ...]:
        h, nb = self.attention_head_dim, len(self.block_out_channels)
        if isinstance(h, int):
            return (h,) * nb
        if len(h) != nb:
            raise ValueError(f"attention_head_dim has {len(h)} entries for {nb} blocks")
        return tuple(int(v) for v in h)

    def down_heads(self, i: int) -> int:
        """head count of the transformers of down block i"""
        return self._heads()[i]

    def mid_heads(self) -> int:
        return self._heads()[-1]

    def up_heads(self, i: int) -> int:
        """head count of the transformers of up block i: the reversed list"""
        return self._heads()[::-1][i]

    def validate(self) -> None:
        nb = len(self.block_out_channels)
        for c in self.block_out_channels:
            if c % 64:
                raise ValueError(f"block_out_channels must be multiples of 64 (got {c}): K tiles of the MFMA GEMM are 64 bf16")
        # every (width, heads) pair a transformer can have: down block i, the mid block, up block i (width reversed with the heads)
        rev = self.block_out_channels[::-1]
        pairs = ([(self.block_out_channels[i], self.down_heads(i), self.down_block_types[i].startswith("CrossAttn")) for i in range(nb)]
                 + [(self.block_out_channels[-1], self.mid_heads(), True)]
                 + [(rev[i], self.up_heads(i), self.up_block_types[i].startswith("CrossAttn")) for i in range(nb)])
        for c, h, attends in pairs:
            if h < 1 or c % h or (c // h) % 8:
                raise ValueError(f"head dim {c}/{h} must be a multiple of 8")
            if attends and c // h > 160:
                raise ValueError(f"head dim {c}/{h} = {c // h} exceeds 160, the widest the attention kernels are built for")
        if self.use_rope_position_encoding and (self.rope_video_length < 2 or self.rope_train_video_length < 1):
            raise ValueError("rope_video_length must be >= 2 and rope_train_video_length >= 1 (the query factor is ln(train) / ln(video))")
        if self.cross_attention_dim % 8:
            raise ValueError("cross_attention_dim must be a multiple of 8")


@dataclass
class VAEDecoderConfig:
    """AutoencoderKL decoder half (reference diffusers/models/vae.py:147-206, 545-563)."""
    latent_channels: int = 4
    out_channels: int = 3
    block_out_channels: Tuple[int, ...] = (128, 256, 512, 512)
    layers_per_block: int = 2
    norm_num_groups: int = 32
    scaling_factor: float = 0.18215


@dataclass
class DDIMConfig:
    """DDIMScheduler.__init__ kwargs (reference diffusers/schedulers/scheduling_ddim.py:157-172);
    defaults = noise_scheduler_kwargs of the shipped YAML."""
    num_train_timesteps: int = 1000
    beta_start: float = 0.00085
    beta_end: float = 0.012
    beta_schedule: str = "linear"
    trained_betas: object = None
    clip_sample: bool = False
    set_alpha_to_one: bool = True
    steps_offset: int = 1
    prediction_type: str = "v_prediction"
    rescale_betas_zero_snr: bool = True
    # how the inference timesteps are spread over the training ones (later diffusers; arXiv:2305.08891 section 3.3): "leading" = the
    # reference's arange(n) * (T // n) + steps_offset, which never reaches T - 1; "trailing" starts at T - 1, the step a
    # zero-terminal-SNR model was trained to see pure noise at; "linspace" spreads T - 1 .. 0 evenly
    timestep_spacing: str = "leading"


@dataclass
class SolverConfig:
    """DPMSolverMultistepScheduler.__init__ kwargs (reference diffusers/schedulers/scheduling_dpmsolver_multistep.py:124-141) with the reference's
    defaults, plus rescale_betas_zero_snr (an engine extension: the reference's class has no such kwarg, the shipped checkpoints need it).
    thresholding (a per-sample quantile) and beta_schedule "squaredcos_cap_v2" are not implemented."""
    num_train_timesteps: int = 1000
    beta_start: float = 0.0001
    beta_end: float = 0.02
    beta_schedule: str = "linear"
    trained_betas: object = None
    solver_order: int = 2
    prediction_type: str = "epsilon"
    thresholding: bool = False
    algorithm_type: str = "dpmsolver++"
    solver_type: str = "midpoint"
    lower_order_final: bool = True
    rescale_betas_zero_snr: bool = False


@dataclass
class SigmaConfig:
    """EulerDiscreteScheduler / EulerAncestralDiscreteScheduler / LMSDiscreteScheduler.__init__ kwargs (reference diffusers/schedulers/
    scheduling_euler_discrete.py:79-87, the other two alike) with the reference's defaults, plus `kind` (which of the three) and
    rescale_betas_zero_snr (an engine extension as in SolverConfig: the tables use the rescaled betas and set alphas_cumprod[-1] = 2^-24, the
    convention later diffusers adopted for its sigma-space schedulers, so that sigma_max stays finite)."""
    kind: str = "euler"                 # "euler" | "euler_ancestral" | "lms"
    num_train_timesteps: int = 1000
    beta_start: float = 0.0001
    beta_end: float = 0.02
    beta_schedule: str = "linear"
    trained_betas: object = None
    prediction_type: str = "epsilon"
    rescale_betas_zero_snr: bool = False


@dataclass
class PNDMConfig:
    """PNDMScheduler.__init__ kwargs (reference diffusers/schedulers/scheduling_pndm.py:100-111) with the reference's defaults, plus
    rescale_betas_zero_snr (an engine extension as in SolverConfig).  skip_prk_steps = True is the PLMS mode Stable Diffusion 1.x ships
    (n + 1 evaluations of n steps); False, the class default, runs twelve Runge-Kutta evaluations first (n + 9 evaluations)."""
    num_train_timesteps: int = 1000
    beta_start: float = 0.0001
    beta_end: float = 0.02
    beta_schedule: str = "linear"
    trained_betas: object = None
    skip_prk_steps: bool = False
    set_alpha_to_one: bool = False
    prediction_type: str = "epsilon"
    steps_offset: int = 0
    rescale_betas_zero_snr: bool = False
