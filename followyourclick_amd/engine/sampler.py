"""The DDIM sampling loop on the engine: latents in -> latents out.

Restates the hot loop of AnimationPipeline.__call__ (reference
animatediff/pipelines/pipeline_animation.py:686-773) for the mask + first-frame concat conditioning
with classifier-free guidance, and - for a UNet built without the concat conditioning - the loop of
StableDiffusionPipeline.__call__ (reference diffusers/pipelines/stable_diffusion/pipeline_stable_diffusion.py:522-541).  Per step: build the 9-channel channels-last input (one kernel instead
of 3 zeros_like + 2 cat), UNet forward on the CFG pair, guidance + DDIM update (one kernel, no host
sync).  Everything that is constant over the loop (text/IP K/V, all time embeddings, DDIM
coefficients) is prepared once per clip.  SolverSampler is the same loop for a DPM-Solver multistep scheduler
(the reference's loop is scheduler-agnostic): it shares the input build and the forward and differs in the schedule and the update kernel.
SigmaSampler is the loop for the sigma-space schedulers (Euler, Euler ancestral, LMS): the input build also divides by sqrt(sigma^2 + 1).
PNDMSampler is the loop for PNDM in its PLMS and Runge-Kutta modes: one pass per entry of its timestep list, n + 1 or n + 9 of them.
All four start part-way on request (`sample(start_index=k)`: the img2img / legacy inpainting `strength`, reference
pipeline_stable_diffusion_img2img.py:393-400) and re-impose a known region after every step (`blend=`: ops.renoise_blend, the legacy inpainting loop).
"""
from __future__ import annotations

import os
from typing import Callable, Optional, Sequence

import torch

from .config import DDIMConfig, PNDMConfig, SigmaConfig, SolverConfig
from .scheduler import DDIMTables, PNDMTables, SigmaTables, SolverTables, check_start_index
from .unet3d import UNet3DEngine
from .weights import pad_channels

Tensor = torch.Tensor


def check_guidance_rescale(value, what: str = "guidance_rescale") -> float:
    """the factor phi of the guidance rescale (arXiv:2305.08891 section 3.4): 0 = off .. 1 = the conditional prediction's standard deviation"""
    try:
        phi = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{what} = {value!r} is not a number") from None
    if not 0.0 <= phi <= 1.0:           # (NaN fails both comparisons)
        raise ValueError(f"{what} = {value!r} must lie in [0, 1]")
    return phi


def resolve_guidance_rescale(value=None) -> float:
    """the caller's keyword, else the FYC_GUIDANCE_RESCALE environment switch (unset or empty = 0 = off): for front ends whose callers cannot pass the
    keyword (AnimationPipeline under the reference's scripts), read once per clip.  The sampler itself takes the number only."""
    if value is not None:
        return check_guidance_rescale(value)
    env = os.environ.get("FYC_GUIDANCE_RESCALE", "")
    return check_guidance_rescale(env, "FYC_GUIDANCE_RESCALE") if env.strip() else 0.0


class DDIMSampler:
    # What `sample`'s loop does with the caller's eta, generator, use_clipped_model_output and use_graph.  None: DDIM takes them as they are.
    # A scheduler whose step() takes none of them (the reference's prepare_extra_step_kwargs drops them) and whose buffers change roles per
    # step, so that nothing is replayed from a captured graph, says here whether it draws one noise tensor per step from the generator.
    noise_per_step: Optional[bool] = None

    def __init__(self, unet: UNet3DEngine, ddim: DDIMConfig):
        self.unet = unet
        self.tables = DDIMTables(ddim)
        self.clip_sample = bool(ddim.clip_sample)

    @staticmethod
    def _check_rescale(st: dict, guidance_rescale) -> float:
        phi = check_guidance_rescale(guidance_rescale)
        if phi > 0 and not st["cfg"]:
            raise ValueError(f"guidance_rescale = {phi} needs classifier-free guidance (guidance_scale > 1)")
        return phi

    @staticmethod
    def _state_buffers(slot: dict, latents: Tensor, names) -> dict:
        """the latent-shaped f32 buffers a sampler keeps in the clip's state, by name (a count: 0 .. count - 1): allocated when absent or of
        another shape or device"""
        names = range(names) if isinstance(names, int) else names
        if any(k not in slot or slot[k].shape != latents.shape or slot[k].device != latents.device for k in names):
            slot.update((k, torch.empty_like(latents)) for k in names)
        return slot

    @staticmethod
    def _guidance_kwargs(st: dict, latents: Tensor, pred: Tensor, single: Optional[Tensor], phi: float) -> dict:
        """the shape and guidance keywords every ops.cfg_*_step takes"""
        B, CL, F, H, W = latents.shape
        return dict(B=B, F=F, HW=H * W, c_latent=CL, ld=pred.shape[1], cfg=st["cfg"], guidance=st["guidance"], pred_single=single,
                    video_scale=st.get("video_scale", 0.0), guidance_rescale=phi)

    def schedule(self, num_steps: int, eta: float, use_clipped_model_output: bool, start_index: int = 0):
        """-> (timesteps, the host coefficient table [n][.] f32, further per-clip entries of the state `prepare` returns).  start_index = k > 0:
        entries k .. of the scheduler's timestep list and their rows - what the reference's img2img / legacy inpainting loops hand a scheduler
        whose state starts from zero (`strength`); every sampler's schedule follows its own scheduler class there"""
        k = check_start_index(start_index, num_steps)
        ts = self.tables.timesteps(num_steps)[k:]
        for t in ts.tolist():           # a step at abar_t = 0 (trailing spacing on a zero-SNR table) that would divide by it
            self.tables.check_step(t, use_clipped_model_output)
        coef_host = self.tables.coefficient_table(num_steps, eta)[k:]
        return ts, coef_host, dict(sigma=coef_host[:, 4].tolist())           # eta > 0: per-step std of the added noise (0 for eta = 0)

    @torch.no_grad()
    def prepare(self, text_embeddings: Tensor, num_steps: int, batch: int, guidance_scale: float,
                fps: Optional[Sequence[float]] = None, flow: Optional[Sequence[float]] = None,
                ip_tokens: Optional[Tensor] = None, video_scale: float = 0.0, frames: int = 0,
                first_frame_condition: bool = False, eta: float = 0.0, camera: Optional[Sequence[float]] = None,
                guidance_rescale: float = 0.0, use_clipped_model_output: bool = False, start_index: int = 0) -> dict:
        """text_embeddings: (cfg*batch, 77, D) with the unconditional half first (reference :397).
        start_index: the first entry of the timestep list this run takes (`schedule`); the state's rows are those of the entries taken.
        guidance_rescale (0 = off .. 1) is checked here and handed to every `step` by `sample`: the guided prediction of every sample is rescaled
        towards the standard deviation of its conditional one (ops.cfg_ddim_step_rescaled); it needs classifier-free guidance.  use_clipped_model_output is only checked here, against the schedule."""
        u = self.unet
        cfg_on = guidance_scale > 1.0
        guidance_rescale = check_guidance_rescale(guidance_rescale)
        if guidance_rescale > 0 and not cfg_on:
            raise ValueError(f"guidance_rescale = {guidance_rescale} needs classifier-free guidance (guidance_scale > 1, got {guidance_scale}): "
                             "without it there is no guided prediction to rescale")
        beff = batch * (2 if cfg_on else 1)
        if text_embeddings.shape[0] != beff:
            raise ValueError(f"text_embeddings batch {text_embeddings.shape[0]} != {beff}")
        ts, coef_host, sched = self.schedule(num_steps, eta, use_clipped_model_output, start_index)

        def dup(v):
            if v is None:
                return None
            v = [float(x) for x in v]
            if len(v) == 1:
                v = v * batch
            return v * 2 if cfg_on else v

        extra = {}
        if video_scale > 0 and cfg_on:
            # `video_scale` (reference :738-760): every frame is also denoised on its own, as a one-frame clip.  The reference
            # builds that call's text batch as cat([text_embeddings] * f).chunk(2)[0], i.e. single-frame clip j gets
            # text_embeddings[j mod 2B] - for B = 1 the frames alternate between the negative and the positive prompt - and
            # passes no fps / flow conditioning; both are reproduced as they are.
            nf = batch * frames
            idx = torch.arange(nf) % (2 * batch)
            u.prepare_context(text_embeddings[idx], None)
            _, temb_s = u.prepare_time_embeddings(ts.tolist(), None, None, nf)
            extra = dict(ctx_single=u.ctx_cache, temb_single=temb_s.reshape(len(ts), nf, -1), video_scale=float(video_scale))
        if first_frame_condition:
            # `use_first_frame_condition` (reference :691-692; unet.py:523-524): frame 0 of the latents is pinned to the clean
            # first-frame latents and every ResNet gives that frame the embedding of timestep 0
            if fps is not None:
                raise ValueError("use_first_frame_condition cannot be combined with fps conditioning (the reference's embeddings "
                                 "have mismatching batch sizes there)")
            _, temb0 = u.prepare_time_embeddings([0], None, None, 1)
            extra["temb_first"] = temb0
        u.prepare_context(text_embeddings, ip_tokens)
        emb, temb = u.prepare_time_embeddings(ts.tolist(), dup(fps), dup(flow), beff, camera=dup(camera))
        coef = coef_host.to(u.device)
        extra.update(sched)
        # (one row per entry of the timestep list: PNDM evaluates the UNet more often than it has steps)
        return dict(timesteps=ts, temb=temb.reshape(len(ts), beff, -1), coef=coef, cfg=cfg_on, beff=beff,
                    guidance=float(guidance_scale), steps=num_steps, batch=batch, ctx_main=u.ctx_cache,
                    guidance_rescale=guidance_rescale, start_index=int(start_index), **extra)

    @torch.no_grad()
    def predict(self, st: dict, i: int, latents: Tensor, first_image_latents: Optional[Tensor], mask: Optional[Tensor],
                input_denom: Optional[float] = None):
        """the part of a step every scheduler shares: pin frame 0 (first_frame_condition), build the UNet input, run the forward(s)
        -> (pred [cfg B F HW][ld], the per-frame unconditional prediction or None).  input_denom (a sigma-space scheduler's scale_model_input,
        sqrt(sigma^2 + 1)): the tensor handed to the UNet is divided by it (ops.unet_input_scaled); None: the launches of an alpha-space scheduler"""
        u, o = self.unet, self.unet.ops
        B, CL, F, H, W = latents.shape
        cp = pad_channels(u.cfg.conv_in_channels)
        dupn = 2 if st["cfg"] else 1
        # the CFG halves differ in their text states only (`prepare` duplicates fps / flow / camera): where the engine can run the UNet
        # up to the first cross-attention once, the input holds the B distinct clips and nothing is duplicated here
        share = st["cfg"] and u.shares_prefix(dupn * B, st.get("temb_first"))
        dupx = 1 if share else dupn
        x = u.new(dupx * B * F * H * W, cp)
        if "temb_first" in st:
            latents[:, :, 0] = first_image_latents.reshape(B, CL, H, W)
        # (same precedence as UNet3DConfig.conv_in_channels / pack_unet and the reference's constructor, unet.py:114-126: the 8-channel
        # concat wins when both flags are set - the mask flag defaults to True)
        if u.cfg.use_first_frame_condition_concat:
            # the reference's UNet concatenates `reference_images_latent` (the clean first-frame latents) beside EVERY frame's latents
            # (unet.py:580-586; pipeline_animation.py:705-706 passes the plain latents); conv_in's `/ 2` lives in its packed weights
            # (a sigma-space scheduler scales the pipeline's tensor, the plain latents: the clean first-frame latents stay undivided)
            if input_denom is None:
                o.unet_input(latents, None, first_image_latents, x, B=B, F=F, HW=H * W, c_latent=CL, c_pad=cp, cfg_dup=dupx, mode=1)
            else:
                o.unet_input_scaled(latents, None, first_image_latents, x, denom=input_denom, scale_cond=False, B=B, F=F, HW=H * W,
                                    c_latent=CL, c_pad=cp, cfg_dup=dupx, mode=1)
        elif u.cfg.use_first_frame_mask_condition_concat:
            if input_denom is None:
                o.unet_input(latents, mask, first_image_latents, x, B=B, F=F, HW=H * W, c_latent=CL, c_pad=cp, cfg_dup=dupx,
                             mask_frames=1)
            else:       # the reference scales the concatenated tensor (pipeline_animation.py:708-712): mask and first-frame block too;
                # the 2-D inpainting pipeline scales the latents before the concat (scale_condition = False)
                o.unet_input_scaled(latents, mask, first_image_latents, x, denom=input_denom, scale_cond=st.get("scale_condition", True), B=B, F=F, HW=H * W,
                                    c_latent=CL, c_pad=cp, cfg_dup=dupx, mask_frames=1)
        else:
            # plain latents (the 2-D Stable Diffusion first-image path, reference pipeline_stable_diffusion.py:527-528)
            n = B * F * H * W
            frames = latents.permute(0, 2, 1, 3, 4).reshape(B * F, CL, H * W).contiguous()
            # (sigma-space: times the f32 reciprocal - one rounding more than the reference's division)
            scale = 1.0 if input_denom is None else float(torch.tensor(1.0) / torch.tensor(input_denom, dtype=torch.float32))
            for d in range(dupx):
                o.nchw_to_nhwc(frames, x[d * n:(d + 1) * n], N=B * F, C_=CL, HW=H * W, c_pad=cp, scale=scale)
        if share:
            pred = u.forward(x, st["temb"][i], dupn * B, F, H, W, shared_prefix=2)
        else:
            pred = u.forward(x, st["temb"][i], dupn * B, F, H, W, temb_first=st.get("temb_first"))
        single = None
        if "ctx_single" in st:      # per-frame unconditional pass: the first (unconditional) half of x as B*F one-frame clips
            u.ctx_cache = st["ctx_single"]
            single = u.forward(x[: B * F * H * W], st["temb_single"][i], B * F, 1, H, W)
            u.ctx_cache = st["ctx_main"]
        return pred, single

    @torch.no_grad()
    def step(self, st: dict, i: int, latents: Tensor, first_image_latents: Optional[Tensor], mask: Optional[Tensor],
             variance_noise: Optional[Tensor] = None, use_clipped_model_output: bool = False,
             guidance_rescale: float = 0.0) -> None:
        """one DDIM step, latents (B,4,F,h,w) f32 updated in place.  guidance_rescale = 0: ops.cfg_ddim_step as ever; above 0: ops.cfg_ddim_step_rescaled.  variance_noise (latents' shape, f32): the noise of a stochastic
        step (eta > 0, reference scheduling_ddim.py:346-363), scaled by the step's sigma from `prepare(eta=...)`."""
        o = self.unet.ops
        B, CL, F, H, W = latents.shape
        pred, single = self.predict(st, i, latents, first_image_latents, mask)
        kw = dict(B=B, F=F, HW=H * W, c_latent=CL, ld=pred.shape[1], cfg=st["cfg"],
                  guidance=st["guidance"], pred_type=self.tables.pred_type, clip_sample=self.clip_sample,
                  pred_single=single, video_scale=st.get("video_scale", 0.0),
                  variance_noise=variance_noise, sigma=st["sigma"][i] if variance_noise is not None else 0.0,
                  clipped_model_output=use_clipped_model_output)
        phi = self._check_rescale(st, guidance_rescale)
        if phi > 0:             # two more launches (moments, factor) in front of the step; an ops object without the method cannot run it
            o.cfg_ddim_step_rescaled(pred, latents, st["coef"][i], guidance_rescale=phi, **kw)
        else:
            o.cfg_ddim_step(pred, latents, st["coef"][i], **kw)

    @torch.no_grad()
    def sample(self, latents: Tensor, text_embeddings: Tensor, num_steps: int, guidance_scale: float,
               first_image_latents: Optional[Tensor] = None, first_images_mask: Optional[Tensor] = None,
               fps: Optional[Sequence[float]] = None, flow: Optional[Sequence[float]] = None,
               ip_tokens: Optional[Tensor] = None, callback: Optional[Callable] = None, callback_steps: int = 1,
               use_graph: Optional[bool] = None, video_scale: float = 0.0, first_frame_condition: bool = False,
               eta: float = 0.0, generator=None, use_clipped_model_output: bool = False,
               camera: Optional[Sequence[float]] = None, guidance_rescale: float = 0.0, start_index: int = 0,
               blend: Optional[Sequence[Tensor]] = None, scale_condition: bool = True) -> Tensor:
        """use_graph: replay steps 1..n-1 from one captured hipGraph (None = the FYC_HIPGRAPH environment switch, default off).
        Measured on MI355X it buys nothing: at cfg2 the loop is GPU-bound (56 ms of kernels per step) and even the 2-D
        one-frame case (13.7 ms / step, ~700 small kernels) is bound by the kernels' own execution, not by launch overhead
        (profiles/r01_front_end_rows.json).  Kept as an option for hosts with slow Python.
        start_index = k: entries k .. of the timestep list (`strength` of the img2img / legacy inpainting pipelines); the latents are the
        noised start latents of entry k as they are.  blend = (orig, noise, mask): after the step kernel of every entry the known region is
        re-imposed, latents = (c_x orig + c_n noise) mask + latents (1 - mask) (ops.renoise_blend) with (c_x, c_n) the add_noise
        coefficients of that entry's own timestep (reference pipeline_stable_diffusion_inpaint_legacy.py:573-575); orig and noise
        (B, C, h, w) or the latents' shape, mask (B, 1, h, w) or (B, C, h, w) with equal channels.  Either one runs the eager loop.
        scale_condition = False: a sigma-space scheduler's divisor reaches the latents only, not the mask and image channels of the concat
        input (the 2-D inpainting pipeline scales before it concatenates, pipeline_stable_diffusion_inpaint.py:699-703)."""
        u = self.unet
        if self.noise_per_step is not None:
            eta, use_clipped_model_output, use_graph = (1.0 if self.noise_per_step else 0.0), False, False
            generator = generator if self.noise_per_step else None
        latents = latents.to(device=u.device, dtype=torch.float32).contiguous().clone()
        B, CL, F, H, W = latents.shape
        first = None if first_image_latents is None else first_image_latents.to(u.device, torch.float32).reshape(B, CL, H * W).contiguous()
        mask = None
        if first_images_mask is not None:
            # mask for ALL frames = clamp(first_images_mask[:, :, 0:1]) (reference :632-635)
            mask = first_images_mask.to(u.device, torch.float32)[:, :, 0].reshape(B, 1, H * W).contiguous()
        st = self.prepare(text_embeddings, num_steps, B, guidance_scale, fps, flow, ip_tokens, video_scale=video_scale, frames=F,
                          first_frame_condition=first_frame_condition, eta=eta, camera=camera, guidance_rescale=guidance_rescale,
                          use_clipped_model_output=use_clipped_model_output, start_index=start_index)
        if not scale_condition:
            st["scale_condition"] = False
        ts, phi = st["timesteps"].tolist(), st["guidance_rescale"]
        if use_graph is None:
            use_graph = os.environ.get("FYC_HIPGRAPH", "0") == "1"
        if eta > 0:
            use_graph = False             # the noise of every step comes from the generator: nothing to replay
        blend_co = None
        if blend is not None:
            orig, bnoise, bmask = blend
            orig, bnoise = [t.to(u.device, torch.float32).reshape(B, CL, -1, H * W).contiguous() for t in (orig, bnoise)]
            if orig.shape != bnoise.shape or orig.shape[2] not in (1, F):
                raise ValueError(f"blend: orig {tuple(blend[0].shape)} and noise {tuple(blend[1].shape)} must be (B, C, h, w) or the latents' shape")
            bmask = bmask.to(u.device, torch.float32).reshape(B, -1, H * W)
            if bmask.shape[1] > 1 and not bool((bmask == bmask[:, :1]).all()):
                raise ValueError("blend: the mask's channels differ; the kernel broadcasts one mask over the channels")
            bmask = bmask[:, :1].contiguous()
            blend_co = [self.tables.add_noise_coefficients(t, num_steps) for t in ts]
        if start_index > 0 or blend is not None:
            use_graph = False             # a sliced or blended run is the eager loop
        if not (use_graph and latents.is_cuda and num_steps >= 3):
            for i, t in enumerate(ts):
                noise = None
                if eta > 0:
                    # drawn exactly as the reference's scheduler draws it (scheduling_ddim.py:355-361): on the latents' device, in
                    # their dtype, from the caller's generator (or the device's global one); a generator of another device (a seeded CPU
                    # one beside latents on the GPU, which the reference's call refuses) draws on its own device
                    gdev = latents.device if generator is None else generator.device
                    noise = torch.randn(latents.shape, generator=generator, device=gdev, dtype=latents.dtype).to(latents.device)
                self.step(st, i, latents, first, mask, variance_noise=noise, use_clipped_model_output=use_clipped_model_output, guidance_rescale=phi)
                if blend_co is not None:
                    u.ops.renoise_blend(latents, orig, bnoise, bmask, c_x=blend_co[i][0], c_n=blend_co[i][1], B=B, C_=CL, F=F, HW=H * W)
                if callback is not None and i % callback_steps == 0:
                    callback(i, t, latents)
            return latents
        # Step 0 runs eagerly (it is also the warm-up: lazily set kernel attributes, allocator pools); step 1 is captured
        # reading its time-embedding row and DDIM coefficients from two fixed buffers, which are refreshed before every replay.
        self.step(st, 0, latents, first, mask, use_clipped_model_output=use_clipped_model_output, guidance_rescale=phi)
        if callback is not None:
            callback(0, ts[0], latents)
        temb_cur, coef_cur = torch.empty_like(st["temb"][0]), torch.empty_like(st["coef"][0])
        gst = dict(st, temb=temb_cur[None], coef=coef_cur[None])
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(device=u.device)
        side.wait_stream(torch.cuda.current_stream(u.device))
        with torch.cuda.graph(graph, stream=side):
            self.step(gst, 0, latents, first, mask, use_clipped_model_output=use_clipped_model_output, guidance_rescale=phi)
        for i in range(1, num_steps):
            temb_cur.copy_(st["temb"][i])
            coef_cur.copy_(st["coef"][i])
            graph.replay()
            if callback is not None and i % callback_steps == 0:
                callback(i, ts[i], latents)
        return latents


class SolverSampler(DDIMSampler):
    """The same loop with a DPM-Solver multistep scheduler (engine/scheduler.py::SolverTables; the reference's loop is scheduler-agnostic,
    pipeline_animation.py:712, :767).  Input build and UNet forward are DDIMSampler.predict; `prepare` differs in the schedule (linspace
    timesteps, the per-step order, the table of collapsed coefficients) and the update is ops.cfg_solver_step.  The sampler owns three
    latent-shaped f32 history buffers (the converted outputs of this step and of the two before) and rotates their roles per step; because
    those pointers change per step nothing is replayed from a captured graph.  eta, generator and use_clipped_model_output are accepted and
    unused, as the reference's prepare_extra_step_kwargs drops them for a scheduler whose step() does not take them; there is no clip_sample."""

    noise_per_step = False

    def __init__(self, unet: UNet3DEngine, solver: SolverConfig):
        self.unet = unet
        self.tables = SolverTables(solver)
        self.clip_sample = False

    def schedule(self, num_steps: int, eta: float, use_clipped_model_output: bool, start_index: int = 0):
        k = check_start_index(start_index, num_steps)
        ts = self.tables.timesteps(num_steps)[k:]
        coef_host = self.tables.coefficient_table(num_steps, k)          # (checks every step: a zero-SNR first step the family cannot take)
        return ts, coef_host, dict(orders=self.tables.plan(num_steps, k), hist={})

    @torch.no_grad()
    def step(self, st: dict, i: int, latents: Tensor, first_image_latents: Optional[Tensor], mask: Optional[Tensor],
             variance_noise: Optional[Tensor] = None, use_clipped_model_output: bool = False,
             guidance_rescale: float = 0.0) -> None:
        """one solver step, latents (B,4,F,h,w) f32 updated in place; the steps of a clip are taken in order from i = 0 (the history is the state)"""
        phi = self._check_rescale(st, guidance_rescale)
        hist = self._state_buffers(st["hist"], latents, 3)
        pred, single = self.predict(st, i, latents, first_image_latents, mask)
        order = st["orders"][i]
        self.unet.ops.cfg_solver_step(pred, latents, st["coef"][i], hist_out=hist[i % 3], hist_1=hist[(i - 1) % 3] if order >= 2 else None,
                                      hist_2=hist[(i - 2) % 3] if order == 3 else None, order=order,
                                      **self._guidance_kwargs(st, latents, pred, single, phi))


class SigmaSampler(DDIMSampler):
    """The same loop with a sigma-space scheduler: Euler, Euler ancestral or LMS (engine/scheduler.py::SigmaTables).  `prepare` is shared; the
    schedule has fractional timesteps, per-step input denominators sqrt(sigma^2 + 1) handed to `predict`, and the table of collapsed
    coefficients; the update is ops.cfg_sigma_step.  LMS owns four latent-shaped f32 history buffers (the derivative of this step and of the
    three before) and rotates their roles per step; the Euler kinds store none.  The ancestral kind draws one noise tensor per step from the
    caller's generator, as the eta > 0 DDIM path does.  Nothing is replayed from a captured graph; eta and use_clipped_model_output are
    accepted and unused, as the reference's prepare_extra_step_kwargs drops them for these schedulers; there is no clip_sample.  The latents
    handed to `sample` are in sigma space: the caller has multiplied the initial noise by tables.init_noise_sigma."""

    def __init__(self, unet: UNet3DEngine, sigma: SigmaConfig):
        self.unet = unet
        self.tables = SigmaTables(sigma)
        self.clip_sample = False
        self.kind = sigma.kind
        self.noise_per_step = sigma.kind == "euler_ancestral"      # (as the eta > 0 DDIM path draws it)

    def schedule(self, num_steps: int, eta: float, use_clipped_model_output: bool, start_index: int = 0):
        k = check_start_index(start_index, num_steps)
        ts = self.tables.timesteps(num_steps)[k:]
        coef_host = self.tables.coefficient_table(num_steps, k)          # (refuses a schedule over an infinite sigma)
        # (a sliced LMS run: the order of the step's place in the list, cut to the derivatives stored since entry k - SigmaTables.plan)
        return ts, coef_host, dict(orders=self.tables.plan(num_steps, k), hist={}, input_denom=self.tables.input_denominators(num_steps)[k:])

    @torch.no_grad()
    def step(self, st: dict, i: int, latents: Tensor, first_image_latents: Optional[Tensor], mask: Optional[Tensor],
             variance_noise: Optional[Tensor] = None, use_clipped_model_output: bool = False,
             guidance_rescale: float = 0.0) -> None:
        """one step, latents (B,4,F,h,w) f32 updated in place; the steps of a clip are taken in order from i = 0 (LMS: the history is the state).
        variance_noise (latents' shape, f32): the noise of an ancestral step, scaled by the step's sigma_up"""
        phi = self._check_rescale(st, guidance_rescale)
        if (variance_noise is not None) != (self.kind == "euler_ancestral"):
            raise ValueError(f"the {self.kind} sampler takes {'a' if self.kind == 'euler_ancestral' else 'no'} noise tensor per step")
        hk = dict(order=1)
        if self.kind == "lms":
            hist, order = self._state_buffers(st["hist"], latents, 4), st["orders"][i]
            hk = dict(order=order, hist_out=hist[i % 4], hist_1=hist[(i - 1) % 4] if order >= 2 else None,
                      hist_2=hist[(i - 2) % 4] if order >= 3 else None, hist_3=hist[(i - 3) % 4] if order >= 4 else None)
        pred, single = self.predict(st, i, latents, first_image_latents, mask, input_denom=st["input_denom"][i])
        self.unet.ops.cfg_sigma_step(pred, latents, st["coef"][i], noise=variance_noise, **hk, **self._guidance_kwargs(st, latents, pred, single, phi))


class PNDMSampler(DDIMSampler):
    """The same loop with the PNDM scheduler (engine/scheduler.py::PNDMTables), PLMS mode (skip_prk_steps) or Runge-Kutta mode.  `prepare`
    and `predict` are shared; the schedule is the reference's timestep list - n + 1 entries in PLMS mode, n + 9 in Runge-Kutta mode, one UNet
    evaluation each: time embeddings, callbacks and the loop follow that list, not num_inference_steps -, the per-evaluation plan and the
    table of collapsed coefficients; the update is ops.cfg_pndm_step.  The sampler owns four latent-shaped f32 history buffers of guided
    predictions whose roles rotate by the plan, one buffer for the saved sample and one for the Runge-Kutta accumulator.  With
    use_first_frame_condition `predict` pins frame 0 before the input build, so the saved sample is the pinned one, as in the reference.
    Nothing is replayed from a captured graph; eta, generator and use_clipped_model_output are accepted and unused, as the reference's
    prepare_extra_step_kwargs drops them for this scheduler; there is no clip_sample."""

    noise_per_step = False

    def __init__(self, unet: UNet3DEngine, pndm: PNDMConfig):
        self.unet = unet
        self.tables = PNDMTables(pndm)
        self.clip_sample = False

    def schedule(self, num_steps: int, eta: float, use_clipped_model_output: bool, start_index: int = 0):
        plan = self.tables.plan(num_steps, start_index)               # (refuses a start part-way in Runge-Kutta mode)
        ts = self.tables.timesteps(num_steps)[start_index:]
        coef_host = self.tables.coefficient_table(num_steps, start_index)          # (refuses a step at alphas_cumprod = 0 with the timestep named)
        return ts, coef_host, dict(plan=plan, buffers={})

    @torch.no_grad()
    def step(self, st: dict, i: int, latents: Tensor, first_image_latents: Optional[Tensor], mask: Optional[Tensor],
             variance_noise: Optional[Tensor] = None, use_clipped_model_output: bool = False,
             guidance_rescale: float = 0.0) -> None:
        """evaluation i of the timestep list, latents (B,4,F,h,w) f32 updated in place; the evaluations of a clip are taken in order from
        i = 0 (the histories, the saved sample and the accumulator are the state)"""
        phi = self._check_rescale(st, guidance_rescale)
        buf = self._state_buffers(st["buffers"], latents, (0, 1, 2, 3, "sample", "acc"))      # (the plan's slots: a history 0 .. 3 or "acc")
        ev = st["plan"][i]
        hists = [buf[s] for s in ev.hist] + [None] * (4 - ev.order)
        pred, single = self.predict(st, i, latents, first_image_latents, mask)
        self.unet.ops.cfg_pndm_step(pred, latents, st["coef"][i], sample_in=buf["sample"] if ev.sample_in else None,
                                    sample_out=buf["sample"] if ev.sample_out else None,
                                    hist_out=None if ev.hist_out is None else buf[ev.hist_out], hist_1=hists[0], hist_2=hists[1],
                                    hist_3=hists[2], order=ev.order, acc_in=buf["acc"] if ev.acc_in else None,
                                    acc_out=buf["acc"] if ev.acc_out else None, **self._guidance_kwargs(st, latents, pred, single, phi))


def make_sampler(unet: UNet3DEngine, scheduler_config) -> DDIMSampler:
    """the sampler of a scheduler's engine_config: SolverConfig -> SolverSampler, SigmaConfig -> SigmaSampler, PNDMConfig -> PNDMSampler,
    DDIMConfig -> DDIMSampler"""
    if isinstance(scheduler_config, PNDMConfig):
        return PNDMSampler(unet, scheduler_config)
    if isinstance(scheduler_config, SolverConfig):
        return SolverSampler(unet, scheduler_config)
    if isinstance(scheduler_config, SigmaConfig):
        return SigmaSampler(unet, scheduler_config)
    if isinstance(scheduler_config, DDIMConfig):
        return DDIMSampler(unet, scheduler_config)
    raise TypeError(f"no sampler for a scheduler config of type {type(scheduler_config).__name__} (DDIMConfig, SolverConfig, SigmaConfig or PNDMConfig)")
