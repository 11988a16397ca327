"""Zero-SNR sampling without a GPU: the timestep spacings of DDIMTables and the drop-in scheduler, the first trailing step at alphas_cumprod = 0, the guidance
rescale on the emulator (tests/emu_ops_sampling.py) against the f64 specification (tests/sampling_spec.py) and through the sampler against a loop on the oracle's
UNet, the C surface of fyc_cfg_ddim_step_rescaled (layout, tables, refusals) and the routing of `guidance_rescale` / FYC_GUIDANCE_RESCALE through AnimationPipeline."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kernel_compare as KC
import sampling_spec as SS
from emu_ops import EmuOps
from emu_ops_sampling import SamplingEmuOps
from followyourclick_amd.engine import DDIMConfig, UNet3DConfig
from followyourclick_amd.engine.sampler import DDIMSampler
from followyourclick_amd.engine.scheduler import DDIMTables
from followyourclick_amd.engine.unet3d import UNet3DEngine
from followyourclick_amd.engine.weights import pack_unet
from kernel_compare import compare
from oracle import functional as Fn
from oracle import weights as W


# ---- timestep spacing --------------------------------------------------------------------------------------------------------------------------------------
def test_leading_is_the_default_and_unchanged(golden_dir):
    g = np.load(os.path.join(golden_dir, "ddim.npz"))
    assert DDIMConfig().timestep_spacing == "leading"
    tb, explicit = DDIMTables(DDIMConfig()), DDIMTables(DDIMConfig(timestep_spacing="leading"))
    assert torch.equal(tb.alphas_cumprod, torch.from_numpy(g["alphas_cumprod"]))
    for n in (5, 25, 50):
        assert np.array_equal(tb.timesteps(n).numpy(), g[f"timesteps_{n}"]) and torch.equal(tb.timesteps(n), explicit.timesteps(n))
        assert tb.timesteps(n).dtype == torch.int64
        assert np.array_equal(tb.timesteps(n).numpy(), SS.timesteps("leading", n, 1000, 1))
    assert tb.timesteps(25)[0].item() == 961                                # abar[999] = 0 is never sampled


def test_trailing_values():
    tb = DDIMTables(DDIMConfig(timestep_spacing="trailing"))
    assert tb.timesteps(25).tolist() == list(range(999, 0, -40))             # 999, 959, ..., 39: no steps_offset
    t30 = tb.timesteps(30).tolist()
    assert len(t30) == 30 and t30[:4] == [999, 966, 932, 899] and t30[-3:] == [99, 66, 32]
    assert tb.timesteps(30).dtype == torch.int64
    for n in (1, 2, 3, 7, 25, 30, 50, 999, 1000):
        assert np.array_equal(tb.timesteps(n).numpy(), SS.timesteps("trailing", n))
    # the previous timestep stays t - T // n, final_alpha_cumprod below 0: the last step returns x0
    c = tb.step_coefficients(39, 25)
    assert c[2] == 1.0 and c[3] == 0.0
    assert tb.step_coefficients(999, 25)[2] == float(tb.alphas_cumprod[959] ** 0.5)


def test_linspace_values():
    tb = DDIMTables(DDIMConfig(timestep_spacing="linspace"))
    t30 = tb.timesteps(30).tolist()
    assert len(t30) == 30 and t30[:4] == [999, 965, 930, 896] and t30[-3:] == [69, 34, 0]
    for n in (2, 3, 25, 50, 1000):
        assert np.array_equal(tb.timesteps(n).numpy(), SS.timesteps("linspace", n))


def test_bad_step_counts_and_spacings_are_refused():
    """np.arange(T, 0, -T / n) has n + 1 entries, the last one -1 after the shift, for 62 values of n up to 1000 (61, 103, 121, 122, 201, ...)"""
    tb = DDIMTables(DDIMConfig(timestep_spacing="trailing"))
    bad = [n for n in range(1, 1001) if len(SS.timesteps("trailing", n)) != n or SS.timesteps("trailing", n).min() < 0]
    assert bad[:5] == [61, 103, 121, 122, 201] and len(bad) == 62
    for n in (61, 103):
        with pytest.raises(ValueError, match=str(n)):
            tb.timesteps(n)
    assert all(len(set(SS.timesteps("trailing", n).tolist())) == len(SS.timesteps("trailing", n)) for n in range(1, 1001))      # never a duplicate
    with pytest.raises(ValueError, match="leading.*trailing.*linspace"):
        DDIMTables(DDIMConfig(timestep_spacing="karras")).timesteps(25)


def test_first_trailing_step_coefficients_and_refusals():
    tb = DDIMTables(DDIMConfig(timestep_spacing="trailing"))
    sa, sb, sap, sbp, sigma = tb.step_coefficients(999, 25)
    assert sa == 0.0 and sb == 1.0 and sigma == 0.0 and 0 < sap < 1 and 0 < sbp < 1
    assert all(np.isfinite(tb.step_coefficients(999, 25, eta=1.0)))         # eta > 0 stays valid: the variance is finite there
    tb.check_step(999)
    with pytest.raises(ValueError, match="999"):
        tb.check_step(999, use_clipped_model_output=True)
    eps_tb = DDIMTables(DDIMConfig(timestep_spacing="trailing", prediction_type="epsilon"))
    with pytest.raises(ValueError, match="999"):
        eps_tb.check_step(999)
    eps_tb.check_step(959)
    DDIMTables(DDIMConfig(timestep_spacing="trailing", prediction_type="sample")).check_step(999)
    # the sampler refuses them before any launch
    smp = object.__new__(DDIMSampler)
    smp.unet, smp.tables, smp.clip_sample = None, eps_tb, False
    with pytest.raises(ValueError, match="999"):
        smp.prepare(torch.zeros(2, 77, 64), 25, 1, 8.0)
    smp.tables = tb
    with pytest.raises(ValueError, match="999"):
        smp.prepare(torch.zeros(2, 77, 64), 25, 1, 8.0, use_clipped_model_output=True)


@pytest.fixture()
def dropin():
    import followyourclick_amd
    saved = {k: v for k, v in sys.modules.items() if k.split(".")[0] in ("animatediff", "diffusers", "ip_adapter")}
    path = list(sys.path)
    followyourclick_amd.install_dropin(force=True)
    yield
    for name in [k for k in sys.modules if k.split(".")[0] in ("animatediff", "diffusers", "ip_adapter")]:
        del sys.modules[name]
    sys.modules.update(saved)
    sys.path[:] = path


ZERO_SNR = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False,
                prediction_type="v_prediction", rescale_betas_zero_snr=True)


def test_dropin_scheduler_takes_the_spacing(dropin):
    from diffusers import DDIMScheduler
    s = DDIMScheduler(timestep_spacing="trailing", **ZERO_SNR)
    s.set_timesteps(25)
    assert s.timesteps.tolist() == list(range(999, 0, -40)) and s.config.timestep_spacing == "trailing"
    kept = DDIMScheduler.from_config(dict(ZERO_SNR, timestep_spacing="linspace", skip_prk_steps=True))
    assert kept.config.timestep_spacing == "linspace" and kept.engine_config.timestep_spacing == "linspace"
    assert DDIMScheduler(**ZERO_SNR).config.timestep_spacing == "leading"
    params = list(inspect.signature(DDIMScheduler.__init__).parameters)
    assert params[-2:] == ["timestep_spacing", "kwargs"]


def test_dropin_scheduler_step_at_the_last_timestep(dropin):
    from diffusers import DDIMScheduler
    s = DDIMScheduler(timestep_spacing="trailing", **ZERO_SNR)
    s.set_timesteps(25)
    g = torch.Generator().manual_seed(999)
    x, v = torch.randn(2, 4, 3, 8, 8, generator=g), torch.randn(2, 4, 3, 8, 8, generator=g)
    a_prev = s.alphas_cumprod[959].double()
    ref = a_prev.sqrt() * (-v.double()) + (1 - a_prev).sqrt() * x.double()      # abar_t = 0: x0 = -v, eps = x
    out = s.step(v, 999, x)
    assert torch.isfinite(out.prev_sample).all() and (out.prev_sample.double() - ref).abs().max().item() < 1e-6
    assert torch.equal(out.pred_original_sample, -v)
    with pytest.raises(ValueError, match="999"):
        s.step(v, 999, x, use_clipped_model_output=True)
    e = DDIMScheduler(timestep_spacing="trailing", **dict(ZERO_SNR, prediction_type="epsilon"))
    e.set_timesteps(25)
    with pytest.raises(ValueError, match="999"):
        e.step(v, 999, x)


# ---- the emulator against the specification ----------------------------------------------------------------------------------------------------------------
def labels(shape):
    return KC.Labels(row=lambda i: f"sample {i // shape[3]}, channel {i % shape[3]}", col=lambda j: f"frame-pixel {j}")


def run_step(ops, shape, dt, var, *, phi=None, on=lambda t: t):
    """one launch of the op under test on clones of the shared operands -> the latents [B c_latent][F HW]"""
    B, F, HW, CL, ld = shape
    o = SS.operands(shape, dt)
    lat = on(o["latents"].clone())
    ops.cfg_ddim_step_rescaled(on(o["pred"]), lat, on(o["coef"]), guidance_rescale=var.phi if phi is None else phi,
                               pred_single=on(o["single"]) if var.single else None, variance_noise=on(o["noise"]) if var.noise else None,
                               **SS.step_kwargs(shape, var))
    return lat.reshape(B * CL, F * HW)


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape", SS.SHAPES, ids=["x".join(map(str, s)) for s in SS.SHAPES])
def test_emulator_inside_the_bound_of_the_specification(shape, dt):
    emu = SamplingEmuOps()
    for var in SS.VARIANTS:
        ref, bound = SS.reference(shape, dt, var)
        compare(run_step(emu, shape, dt, var), ref, dtype="f32", bound=bound, rtol=KC.RTOL["f32"], labels=labels(shape), tag=f"emu {shape} {dt} {var}")
        if var.phi == 1.0:        # the whole point of phi = 1: the rescaled guided prediction has the conditional one's standard deviation
            B, F, HW, CL, ld = shape
            o = SS.operands(shape, dt)
            v, factor = emu.guided_rescaled(o["pred"], B=B, F=F, HW=HW, c_latent=CL, ld=ld, guidance=SS.GUIDANCE, guidance_rescale=1.0,
                                            pred_single=o["single"] if var.single else None, video_scale=SS.VIDEO_SCALE if var.single else 0.0)
            cond = o["pred"].reshape(2, B, -1, ld)[1, :, :, :CL].double()
            s_v, s_c = v.double().reshape(B, -1).std(dim=1), cond.reshape(B, -1).std(dim=1)
            assert ((s_v - s_c).abs() / s_c).max().item() < 4 * 2.0 ** -24, (s_v, s_c)
            assert (factor < 1.0).all()                                      # guidance 8 inflates the deviation: the rescale shrinks


def test_rescale_zero_is_the_plain_step_and_uniform_sample_keeps_factor_one():
    shape, dt, var = SS.SHAPES[0], "f32", SS.VARIANTS[2]
    B, F, HW, CL, ld = shape
    o = SS.operands(shape, dt)
    emu = SamplingEmuOps()
    plain = o["latents"].clone()
    EmuOps().cfg_ddim_step(o["pred"], plain, o["coef"], **SS.step_kwargs(shape, var))
    assert torch.equal(run_step(emu, shape, dt, var, phi=0.0), plain.reshape(B * CL, F * HW))
    pred = o["pred"].clone().reshape(2, B, F * HW, ld)
    pred[1, 0] = pred[0, 0]                                                 # sample 0: c == u, so v == c and the factor is exactly 1
    lat = o["latents"].clone()
    emu.cfg_ddim_step_rescaled(pred.reshape(-1, ld), lat, o["coef"], guidance_rescale=0.7, **SS.step_kwargs(shape, var))
    plain = o["latents"].clone()
    emu.cfg_ddim_step(pred.reshape(-1, ld), plain, o["coef"], **SS.step_kwargs(shape, var))
    assert torch.equal(lat[0], plain[0]) and not torch.equal(lat[1], plain[1])


# ---- the sampler on the emulator -------------------------------------------------------------------------------------------------------------------------
def tiny_cfg(**kw):
    return UNet3DConfig(block_out_channels=(64, 128, 256, 256), cross_attention_dim=64, sample_size=8, **kw)


def oracle_trailing_run(sd, ocfg, inp, steps, guidance, phi):
    """the DDIM loop of oracle/functional.py::denoise with sampling_spec's trailing timesteps and rescale_noise_cfg -> latents after every step"""
    sched = Fn.DDIMConfig()
    abar, lat, traj = Fn.ddim_alphas_cumprod(sched), inp["latents"], []
    with torch.no_grad():
        for t in SS.timesteps("trailing", steps).tolist():
            x = torch.cat([Fn.build_model_input(lat, inp["first_image_latents"], inp["first_images_mask"])] * 2)
            u, c = Fn.unet3d_forward(sd, ocfg, x, torch.tensor(t), inp["text"], torch.tensor([2, 2]), torch.tensor([4, 4])).chunk(2)
            v = SS.rescale_noise_cfg(c.double(), (u + guidance * (c - u)).double(), phi).float()
            lat = Fn.ddim_step(sched, abar, steps, v, t, lat)
            traj.append(lat.clone())
    return torch.stack(traj)


@pytest.fixture(scope="module")
def trailing_problem():
    ocfg = Fn.tiny_unet_config()
    sd = W.make_weights(W.unet_state_shapes(ocfg), 0)
    inp = W.seeded_inputs(ocfg, 1, 4, 8, 8, seed=7)
    return sd, inp, oracle_trailing_run(sd, ocfg, inp, 3, 8.0, 0.7)


def test_sampler_with_trailing_steps_and_guidance_rescale(trailing_problem):
    """3 trailing steps (999, 666, 332: the first one at alphas_cumprod = 0) with guidance_rescale 0.7, f32 engine on the emulator, under the bound of the f32
    sampler run of tests/test_engine_emulated.py (5e-4 relative L2 per step)"""
    sd, inp, ref = trailing_problem
    eng = UNet3DEngine(pack_unet(sd, tiny_cfg(), torch.float32, "cpu"), ops=SamplingEmuOps())
    traj = []
    smp = DDIMSampler(eng, DDIMConfig(timestep_spacing="trailing"))
    smp.sample(inp["latents"], inp["text"], 3, 8.0, inp["first_image_latents"], inp["first_images_mask"], fps=[2], flow=[4],
               callback=lambda i, t, l: traj.append((t, l.clone())), guidance_rescale=0.7)
    assert [t for t, _ in traj] == [999, 666, 332]
    got = torch.stack([l for _, l in traj])
    err = (got - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)
    assert torch.isfinite(got).all() and err.max().item() < 5e-4, err
    # the rescale is not a no-op on this problem, and an ops object without the method still runs everything with guidance_rescale = 0
    plain = DDIMSampler(UNet3DEngine(pack_unet(sd, tiny_cfg(), torch.float32, "cpu"), ops=EmuOps()), DDIMConfig(timestep_spacing="trailing")).sample(
        inp["latents"], inp["text"], 3, 8.0, inp["first_image_latents"], inp["first_images_mask"], fps=[2], flow=[4])
    assert ((plain - ref[-1]).norm() / ref[-1].norm()).item() > 1e-2
    with pytest.raises(ValueError, match="guidance_rescale"):
        smp.prepare(inp["text"][:1], 3, 1, 1.0, guidance_rescale=0.7)      # no classifier-free guidance: nothing to rescale
    with pytest.raises(ValueError, match="guidance_rescale"):
        smp.prepare(inp["text"], 3, 1, 8.0, guidance_rescale=1.5)


# ---- the C surface, no device ----------------------------------------------------------------------------------------------------------------------------
def _lib():
    from followyourclick_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib, _lib.load()


def test_binding_and_python_surface(tmp_path):
    from followyourclick_amd import _lib as L, ops
    assert [n for n, _ in L.CfgDdimRescaleArgs._fields_] == ["step", "guidance_rescale", "workspace", "workspace_bytes"]
    assert L.FYC_VERSION == 308 and L.OPS["fyc_cfg_ddim_step_rescaled"] is L.CfgDdimRescaleArgs and "fyc_cfg_ddim_rescale_workspace_bytes" in L.MISC
    assert L.CfgDdimArgs._fields_[-1][0] == "clipped_model_output"
    header = os.path.join(os.path.dirname(L.HERE), "include", "fyc.h")
    with open(header) as fh:
        head = fh.read()
    assert "#define FYC_VERSION 308" in head and "308, added entry points" in head
    assert "typedef struct { fyc_cfg_ddim_args step; float guidance_rescale; void* workspace; int64_t workspace_bytes; } fyc_cfg_ddim_rescale_args;" in head
    fields = ["step", "guidance_rescale", "workspace", "workspace_bytes"]
    src = tmp_path / "abi.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{header}"\nint main(void){{printf("%zu %zu", sizeof(fyc_cfg_ddim_rescale_args), sizeof(fyc_cfg_ddim_args));'
                   + "".join(f'printf(" %zu", offsetof(fyc_cfg_ddim_rescale_args, {f}));' for f in fields) + "return 0;}")
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    size, inner, *offs = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert (size, inner) == (ctypes.sizeof(L.CfgDdimRescaleArgs), ctypes.sizeof(L.CfgDdimArgs))
    assert offs == [getattr(L.CfgDdimRescaleArgs, f).offset for f in fields]
    sig = inspect.signature(ops.HipOps.cfg_ddim_step_rescaled)
    assert sig.parameters["guidance_rescale"].kind is inspect.Parameter.KEYWORD_ONLY
    plain = inspect.signature(ops.HipOps.cfg_ddim_step).parameters
    assert [p for p in sig.parameters if p != "guidance_rescale"] == list(plain)
    for fn in (DDIMSampler.prepare, DDIMSampler.step, DDIMSampler.sample):
        assert "guidance_rescale" in inspect.signature(fn).parameters


def _args(L, fields, shape=(2, 16, 1031, 4, 16)):
    """fyc_cfg_ddim_rescale_args around a valid problem with `fields` written over it (step's fields into .step)"""
    r = L.CfgDdimRescaleArgs()
    s = r.step
    s.pred, s.latents, s.coef = 0x10000000, 0x20000000, 0x30000000
    s.B, s.F, s.HW, s.c_latent, s.ld = shape
    s.cfg, s.guidance, s.pred_type, s.dtype = 1, 8.0, 1, 1
    r.guidance_rescale, r.workspace, r.workspace_bytes = 0.7, 0x40000000, 1 << 20
    for k, v in fields.items():
        setattr(r if k in ("guidance_rescale", "workspace", "workspace_bytes") else s, k, v)
    return r


BAD = [(dict(guidance_rescale=-0.1), b"guidance_rescale"), (dict(guidance_rescale=1.5), b"guidance_rescale"), (dict(guidance_rescale=float("nan")), b"guidance_rescale"),
       (dict(cfg=0), b"cfg"), (dict(workspace=None), b"workspace"), (dict(workspace_bytes=0), b"workspace"), (dict(workspace_bytes=1095), b"workspace"),
       (dict(workspace=0x40000004), b"workspace"), (dict(pred_type=3), b"pred_type"), (dict(B=0), b"dims"), (dict(F=1, HW=1, c_latent=1), b"dims")]


@pytest.mark.parametrize("fields,word", BAD, ids=[",".join(f"{k}={v}" for k, v in b[0].items()) for b in BAD])
def test_bad_arguments_are_refused_by_the_library_without_gpu(fields, word):
    """refused before anything that needs a device or fyc_init (this process never calls fyc_init: a check behind it would report that instead)"""
    L, lib = _lib()
    assert lib.fyc_cfg_ddim_step_rescaled(ctypes.byref(_args(L, fields)), None) != 0
    msg = lib.fyc_last_error()
    assert word in msg and b"fyc_init" not in msg, msg


def test_good_arguments_reach_the_init_check_and_the_query_launches_nothing():
    L, lib = _lib()
    for fields in (dict(), dict(guidance_rescale=1.0), dict(dtype=0), dict(dtype=2, ld=5), dict(pred_single=0x50000000, video_scale=0.3)):
        assert lib.fyc_cfg_ddim_step_rescaled(ctypes.byref(_args(L, fields)), None) != 0
        assert b"fyc_init" in lib.fyc_last_error(), lib.fyc_last_error()
    assert lib.fyc_cfg_ddim_step_rescaled(None, None) != 0 and b"null" in lib.fyc_last_error()
    # 2 samples x 17 runs of 1024 rows (16 x 1031 rows per sample) x 4 f64, then 2 f32 factors, in 256-byte units
    assert lib.fyc_cfg_ddim_rescale_workspace_bytes(ctypes.byref(_args(L, {}))) == 1280
    assert lib.fyc_cfg_ddim_rescale_workspace_bytes(ctypes.byref(_args(L, {}, (2, 3, 20, 4, 8)))) == 256
    assert lib.fyc_cfg_ddim_rescale_workspace_bytes(ctypes.byref(_args(L, dict(guidance_rescale=0.0)))) == 0
    assert lib.fyc_cfg_ddim_rescale_workspace_bytes(ctypes.byref(_args(L, dict(B=0)))) == 0
    assert lib.fyc_cfg_ddim_rescale_workspace_bytes(None) == 0
    assert lib.fyc_cfg_ddim_step_rescaled(ctypes.byref(_args(L, dict(workspace_bytes=1280))), None) != 0 and b"fyc_init" in lib.fyc_last_error()


# ---- AnimationPipeline ------------------------------------------------------------------------------------------------------------------------------------
MM = dict(num_attention_heads=8, num_transformer_block=1, attention_block_types=["Temporal_Self", "Temporal_Self"],
          temporal_position_encoding=True, temporal_position_encoding_max_len=24, temporal_attention_dim_div=1, zero_initialize=True)
TINY = dict(sample_size=8, in_channels=4, out_channels=4, block_out_channels=(64, 128, 256, 256), layers_per_block=2,
            cross_attention_dim=64, attention_head_dim=8, use_motion_module=True, motion_module_resolutions=(1, 2, 4, 8),
            unet_use_cross_frame_attention=False, unet_use_temporal_attention=False, use_fps_condition=True,
            use_first_frame_mask_condition_concat=True, motion_module_type="Vanilla", motion_module_kwargs=MM)


class Recording:
    """records the launches of an ops object by name (and the guidance_rescale they carry), forwarding everything"""

    def __init__(self, inner):
        self.inner, self.order, self.phi = inner, [], []

    def __getattr__(self, name):
        v = getattr(self.inner, name)
        if not callable(v) or name == "ensure_init":
            return v

        def call(*a, **kw):
            self.order.append(name)
            if "guidance_rescale" in kw:
                self.phi.append(kw["guidance_rescale"])
            return v(*a, **kw)
        return call


def test_pipeline_routes_the_keyword_and_the_environment_switch(dropin, monkeypatch):
    from animatediff.models.unet import UNet3DConditionModel
    from animatediff.pipelines.pipeline_animation import AnimationPipeline
    from diffusers import AutoencoderKL, DDIMScheduler
    from followyourclick_amd import ops as ops_mod
    from oracle import stubs
    monkeypatch.delenv("FYC_GUIDANCE_RESCALE", raising=False)
    monkeypatch.setattr(AnimationPipeline, "decode_latents", lambda self, latents: np.zeros((1, 3, 2, 64, 64), np.float32))      # routing only: no VAE run
    vae = AutoencoderKL(block_out_channels=(64, 128, 128, 128), layers_per_block=2, latent_channels=4)
    pipe = AnimationPipeline(vae=vae, text_encoder=stubs.StubTextEncoder(64), tokenizer=stubs.FakeTokenizer(), unet=UNet3DConditionModel(**TINY),
                             scheduler=DDIMScheduler(timestep_spacing="trailing", **ZERO_SNR))

    def run(ops, **kw):
        rec = Recording(ops)
        monkeypatch.setattr(ops_mod, "impl", rec)
        pipe.unet._engine = None                                            # the engine holds the ops object it was built with
        pipe("a corgi", video_length=2, height=64, width=64, num_inference_steps=2, guidance_scale=8.0, use_first_frame_mask_condition_concat=True,
             first_image_latents=torch.zeros(1, 4, 8, 8), generator=torch.Generator().manual_seed(0), **kw)
        return rec

    parent = run(EmuOps())                                                   # absent and unset: the launches as they were, on an ops object without the new method
    assert parent.order.count("cfg_ddim_step") == 2 and "cfg_ddim_step_rescaled" not in parent.order and parent.phi == []
    assert run(SamplingEmuOps()).order == parent.order
    want = [n if n != "cfg_ddim_step" else "cfg_ddim_step_rescaled" for n in parent.order]
    by_kw = run(SamplingEmuOps(), guidance_rescale=0.7)
    assert by_kw.order == want and by_kw.phi == [0.7, 0.7]
    monkeypatch.setenv("FYC_GUIDANCE_RESCALE", "0.7")
    by_env = run(SamplingEmuOps())
    assert by_env.order == want and by_env.phi == [0.7, 0.7]
    assert run(SamplingEmuOps(), guidance_rescale=0.0).order == parent.order      # the keyword wins over the switch
    monkeypatch.setenv("FYC_GUIDANCE_RESCALE", "1.5")
    with pytest.raises(ValueError, match="FYC_GUIDANCE_RESCALE"):
        run(SamplingEmuOps())
    monkeypatch.delenv("FYC_GUIDANCE_RESCALE")
    with pytest.raises(ValueError, match="guidance_rescale"):
        run(SamplingEmuOps(), guidance_rescale=1.5)
