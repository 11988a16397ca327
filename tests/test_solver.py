"""The DPM-Solver multistep scheduler without a GPU: SolverTables against the golden vectors of the reference's own class (tests/golden/dpm_solver*.npz, written by
tools/make_golden_solver.py), the golden, the drop-in's step() and the emulator (tests/emu_ops_solver.py) against the f64 specification (tests/solver_spec.py) inside
the bounds derived there, the zero-terminal-SNR first step, the C surface of fyc_cfg_solver_step (layout, tables, refusals), the routing through AnimationPipeline
and the multistep sampler on the emulator against a hand loop."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import solver_spec as SP
from emu_ops import EmuOps
from emu_ops_solver import SolverEmuOps
from followyourclick_amd.engine import DDIMConfig, SolverConfig, UNet3DConfig
from followyourclick_amd.engine.sampler import DDIMSampler, SolverSampler, make_sampler
from followyourclick_amd.engine.scheduler import SolverTables
from followyourclick_amd.engine.unet3d import UNet3DEngine
from followyourclick_amd.engine.weights import pack_unet
from oracle import functional as Fn
from oracle import weights as W

FILES = {"plain": "dpm_solver.npz", "zsnr": "dpm_solver_zero_snr.npz"}
PLAN_COUNTS = (4, 10, 14, 15, 25)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return {k: np.load(os.path.join(golden_dir, f)) for k, f in FILES.items()}


def config_of(betas, **family):
    return SolverConfig(**SP.BETAS, rescale_betas_zero_snr=betas == "zsnr", **family)


def tables_of(g):
    return {k: torch.from_numpy(g[k]) for k in ("alpha_t", "sigma_t", "lambda_t")}


# ---- tables, timesteps, the order plan ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("betas", ["plain", "zsnr"])
def test_tables_and_timesteps_are_the_reference_bits(golden, betas):
    g, tb = golden[betas], SolverTables(config_of(betas))
    for name in ("alpha_t", "sigma_t", "lambda_t"):
        assert torch.equal(getattr(tb, name), torch.from_numpy(g[name])), name           # (torch.equal: -inf == -inf, and no NaN anywhere)
        assert not torch.isnan(getattr(tb, name)).any()
    assert (tb.lambda_t[999].item() == float("-inf")) == (betas == "zsnr")
    for n in PLAN_COUNTS:
        assert np.array_equal(tb.timesteps(n).numpy(), g[f"timesteps_n{n}"]) and tb.timesteps(n).dtype == torch.int64
        assert np.array_equal(SP.timesteps(n), g[f"timesteps_n{n}"])


@pytest.mark.parametrize("order", SP.ORDERS)
def test_order_plan_is_the_reference(golden, order):
    """recorded from the reference's step() by wrapping its three update methods: warm-up from first order, lower orders at the end of a schedule shorter than 15"""
    tb = SolverTables(config_of("plain", solver_order=order))
    for n in PLAN_COUNTS:
        want = golden["plain"][f"orders_o{order}_n{n}"].tolist()
        assert tb.plan(n) == want and SP.plan(n, order) == want, (order, n)
    assert SolverTables(config_of("plain", solver_order=3)).plan(4) == [1, 2, 2, 1] and SolverTables(config_of("plain", solver_order=3)).plan(15)[-3:] == [3, 3, 3]
    assert SolverTables(config_of("plain", solver_order=3, lower_order_final=False)).plan(4) == [1, 2, 3, 3]


# ---- golden, drop-in and emulator against the specification ------------------------------------------------------------------------------------------------
def channels_last(v):
    """(B, C, F, h, w) -> the UNet's layout [B F HW][C]"""
    B, C = v.shape[:2]
    return v.reshape(B, C, -1).permute(0, 2, 1).reshape(-1, C).contiguous()


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


@pytest.mark.parametrize("betas", ["plain", "zsnr"])
def test_golden_dropin_and_emulator_inside_their_bounds(golden, dropin, betas):
    """Every step of every case starts from the reference's own previous output.  The golden (the reference's f32 result) lies inside the K_REFERENCE bound of the
    specification, the drop-in's step() and the emulator's cfg_solver_step inside the K_KERNEL bound, and therefore both inside the sum of the two of the golden."""
    from diffusers import DPMSolverMultistepScheduler
    g, tables, emu = golden[betas], tables_of(golden[betas]), SolverEmuOps()
    B, C, F, h, w = (SP.LATENT_SHAPE[0], SP.LATENT_SHAPE[1], 1, *SP.LATENT_SHAPE[2:])
    worst = dict(golden=0.0, dropin=0.0, emu=0.0)
    cases = [c for c in SP.golden_cases() if c.betas == betas]
    assert len(cases) == (108 if betas == "plain" else 36)
    for case in cases:
        fam, tag = SP.family(case), "/".join(map(str, case))
        prev = torch.from_numpy(g[SP.case_key(case)])
        xs, (_, vs) = SP.case_samples(case, prev), SP.case_inputs(case)
        tb = SolverTables(config_of(betas, **fam))
        ts, orders = tb.timesteps(case.n).tolist(), tb.plan(case.n)
        coef = tb.coefficient_table(case.n)
        assert torch.isfinite(coef).all(), tag
        sched = DPMSolverMultistepScheduler(**SP.BETAS, rescale_betas_zero_snr=betas == "zsnr", **fam)
        sched.set_timesteps(case.n)
        hist = [torch.full(SP.LATENT_SHAPE, float("nan")) for _ in range(3)]
        for i, t in enumerate(ts):
            ref, S = SP.schedule_step(tables, fam, ts, i, orders[i], xs, vs)
            b_ref, b_ker = SP.gamma(SP.K_REFERENCE) * S, SP.gamma(SP.K_KERNEL) * S
            worst["golden"] = max(worst["golden"], SP.inside(prev[i], ref, b_ref, f"golden {tag} step {i}"))
            got = sched.step(vs[i], t, xs[i]).prev_sample
            assert got.dtype == torch.float32
            worst["dropin"] = max(worst["dropin"], SP.inside(got, ref, b_ker, f"drop-in {tag} step {i}"))
            SP.inside(got, prev[i].double(), b_ref + b_ker, f"drop-in vs golden {tag} step {i}")
            lat = xs[i].clone()
            emu.cfg_solver_step(channels_last(vs[i].reshape(B, C, F, h, w)), lat, coef[i], hist_out=hist[i % 3], hist_1=hist[(i - 1) % 3], hist_2=hist[(i - 2) % 3],
                                order=orders[i], B=B, F=F, HW=h * w, c_latent=C, ld=C, cfg=False, guidance=1.0)
            worst["emu"] = max(worst["emu"], SP.inside(lat, ref, b_ker, f"emulator {tag} step {i}"))
            SP.inside(lat, prev[i].double(), b_ref + b_ker, f"emulator vs golden {tag} step {i}")
    print(f"{betas}: worst element / bound  golden {worst['golden']:.3f} (K = {SP.K_REFERENCE})  drop-in {worst['dropin']:.3f}  emulator {worst['emu']:.3f} (K = {SP.K_KERNEL})")


def test_zero_snr_first_step_and_refusals(golden):
    """at alphas_cumprod = 0 the first step is sigma_prev x + alpha_prev x0 and the next step's 1 / r0 is 0: finite coefficients, never inf * 0"""
    for order, stype, pred in [(o, s, p) for o in SP.ORDERS for s in SP.SOLVER_TYPES for p in ("v_prediction", "sample")]:
        tb = SolverTables(config_of("zsnr", solver_order=order, solver_type=stype, prediction_type=pred))
        for n in (4, 20):
            ts, coef = tb.timesteps(n).tolist(), tb.coefficient_table(n)
            assert ts[0] == 999 and torch.isfinite(coef).all()
            a_x, a_v, c_x, c_0, c_1, c_2 = coef[0, :6].tolist()
            assert (a_x, a_v) == ((0.0, -1.0) if pred == "v_prediction" else (0.0, 1.0))
            assert c_x == tb.sigma_t[ts[1]].item() and c_0 == tb.alpha_t[ts[1]].item() and c_1 == 0.0 and c_2 == 0.0
            if order >= 2:
                assert coef[1, 4].item() == 0.0 and tb.plan(n)[1] == 2              # 1 / r0 = 0: the second-order term of step 1 vanishes
    for bad in (dict(algorithm_type="dpmsolver", prediction_type="v_prediction"), dict(algorithm_type="dpmsolver", prediction_type="epsilon"),
                dict(algorithm_type="dpmsolver", prediction_type="sample"), dict(algorithm_type="dpmsolver++", prediction_type="epsilon")):
        tb = SolverTables(config_of("zsnr", **bad))
        with pytest.raises(ValueError, match="timestep 999"):
            tb.check_step(999)
        with pytest.raises(ValueError, match="timestep 999"):
            tb.coefficient_table(10)
        tb.check_step(899)
        smp = object.__new__(SolverSampler)                                       # the sampler refuses them before any launch
        smp.unet, smp.tables, smp.clip_sample = None, tb, False
        with pytest.raises(ValueError, match="timestep 999"):
            smp.prepare(torch.zeros(2, 77, 64), 10, 1, 8.0)
    SolverTables(config_of("plain", algorithm_type="dpmsolver")).coefficient_table(10)


def test_unsupported_options_and_duplicate_timesteps_are_refused(dropin):
    from diffusers import DPMSolverMultistepScheduler
    with pytest.raises(NotImplementedError, match="thresholding"):
        SolverTables(SolverConfig(thresholding=True))
    with pytest.raises(NotImplementedError, match="thresholding"):
        DPMSolverMultistepScheduler(thresholding=True)
    with pytest.raises(NotImplementedError, match="squaredcos_cap_v2"):
        SolverTables(SolverConfig(beta_schedule="squaredcos_cap_v2"))
    for kw in (dict(algorithm_type="deis"), dict(solver_type="bh1")):
        with pytest.raises(NotImplementedError):
            SolverTables(SolverConfig(**kw))
    with pytest.raises(ValueError, match="solver_order"):
        SolverTables(SolverConfig(solver_order=4))
    tb = SolverTables(SolverConfig())
    assert len(set(tb.timesteps(999).tolist())) == 999
    for n in (1000, 1500):                       # linspace(0, 999, n + 1) rounds two entries to the same timestep
        assert len(set(SP.timesteps(n).tolist())) < n
        with pytest.raises(ValueError, match=str(n)):
            tb.timesteps(n)
    with pytest.raises(ValueError, match="duplicate"):
        SolverTables(SolverConfig(num_train_timesteps=10, trained_betas=[0.01] * 10)).timesteps(12)


# ---- the emulator on the kernel's cases ------------------------------------------------------------------------------------------------------------------------
IDS = ["x".join(map(str, s)) for s in SP.SHAPES]


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape", SP.SHAPES, ids=IDS)
def test_emulator_on_the_kernel_cases(shape, dt):
    emu, nan = SolverEmuOps(), torch.full((shape[0], shape[3], shape[1], shape[2]), float("nan"))
    for var in SP.VARIANTS:
        ref, bound, m0, m0_bound = SP.reference(shape, dt, var)
        lat, out = SP.run_step(emu, shape, dt, var)
        SP.inside(lat, ref, bound, f"emu {shape} {dt} {var}")
        SP.inside(out, m0, m0_bound, f"emu m0 {shape} {dt} {var}")
        if var.order < 3:            # the histories the order does not read may hold anything
            o = SP.operands(shape, dt)
            lat2, out2 = SP.run_step(emu, shape, dt, var, hist=(o["hist_1"] if var.order == 2 else nan, nan))
            assert torch.equal(lat2, lat) and torch.equal(out2, out)
    assert {v.order for v in SP.VARIANTS} == {1, 2, 3} and {v.pred for v in SP.VARIANTS} == set(SP.PREDICTIONS)
    assert {(v.single, v.phi) for v in SP.VARIANTS} == {(False, 0.0), (False, 0.7), (True, 0.0), (True, 0.7)}


# ---- the C surface, no device ------------------------------------------------------------------------------------------------------------------------------
def _lib():
    from followyourclick_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib, _lib.load()


FIELDS = ["pred", "latents", "coef", "B", "F", "HW", "c_latent", "ld", "cfg", "guidance", "dtype", "pred_single", "video_scale", "hist_out", "hist_1", "hist_2",
          "order", "guidance_rescale", "workspace", "workspace_bytes"]


def test_binding_and_python_surface(tmp_path):
    from followyourclick_amd import _lib as L, ops
    assert [n for n, _ in L.CfgSolverArgs._fields_] == FIELDS
    assert L.FYC_VERSION == 308 and L.OPS["fyc_cfg_solver_step"] is L.CfgSolverArgs and "fyc_cfg_solver_workspace_bytes" in L.MISC
    header = os.path.join(os.path.dirname(L.HERE), "include", "fyc.h")
    with open(header) as fh:
        head = fh.read()
    assert "#define FYC_VERSION 308" in head and "} fyc_cfg_solver_args;" in head
    src = tmp_path / "abi.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{header}"\nint main(void){{printf("%zu %zu", sizeof(fyc_cfg_solver_args), sizeof(fyc_cfg_ddim_args));'
                   + "".join(f'printf(" %zu", offsetof(fyc_cfg_solver_args, {f}));' for f in FIELDS) + "return 0;}")
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    size, ddim, *offs = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == ctypes.sizeof(L.CfgSolverArgs) and ddim == ctypes.sizeof(L.CfgDdimArgs)          # the existing struct is untouched
    assert offs == [getattr(L.CfgSolverArgs, f).offset for f in FIELDS]
    lib = _lib()[1]
    assert lib.fyc_version() == 308 and hasattr(lib, "fyc_cfg_solver_step") and hasattr(lib, "fyc_cfg_solver_workspace_bytes")
    sig = inspect.signature(ops.HipOps.cfg_solver_step).parameters
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("hist_out", "hist_1", "hist_2", "order", "guidance_rescale"))
    assert list(inspect.signature(SolverEmuOps.cfg_solver_step).parameters) == list(sig)
    assert not hasattr(EmuOps, "cfg_solver_step")


LAT_BYTES = 2 * 4 * 16 * 1031 * 4


def _args(L, fields, shape=(2, 16, 1031, 4, 16)):
    """fyc_cfg_solver_args around a valid third-order problem with `fields` written over it"""
    a = L.CfgSolverArgs()
    a.pred, a.latents, a.coef = 0x10000000, 0x20000000, 0x30000000
    a.hist_out, a.hist_1, a.hist_2 = 0x50000000, 0x60000000, 0x70000000
    a.B, a.F, a.HW, a.c_latent, a.ld = shape
    a.cfg, a.guidance, a.dtype, a.order = 1, 8.0, 1, 3
    a.guidance_rescale, a.workspace, a.workspace_bytes = 0.7, 0x40000000, 1 << 20
    for k, v in fields.items():
        setattr(a, k, v)
    return a


BAD = [(dict(pred=None), b"null"), (dict(latents=None), b"null"), (dict(coef=None), b"null"), (dict(hist_out=None), b"null"),
       (dict(B=0), b"dims"), (dict(ld=3), b"dims"), (dict(dtype=7), b"dtype"),
       (dict(order=0), b"order"), (dict(order=4), b"order"), (dict(order=2, hist_1=None), b"hist_1"), (dict(hist_1=None), b"hist_1"), (dict(hist_2=None), b"hist_2"),
       (dict(hist_out=0x20000000), b"aliases latents"), (dict(hist_out=0x20000000 + LAT_BYTES - 4), b"aliases latents"), (dict(hist_out=0x60000000), b"aliases hist_1"),
       (dict(hist_out=0x70000000 - LAT_BYTES + 4), b"aliases hist_2"),
       (dict(cfg=0, guidance_rescale=0.0, pred_single=0x80000000), b"pred_single"),
       (dict(guidance_rescale=-0.1), b"guidance_rescale"), (dict(guidance_rescale=1.5), b"guidance_rescale"), (dict(guidance_rescale=float("nan")), b"guidance_rescale"),
       (dict(cfg=0), b"cfg"), (dict(workspace=None), b"workspace"), (dict(workspace_bytes=1095), b"workspace"), (dict(workspace=0x40000004), b"workspace"),
       (dict(F=1, HW=1, c_latent=1, ld=1), b"dims")]


@pytest.mark.parametrize("fields,word", BAD, ids=[",".join(f"{k}={v}" for k, v in b[0].items()) for b in BAD])
def test_bad_arguments_are_refused_by_the_library_without_gpu(fields, word):
    """refused before anything that needs a device or fyc_init (this process never calls fyc_init: a check behind it would report that instead)"""
    L, lib = _lib()
    assert lib.fyc_cfg_solver_step(ctypes.byref(_args(L, fields)), None) != 0
    msg = lib.fyc_last_error()
    assert word in msg and b"fyc_cfg_solver_step" in msg and b"fyc_init" not in msg, msg


def test_good_arguments_reach_the_init_check_and_the_query_launches_nothing():
    L, lib = _lib()
    for fields in (dict(), dict(order=1, hist_1=None, hist_2=None), dict(order=2, hist_2=None), dict(dtype=0), dict(dtype=2, ld=5, c_latent=3),
                   dict(pred_single=0x80000000, video_scale=0.3), dict(hist_out=0x20000000 + LAT_BYTES)):
        assert lib.fyc_cfg_solver_step(ctypes.byref(_args(L, fields)), None) != 0
        assert b"fyc_init" in lib.fyc_last_error(), (fields, lib.fyc_last_error())
    assert lib.fyc_cfg_solver_step(None, None) != 0 and b"null" in lib.fyc_last_error()
    # the workspace is the DDIM rescale's: 2 samples x 17 runs of 1024 rows x 4 f64, then 2 f32 factors, in 256-byte units
    assert lib.fyc_cfg_solver_workspace_bytes(ctypes.byref(_args(L, {}))) == 1280
    assert lib.fyc_cfg_solver_workspace_bytes(ctypes.byref(_args(L, dict(guidance_rescale=0.0)))) == 0
    assert lib.fyc_cfg_solver_workspace_bytes(ctypes.byref(_args(L, dict(B=0)))) == 0
    assert lib.fyc_cfg_solver_workspace_bytes(None) == 0


# ---- front ends --------------------------------------------------------------------------------------------------------------------------------------------
ZERO_SNR = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", prediction_type="v_prediction", rescale_betas_zero_snr=True)


def test_dropin_scheduler_surface(dropin, tmp_path):
    import diffusers
    from diffusers import DPMSolverMultistepScheduler
    from diffusers.schedulers import DPMSolverMultistepScheduler as same
    from diffusers.schedulers.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler as same2
    assert DPMSolverMultistepScheduler is same is same2 and "fyc" in diffusers.__version__
    s = DPMSolverMultistepScheduler()
    assert (s.config.beta_start, s.config.beta_end, s.config.solver_order, s.config.prediction_type, s.config.algorithm_type, s.config.solver_type,
            s.config.lower_order_final, s.config.rescale_betas_zero_snr) == (0.0001, 0.02, 2, "epsilon", "dpmsolver++", "midpoint", True, False)
    assert s.init_noise_sigma == 1.0 and s.order == 1 and len(s) == 1000 and isinstance(s.engine_config, SolverConfig)
    x = torch.randn(1, 4, 2, 2)
    assert s.scale_model_input(x, 5) is x
    with pytest.raises(ValueError, match="set_timesteps"):
        s.step(x, 999, x)
    kept = DPMSolverMultistepScheduler.from_config(dict(ZERO_SNR, solver_order=3, skip_prk_steps=True, steps_offset=1, clip_sample=False))
    assert kept.config.solver_order == 3 and kept.engine_config.rescale_betas_zero_snr and kept.lambda_t[999].item() == float("-inf")
    (tmp_path / "scheduler").mkdir()
    (tmp_path / "scheduler" / "scheduler_config.json").write_text('{"_class_name": "PNDMScheduler", "beta_schedule": "scaled_linear", "beta_start": 0.00085, "beta_end": 0.012, "skip_prk_steps": true}')
    ld = DPMSolverMultistepScheduler.from_pretrained(str(tmp_path), subfolder="scheduler", solver_type="heun")
    assert ld.config.beta_schedule == "scaled_linear" and ld.config.solver_type == "heun"
    # the state: set_timesteps resets it, two runs give the same bits
    kept.set_timesteps(5)
    assert kept.timesteps.tolist() == [999, 799, 599, 400, 200]
    v = torch.randn(5, 1, 4, 2, 2)

    def run():
        kept.set_timesteps(5)
        y, seen = x, []
        for i, t in enumerate(kept.timesteps):
            y = kept.step(v[i], t, y).prev_sample
            seen.append(kept.lower_order_nums)
        return y, seen
    (y1, seen), (y2, _) = run(), run()
    assert torch.equal(y1, y2) and torch.isfinite(y1).all() and seen == [1, 2, 3, 3, 3]
    assert kept.step(v[0], 200, x, return_dict=False)[0].shape == x.shape


MM = dict(num_attention_heads=8, num_transformer_block=1, attention_block_types=["Temporal_Self", "Temporal_Self"],
          temporal_position_encoding=True, temporal_position_encoding_max_len=24, temporal_attention_dim_div=1, zero_initialize=True)
TINY = dict(sample_size=8, in_channels=4, out_channels=4, block_out_channels=(64, 128, 256, 256), layers_per_block=2,
            cross_attention_dim=64, attention_head_dim=8, use_motion_module=True, motion_module_resolutions=(1, 2, 4, 8),
            unet_use_cross_frame_attention=False, unet_use_temporal_attention=False, use_fps_condition=True,
            use_first_frame_mask_condition_concat=True, motion_module_type="Vanilla", motion_module_kwargs=MM)


class Recording:
    """records the launches of an ops object by name (and the order / guidance_rescale a step carries), forwarding everything"""

    def __init__(self, inner):
        self.inner, self.names, self.steps = inner, [], []

    def __getattr__(self, name):
        v = getattr(self.inner, name)
        if not callable(v) or name == "ensure_init":
            return v

        def call(*a, **kw):
            self.names.append(name)
            if name.startswith("cfg_"):
                self.steps.append((name, kw.get("order"), kw.get("guidance_rescale"), kw.get("hist_out").data_ptr() if "hist_out" in kw else None))
            return v(*a, **kw)
        return call


def test_pipeline_routes_by_the_scheduler(dropin, monkeypatch):
    from animatediff.models.unet import UNet3DConditionModel
    from animatediff.pipelines.pipeline_animation import AnimationPipeline
    from diffusers import AutoencoderKL, DDIMScheduler, DPMSolverMultistepScheduler
    from followyourclick_amd import ops as ops_mod
    from oracle import stubs
    assert type(make_sampler(None, DDIMConfig())) is DDIMSampler and type(make_sampler(None, SolverConfig())) is SolverSampler
    with pytest.raises(TypeError, match="SolverConfig"):
        make_sampler(None, object())
    monkeypatch.delenv("FYC_GUIDANCE_RESCALE", raising=False)
    monkeypatch.setattr(AnimationPipeline, "decode_latents", lambda self, latents: np.zeros((1, 3, 2, 64, 64), np.float32))      # routing only: no VAE run
    vae = AutoencoderKL(block_out_channels=(64, 128, 128, 128), layers_per_block=2, latent_channels=4)

    def run(scheduler, ops, steps=4, **kw):
        pipe = AnimationPipeline(vae=vae, text_encoder=stubs.StubTextEncoder(64), tokenizer=stubs.FakeTokenizer(), unet=UNet3DConditionModel(**TINY), scheduler=scheduler)
        rec = Recording(ops)
        monkeypatch.setattr(ops_mod, "impl", rec)
        pipe("a corgi", video_length=2, height=64, width=64, num_inference_steps=steps, guidance_scale=8.0, use_first_frame_mask_condition_concat=True,
             first_image_latents=torch.zeros(1, 4, 8, 8), generator=torch.Generator().manual_seed(0), **kw)
        return rec

    ddim = run(DDIMScheduler(steps_offset=1, clip_sample=False, **ZERO_SNR), EmuOps())          # plain EmuOps has no cfg_solver_step: the old sampler never asks for it
    assert [s[0] for s in ddim.steps] == ["cfg_ddim_step"] * 4
    sol = run(DPMSolverMultistepScheduler(solver_order=3, **ZERO_SNR), SolverEmuOps(), eta=0.5)        # eta is accepted and unused, as in the reference
    assert [s[:3] for s in sol.steps] == [("cfg_solver_step", o, 0.0) for o in (1, 2, 2, 1)]
    assert len({s[3] for s in sol.steps[:3]}) == 3 and sol.steps[3][3] == sol.steps[0][3]            # three history buffers, their roles rotating
    assert [n for n in sol.names if not n.startswith("cfg_")] == [n for n in ddim.names if not n.startswith("cfg_")]      # the same input build and forward
    assert [s[2] for s in run(DPMSolverMultistepScheduler(**ZERO_SNR), SolverEmuOps(), guidance_rescale=0.7).steps] == [0.7] * 4
    monkeypatch.setenv("FYC_GUIDANCE_RESCALE", "0.7")
    assert [s[2] for s in run(DPMSolverMultistepScheduler(**ZERO_SNR), SolverEmuOps()).steps] == [0.7] * 4
    monkeypatch.delenv("FYC_GUIDANCE_RESCALE")
    with pytest.raises(ValueError, match="timestep 999"):
        run(DPMSolverMultistepScheduler(**dict(ZERO_SNR, prediction_type="epsilon")), SolverEmuOps())


def test_sd_pipeline_routes_by_the_scheduler(dropin, monkeypatch):
    """the 2-D first-image path goes through the same samplers: a solver scheduler makes its update launches cfg_solver_step"""
    from diffusers import AutoencoderKL, DDIMScheduler, DPMSolverMultistepScheduler, StableDiffusionPipeline, UNet2DConditionModel
    from followyourclick_amd import ops as ops_mod
    from oracle import stubs
    monkeypatch.setattr(StableDiffusionPipeline, "decode_latents", lambda self, latents: np.zeros((1, 64, 64, 3), np.float32))      # routing only: no VAE run
    vae = AutoencoderKL(block_out_channels=(64, 128, 128, 128))
    sd15 = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")

    def run(scheduler, ops):
        rec = Recording(ops)
        monkeypatch.setattr(ops_mod, "impl", rec)
        pipe = StableDiffusionPipeline(vae, stubs.StubTextEncoder(64), stubs.FakeTokenizer(), UNet2DConditionModel(sample_size=8, block_out_channels=(64, 128, 256, 256),
                                                                                                          cross_attention_dim=64), scheduler, safety_checker=None)
        pipe("a corgi", height=64, width=64, num_inference_steps=3, guidance_scale=8.0, generator=torch.Generator().manual_seed(0), output_type="np")
        return rec
    assert [s[0] for s in run(DDIMScheduler(steps_offset=1, clip_sample=False, set_alpha_to_one=False, **sd15), EmuOps()).steps] == ["cfg_ddim_step"] * 3
    assert [s[:2] for s in run(DPMSolverMultistepScheduler(**sd15), SolverEmuOps()).steps] == [("cfg_solver_step", o) for o in (1, 2, 1)]


# ---- the sampler on the emulator -------------------------------------------------------------------------------------------------------------------------
def test_solver_sampler_against_a_hand_loop(golden):
    """the tiny UNet of tests/test_engine_gpu.py, f32 on the emulator, 4 steps of DPM-Solver++(2M) on the zero-SNR betas with v_prediction.  The hand loop takes the
    emulator's forward (DDIMSampler.predict on an engine of its own), forms the guided prediction in f64 and steps with the specification on the golden's tables;
    per step the sampler stays below the f32 sampler bound of that file (1e-3 relative L2)."""
    ocfg = Fn.tiny_unet_config()
    cfg = UNet3DConfig(block_out_channels=(64, 128, 256, 256), cross_attention_dim=64, sample_size=8)
    sd = W.make_weights(W.unet_state_shapes(ocfg), 0)
    inp = W.seeded_inputs(ocfg, 1, 4, 8, 8, seed=7)
    fam = dict(algorithm_type="dpmsolver++", solver_order=2, solver_type="midpoint", prediction_type="v_prediction")
    scfg = config_of("zsnr", **fam)
    steps, guidance = 4, 8.0

    traj = []
    smp = SolverSampler(UNet3DEngine(pack_unet(sd, cfg, torch.float32, "cpu"), ops=SolverEmuOps()), scfg)
    out = smp.sample(inp["latents"], inp["text"], steps, guidance, inp["first_image_latents"], inp["first_images_mask"], fps=[2], flow=[4],
                     callback=lambda i, t, l: traj.append((t, l.clone())), use_graph=True, eta=0.3)          # use_graph and eta: accepted, unused
    assert [t for t, _ in traj] == [999, 749, 500, 250] and torch.equal(out, traj[-1][1])

    hand = SolverSampler(UNet3DEngine(pack_unet(sd, cfg, torch.float32, "cpu"), ops=SolverEmuOps()), scfg)
    st = hand.prepare(inp["text"], steps, 1, guidance, [2], [4])
    assert st["orders"] == [1, 2, 2, 1] and st["coef"].shape == (4, 8)
    tables, ts = tables_of(golden["zsnr"]), st["timesteps"].tolist()
    lat = inp["latents"].clone().float()
    B, CL, F, H, Wd = lat.shape
    first, mask = inp["first_image_latents"].reshape(B, CL, H * Wd).float(), inp["first_images_mask"].float()[:, :, 0].reshape(B, 1, H * Wd)
    xs, vs, errs = [], [], []
    for i in range(steps):
        pred, _ = hand.predict(st, i, lat, first, mask)
        p = pred.reshape(2, B, F, H * Wd, -1)[..., :CL].double()
        v = (p[0] + guidance * (p[1] - p[0])).permute(0, 3, 1, 2).reshape(lat.shape)
        xs.append(lat.clone())
        vs.append(v)
        ref, _ = SP.schedule_step(tables, fam, ts, i, st["orders"][i], xs, vs)
        errs.append(((traj[i][1].double() - ref).norm() / ref.norm()).item())
        lat = ref.float()
    print(f"solver sampler on the emulator vs hand loop: per-step rel-L2 {[f'{e:.2e}' for e in errs]}")
    assert torch.isfinite(out).all() and max(errs) < 1e-3, errs
    # another scheduler is another trajectory: the DDIM run on the same schedule parameters ends elsewhere
    ddim = DDIMSampler(UNet3DEngine(pack_unet(sd, cfg, torch.float32, "cpu"), ops=EmuOps()), DDIMConfig()).sample(
        inp["latents"], inp["text"], steps, guidance, inp["first_image_latents"], inp["first_images_mask"], fps=[2], flow=[4])
    assert ((ddim - out).norm() / out.norm()).item() > 1e-2
