"""The PNDM scheduler, PLMS and Runge-Kutta modes, without a GPU: PNDMTables against the golden vectors of the reference's own class (tests/golden/pndm.npz, written by
tools/make_golden_pndm.py), the golden, the drop-in's step() and the emulator (tests/emu_ops_pndm.py) against the f64 specification (tests/pndm_spec.py) inside the
bounds derived there, the refusals, the C surface of fyc_cfg_pndm_step (layout, refusals), the routing through the two pipelines, the sampler's launches on the
emulator and the reference pipeline's trajectories."""
import ctypes
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pndm_spec as SP
from emu_ops import EmuOps
from emu_ops_pndm import PNDMEmuOps
from emu_ops_sigma import SigmaEmuOps
from emu_ops_solver import SolverEmuOps
from followyourclick_amd.engine import DDIMConfig, PNDMConfig, SigmaConfig, SolverConfig, UNet3DConfig
from followyourclick_amd.engine.sampler import DDIMSampler, PNDMSampler, SigmaSampler, SolverSampler, make_sampler
from followyourclick_amd.engine.scheduler import PNDMTables
from followyourclick_amd.engine.unet3d import UNet3DEngine
from followyourclick_amd.engine.weights import pack_unet
from oracle import functional as Fn
from oracle import weights as W


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "pndm.npz"))


@pytest.fixture(scope="module")
def pipe_golden(golden_dir):
    return {k: torch.from_numpy(v) if v.shape else v for k, v in np.load(os.path.join(golden_dir, "pipeline_tiny_pndm.npz")).items()}


def config_of(betas, mode, **kw):
    kw.setdefault("steps_offset", SP.STEPS_OFFSET)
    return PNDMConfig(**SP.BETA_SETS[betas], rescale_betas_zero_snr=betas == "zsnr", skip_prk_steps=mode == "plms", **kw)


# ---- timesteps and the plan ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("betas", list(SP.BETA_SETS))
def test_timesteps_are_the_reference_bits(golden, betas):
    for mode in SP.MODES:
        tb = PNDMTables(config_of(betas, mode))
        for n in SP.STEP_COUNTS:
            ts = tb.timesteps(n)
            prk, plms = tb.split_timesteps(n)
            assert ts.dtype == torch.int64 and len(ts) == n + (1 if mode == "plms" else 9)
            assert np.array_equal(ts.numpy(), golden[f"{betas}/{mode}/timesteps_n{n}"]) and np.array_equal(ts.numpy(), SP.timesteps(mode, n, offset=SP.STEPS_OFFSET))
            assert np.array_equal(prk, golden[f"{betas}/{mode}/prk_timesteps_n{n}"]) and np.array_equal(plms, golden[f"{betas}/{mode}/plms_timesteps_n{n}"])
    # any steps_offset, read when the schedule is made (the pipelines patch it after construction)
    for mode in SP.MODES:
        cfg = config_of("linear", mode, steps_offset=0)
        tb = PNDMTables(cfg)
        for off in (0, 1, 7):
            cfg.steps_offset = off
            assert np.array_equal(tb.timesteps(10).numpy(), SP.timesteps(mode, 10, offset=off))
    assert PNDMTables(config_of("linear", "plms")).timesteps(5).tolist() == [801, 601, 601, 401, 201, 1]
    assert PNDMTables(config_of("linear", "plms")).timesteps(1).tolist() == [1]               # no second entry to repeat
    assert PNDMTables(config_of("linear", "prk")).timesteps(5).tolist() == [801, 701, 701, 601, 601, 501, 501, 401, 401, 301, 301, 201, 201, 1]


@pytest.mark.parametrize("mode", SP.MODES)
def test_plan_is_the_reference_state_machine(mode):
    """engine/scheduler.py::PNDMTables.plan against the state machine restated in the specification: the pair _get_prev_sample sees, the order, and - with the slots
    resolved to the evaluations that wrote them - which model outputs and which saved sample every evaluation uses"""
    for n in (1, 2, 3, 4, 5, 10, 25) if mode == "plms" else (4, 5, 10, 25):
        tb = PNDMTables(config_of("linear", mode))
        plan, spec = tb.plan(n), SP.schedule(mode, n, offset=SP.STEPS_OFFSET)
        assert len(plan) == len(spec) == len(tb.timesteps(n))
        writer, saved = {}, None
        for i, (ev, sp) in enumerate(zip(plan, spec)):
            assert (ev.counter, ev.timestep, ev.prev_timestep) == (i, sp.timestep, sp.prev_timestep) and ev.order == len(ev.weights) == len(ev.hist) + 1
            if ev.sample_out:
                saved = i
            assert (saved if ev.sample_in else i) == sp.src, (n, i)
            if sp.kind == "prk_last":
                assert ev.hist == ("acc",) and ev.weights == (1 / 6, 1.0) and not ev.acc_out and ev.hist_out is None
            else:
                assert (i,) + tuple(writer[s] for s in ev.hist) == sp.terms, (n, i)
                assert ev.weights == {"single": (1.0,), "redo": (0.5, 0.5), "plms2": (3 / 2, -1 / 2), "plms3": (23 / 12, -16 / 12, 5 / 12),
                                      "plms4": (55 / 24, -59 / 24, 37 / 24, -9 / 24)}[sp.kind]
            if mode == "prk" and i < 12:
                assert (ev.acc_in, ev.acc_out, ev.s_g) == [(False, True, 1 / 6), (True, True, 1 / 3), (True, True, 1 / 3), (False, False, 0.0)][i % 4]
                assert ev.sample_in == (i % 4 != 0) and ev.sample_out == (i % 4 == 0)
            else:
                assert not ev.acc_in and not ev.acc_out and ev.s_g == 0.0 and ev.sample_in == (i == 1 and mode == "plms") and ev.sample_out == (i == 0)
            if ev.hist_out is not None:
                assert ev.hist_out not in ev.hist
                writer[ev.hist_out] = i
        stored = [i for i, ev in enumerate(plan) if ev.hist_out is not None]
        assert stored == ([i for i in range(len(plan)) if i != 1] if mode == "plms" else [0, 4, 8] + list(range(12, len(plan))))
    tab = PNDMTables(config_of("linear", mode)).coefficient_table(10)
    assert tab.shape == (10 + (1 if mode == "plms" else 9), 6) and tab.dtype == torch.float32 and torch.isfinite(tab).all()
    # below timestep 0 the previous alpha is final_alpha_cumprod: alphas_cumprod[0], or 1 with set_alpha_to_one (epsilon prediction: c_x = sqrt(a_prev / a_t))
    for one in (False, True):
        tb = PNDMTables(config_of("linear", mode, set_alpha_to_one=one))
        last = tb.plan(10)[-1]
        a_t, a_0 = float(tb.alphas_cumprod[last.timestep]), float(tb.alphas_cumprod[0])
        assert last.prev_timestep < 0 and float(tb.final_alpha_cumprod) == (1.0 if one else a_0)
        assert abs(tb.step_coefficients(last)[0] - ((1.0 if one else a_0) / a_t) ** 0.5) < 1e-12


# ---- golden, drop-in and emulator against the specification ----------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("betas", list(SP.BETA_SETS))
def test_golden_dropin_and_emulator_inside_their_bounds(golden, dropin, betas):
    """Every evaluation of every case starts from the reference's own previous output (an evaluation that steps from the saved sample: from the reference's input of the
    evaluation that saved it).  The golden (the reference's f32 result) lies inside the K_REFERENCE bound of the specification; the drop-in's step() and the emulator's
    cfg_pndm_step, driven by the engine's plan and coefficient table, inside the K_KERNEL bound, gamma(19) S per element."""
    from diffusers import PNDMScheduler
    emu = PNDMEmuOps()
    B, C, F, h, w = (SP.LATENT_SHAPE[0], SP.LATENT_SHAPE[1], 1, *SP.LATENT_SHAPE[2:])
    worst = dict(golden=0.0, dropin=0.0, emu=0.0)
    cases = [c for c in SP.golden_cases() if c.betas == betas]
    assert len(cases) == 12
    for case in cases:
        tag = "/".join(map(str, case))
        prev = torch.from_numpy(golden[SP.case_key(case)])
        tb = PNDMTables(config_of(betas, case.mode, prediction_type=case.prediction_type))
        plan, coef, ts = tb.plan(case.n), tb.coefficient_table(case.n), tb.timesteps(case.n)
        xs, (_, vs) = SP.case_samples(case, prev), SP.case_inputs(case)
        sched = PNDMScheduler(**SP.BETA_SETS[betas], rescale_betas_zero_snr=betas == "zsnr", skip_prk_steps=case.mode == "plms", steps_offset=SP.STEPS_OFFSET,
                              prediction_type=case.prediction_type)
        sched.set_timesteps(case.n)
        assert torch.equal(sched.timesteps, ts) and sched.init_noise_sigma == 1.0 and torch.equal(sched.alphas_cumprod, tb.alphas_cumprod)
        buf = SP.Buffers(xs[0])
        spec = SP.schedule(case.mode, case.n, offset=SP.STEPS_OFFSET)
        assert len(spec) == len(prev) == len(plan) == SP.evaluations(case)
        for i, (ev, sp) in enumerate(zip(plan, spec)):
            ref, S = SP.schedule_eval(tb.alphas_cumprod, tb.final_alpha_cumprod, case.prediction_type, sp, xs, vs)
            b_ref, b_ker = SP.gamma(SP.K_REFERENCE) * S, SP.gamma(SP.K_KERNEL) * S
            worst["golden"] = max(worst["golden"], SP.inside(prev[i], ref, b_ref, f"golden {tag} evaluation {i}"))
            got = sched.step(vs[i], ts[i], xs[i]).prev_sample
            assert got.dtype == torch.float32 and sched.counter == i + 1
            worst["dropin"] = max(worst["dropin"], SP.inside(got, ref, b_ker, f"drop-in {tag} evaluation {i}"))
            lat = xs[i].clone()
            emu.cfg_pndm_step(channels_last(vs[i].reshape(B, C, F, h, w)), lat, coef[i], B=B, F=F, HW=h * w, c_latent=C, ld=C, cfg=False, guidance=1.0, **buf.kwargs(ev))
            worst["emu"] = max(worst["emu"], SP.inside(lat, ref, b_ker, f"emulator {tag} evaluation {i}"))
    print(f"{betas}: worst element / bound  golden {worst['golden']:.3f} (K = {SP.K_REFERENCE})  drop-in {worst['dropin']:.3f}  emulator {worst['emu']:.3f} (K = {SP.K_KERNEL})")


def test_refusals(dropin):
    from diffusers import PNDMScheduler
    # the Runge-Kutta mode with fewer than four steps (the reference dies in a numpy broadcast)
    for n in (1, 2, 3):
        with pytest.raises(ValueError, match="at least 4"):
            PNDMTables(PNDMConfig()).timesteps(n)
        with pytest.raises(ValueError, match="at least 4"):
            PNDMScheduler().set_timesteps(n)
        assert len(PNDMTables(PNDMConfig(skip_prk_steps=True)).timesteps(n)) == (n + 1 if n > 1 else 1)
    assert len(PNDMTables(PNDMConfig()).timesteps(4)) == 13
    # zero terminal SNR: a schedule that starts at timestep 999 divides by alphas_cumprod = 0
    zs = dict(SP.BETA_SETS["zsnr"], rescale_betas_zero_snr=True)
    for skip in (True, False):
        tb = PNDMTables(PNDMConfig(**zs, skip_prk_steps=skip, steps_offset=0))
        assert tb.alphas_cumprod[-1].item() == 0.0 and tb.timesteps(1000)[0].item() == 999
        with pytest.raises(ValueError, match="timestep 999"):
            tb.coefficient_table(1000)
        smp = object.__new__(PNDMSampler)                                       # the sampler refuses it before any launch
        smp.unet, smp.tables, smp.clip_sample = None, tb, False
        with pytest.raises(ValueError, match="timestep 999"):
            smp.prepare(torch.zeros(2, 77, 64), 1000, 1, 8.0)
        for n in (4, 10, 25):                                                    # leading spacing never starts there
            assert torch.isfinite(PNDMTables(PNDMConfig(**zs, skip_prk_steps=skip, steps_offset=1)).coefficient_table(n)).all()
    sched = PNDMScheduler(**zs, skip_prk_steps=True)
    sched.set_timesteps(1000)
    with pytest.raises(ValueError, match="timestep 999"):
        sched.step(torch.zeros(1, 4, 2, 2), sched.timesteps[0], torch.zeros(1, 4, 2, 2))
    with pytest.raises(ValueError, match="timestep 1000"):                       # a steps_offset that pushes the first step past the table
        PNDMTables(PNDMConfig(skip_prk_steps=True, steps_offset=1)).coefficient_table(1000)
    with pytest.raises(ValueError, match="prediction_type"):
        PNDMTables(PNDMConfig(prediction_type="sample"))
    with pytest.raises(ValueError, match="prediction_type"):
        PNDMScheduler(prediction_type="sample")
    with pytest.raises(NotImplementedError, match="squaredcos_cap_v2"):
        PNDMTables(PNDMConfig(beta_schedule="squaredcos_cap_v2"))
    with pytest.raises(NotImplementedError, match="squaredcos_cap_v2"):
        PNDMScheduler(beta_schedule="squaredcos_cap_v2")
    with pytest.raises(ValueError, match="num_inference_steps"):
        PNDMTables(PNDMConfig(skip_prk_steps=True)).timesteps(0)
    x = torch.randn(1, 4, 2, 2)
    for skip in (True, False):
        with pytest.raises(ValueError, match="set_timesteps"):
            PNDMScheduler(skip_prk_steps=skip).step(x, 999, x)
    s = PNDMScheduler()                                                          # PLMS before the Runge-Kutta phase has run
    s.set_timesteps(10)
    with pytest.raises(ValueError, match="AFTER scheduler has been run in 'prk' mode"):
        s.step_plms(x, s.timesteps[0], x)


# ---- the emulator on the kernel's cases --------------------------------------------------------------------------------------------------------------------
IDS = ["x".join(map(str, s)) for s in SP.SHAPES]


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape", SP.SHAPES, ids=IDS)
def test_emulator_on_the_kernel_cases(shape, dt):
    emu, nan = PNDMEmuOps(), torch.full((shape[0], shape[3], shape[1], shape[2]), float("nan"))
    o = SP.operands(shape, dt)
    for var in SP.VARIANTS:
        ref = SP.reference(shape, dt, var)
        got = SP.run_step(emu, shape, dt, var)
        for k, (val, bound) in ref.items():
            SP.inside(got[k], val, bound, f"emu {k} {shape} {dt} {var}")
        assert torch.equal(got["sample"], o["latents"].reshape(got["sample"].shape)) and (var.acc != "none" or bool(torch.isnan(got["acc"]).all()))
        if var.phi == 0.0 and not var.single:            # the buffers the variant does not read may hold anything; outputs not handed over stay as they were
            hs = [o[f"hist_{k}"] if var.order > k else nan for k in (1, 2, 3)]
            got2 = SP.run_step(emu, shape, dt, var, hist=hs, latents=nan if var.sample_in else None, store=False)          # (no sample_out: that would copy the latents)
            assert torch.equal(got2["lat"], got["lat"]) and bool(torch.isnan(got2["hist"]).all()) and bool(torch.isnan(got2["sample"]).all())
            assert var.acc == "none" or torch.equal(got2["acc"], got["acc"])
    assert len(SP.VARIANTS) == 128 and {v.order for v in SP.VARIANTS} == {1, 2, 3, 4}


# ---- the C surface, no device --------------------------------------------------------------------------------------------------------------------------------
def _lib():
    from followyourclick_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib, _lib.load()


FIELDS = ["pred", "latents", "coef", "B", "F", "HW", "c_latent", "ld", "cfg", "guidance", "dtype", "pred_single", "video_scale", "sample_in", "sample_out", "hist_out",
          "hist_1", "hist_2", "hist_3", "order", "acc_in", "acc_out", "guidance_rescale", "workspace", "workspace_bytes"]


def test_binding_and_python_surface(tmp_path):
    from followyourclick_amd import _lib as L, ops, profiling
    assert [n for n, _ in L.CfgPndmArgs._fields_] == FIELDS
    assert L.FYC_VERSION == 308 and L.OPS["fyc_cfg_pndm_step"] is L.CfgPndmArgs and "fyc_cfg_pndm_workspace_bytes" in L.MISC
    header = os.path.join(os.path.dirname(L.HERE), "include", "fyc.h")
    with open(header) as fh:
        head = fh.read()
    assert "#define FYC_VERSION 308" in head and "} fyc_cfg_pndm_args;" in head
    src = tmp_path / "abi.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{header}"\nint main(void){{'
                   'printf("%zu %zu %zu", sizeof(fyc_cfg_pndm_args), sizeof(fyc_cfg_sigma_args), sizeof(fyc_cfg_solver_args));'
                   + "".join(f'printf(" %zu", offsetof(fyc_cfg_pndm_args, {f}));' for f in FIELDS) + "return 0;}")
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    size, sigma, solver, *offs = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == ctypes.sizeof(L.CfgPndmArgs)
    assert sigma == ctypes.sizeof(L.CfgSigmaArgs) and solver == ctypes.sizeof(L.CfgSolverArgs)          # the existing structs are untouched
    assert offs == [getattr(L.CfgPndmArgs, f).offset for f in FIELDS]
    lib = _lib()[1]
    assert lib.fyc_version() == 308 and all(hasattr(lib, n) for n in ("fyc_cfg_pndm_step", "fyc_cfg_pndm_workspace_bytes"))
    sig = inspect.signature(ops.HipOps.cfg_pndm_step).parameters
    assert list(inspect.signature(PNDMEmuOps.cfg_pndm_step).parameters) == list(sig)
    assert not hasattr(EmuOps, "cfg_pndm_step") and not hasattr(SolverEmuOps, "cfg_pndm_step") and not hasattr(SigmaEmuOps, "cfg_pndm_step")
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("sample_in", "sample_out", "hist_out", "hist_1", "hist_2", "hist_3", "order", "acc_in", "acc_out",
                                                                      "guidance_rescale"))

    class Inner:          # the profiling wrapper forwards it
        name = "inner"

        def cfg_pndm_step(self, *a, **k):
            return ("pndm", a, k)
    timed = profiling.TimedOps(Inner())
    timed.enabled = False
    assert timed.cfg_pndm_step(1, order=2) == ("pndm", (1,), dict(order=2))


LAT_BYTES = 2 * 4 * 16 * 1031 * 4
PTR = dict(latents=0x20000000, sample_in=0x50000000, sample_out=0x60000000, hist_out=0x70000000, hist_1=0x80000000, hist_2=0x90000000, hist_3=0xA0000000,
           acc_in=0xB0000000, acc_out=0xC0000000)


def _args(L, fields, shape=(2, 16, 1031, 4, 16)):
    """fyc_cfg_pndm_args around a valid fourth-order problem with every optional buffer, with `fields` written over it"""
    a = L.CfgPndmArgs()
    a.pred, a.coef = 0x10000000, 0x30000000
    for k, v in PTR.items():
        setattr(a, k, v)
    a.B, a.F, a.HW, a.c_latent, a.ld = shape
    a.cfg, a.guidance, a.dtype, a.order = 1, 8.0, 1, 4
    a.guidance_rescale, a.workspace, a.workspace_bytes = 0.7, 0x40000000, 1 << 20
    for k, v in fields.items():
        setattr(a, k, v)
    return a


INPUTS = ("latents", "hist_1", "hist_2", "hist_3", "sample_in", "acc_in")
OUTS = ("sample_out", "hist_out", "acc_out")
BAD = ([(dict(pred=None), b"null"), (dict(latents=None), b"null"), (dict(coef=None), b"null"),
        (dict(B=0), b"dims"), (dict(ld=3), b"dims"), (dict(dtype=7), b"dtype"),
        (dict(order=0), b"order"), (dict(order=5), b"order"), (dict(order=2, hist_1=None), b"hist_1"), (dict(hist_1=None), b"hist_1"), (dict(hist_2=None), b"hist_2"),
        (dict(hist_3=None), b"hist_3"), (dict(order=3, hist_2=None), b"hist_2"),
        (dict(sample_in=PTR["latents"]), b"sample_in aliases latents"), (dict(sample_in=PTR["latents"] + LAT_BYTES - 4), b"sample_in aliases latents"),
        (dict(sample_in=PTR["latents"] - LAT_BYTES + 4), b"sample_in aliases latents")]
       # every output against every input (equal bases, and the last / first element overlapping) and against the other outputs; acc_out against acc_in only when they
       # overlap without being equal
       + [(dict([(o, PTR[i] + d)]), f"{o} aliases {i}".encode()) for o in OUTS for i in INPUTS for d in (0, LAT_BYTES - 4, 4 - LAT_BYTES) if not (o == "acc_out" and i == "acc_in" and d == 0)]
       + [(dict([(o, PTR[p] + d)]), f"{min(o, p, key=OUTS.index)} aliases {max(o, p, key=OUTS.index)}".encode()) for o in OUTS for p in OUTS if o != p for d in (0, LAT_BYTES - 4)]
       + [(dict(cfg=0, guidance_rescale=0.0, pred_single=0xD0000000), b"pred_single"),
          (dict(guidance_rescale=-0.1), b"guidance_rescale"), (dict(guidance_rescale=1.5), b"guidance_rescale"), (dict(guidance_rescale=float("nan")), b"guidance_rescale"),
          (dict(cfg=0), b"cfg"), (dict(workspace=None), b"workspace"), (dict(workspace_bytes=1095), b"workspace"), (dict(workspace=0x40000004), b"workspace"),
          (dict(F=1, HW=1, c_latent=1, ld=1), b"dims")])


@pytest.mark.parametrize("fields,word", BAD, ids=[",".join(f"{k}={v}" for k, v in b[0].items()) for b in BAD])
def test_bad_arguments_are_refused_by_the_library_without_gpu(fields, word):
    """refused before anything that needs a device or fyc_init (this process never calls fyc_init: a check behind it would report that instead)"""
    L, lib = _lib()
    assert lib.fyc_cfg_pndm_step(ctypes.byref(_args(L, fields)), None) != 0
    msg = lib.fyc_last_error()
    assert word in msg and b"fyc_cfg_pndm_step" in msg and b"fyc_init" not in msg, msg


def test_good_arguments_reach_the_init_check_and_the_query_launches_nothing():
    L, lib = _lib()
    none = dict(sample_in=None, sample_out=None, hist_out=None, acc_in=None, acc_out=None)
    for fields in (dict(), dict(order=1, hist_1=None, hist_2=None, hist_3=None), dict(none, order=1, hist_1=None, hist_2=None, hist_3=None), dict(order=3, hist_3=None),
                   dict(acc_out=PTR["acc_in"]),                                           # the one alias allowed
                   dict(hist_1=PTR["acc_in"], order=2), dict(hist_1=PTR["hist_2"]),       # inputs may alias each other
                   dict(dtype=0), dict(dtype=2, ld=5, c_latent=3), dict(guidance_rescale=0.0, workspace=None, cfg=0), dict(pred_single=0xD0000000, video_scale=0.3),
                   dict(hist_out=PTR["latents"] + LAT_BYTES), dict(sample_in=PTR["latents"] + LAT_BYTES), dict(none, acc_out=PTR["acc_out"])):
        assert lib.fyc_cfg_pndm_step(ctypes.byref(_args(L, fields)), None) != 0
        assert b"fyc_init" in lib.fyc_last_error(), (fields, lib.fyc_last_error())
    assert lib.fyc_cfg_pndm_step(None, None) != 0 and b"null" in lib.fyc_last_error()
    # the workspace is the DDIM rescale's: 2 samples x 17 runs of 1024 rows x 4 f64, then 2 f32 factors, in 256-byte units
    assert lib.fyc_cfg_pndm_workspace_bytes(ctypes.byref(_args(L, {}))) == 1280
    assert lib.fyc_cfg_pndm_workspace_bytes(ctypes.byref(_args(L, dict(guidance_rescale=0.0)))) == 0
    assert lib.fyc_cfg_pndm_workspace_bytes(ctypes.byref(_args(L, dict(B=0)))) == 0
    assert lib.fyc_cfg_pndm_workspace_bytes(None) == 0


# ---- front ends ------------------------------------------------------------------------------------------------------------------------------------------------
YAML = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", prediction_type="v_prediction")
ZERO_SNR = dict(YAML, rescale_betas_zero_snr=True)
# scheduler/scheduler_config.json of the Stable Diffusion 1.5 checkpoint
SD15 = {"_class_name": "PNDMScheduler", "_diffusers_version": "0.6.0", "beta_end": 0.012, "beta_schedule": "scaled_linear", "beta_start": 0.00085,
        "num_train_timesteps": 1000, "set_alpha_to_one": False, "skip_prk_steps": True, "steps_offset": 1, "trained_betas": None, "clip_sample": False}


def test_dropin_scheduler_surface(dropin, tmp_path):
    import diffusers
    from diffusers import PNDMScheduler, schedulers
    from diffusers.schedulers.scheduling_pndm import PNDMScheduler as direct
    assert "fyc" in diffusers.__version__ and schedulers.PNDMScheduler is PNDMScheduler is direct
    s = PNDMScheduler()
    assert (s.config.num_train_timesteps, s.config.beta_start, s.config.beta_end, s.config.beta_schedule, s.config.trained_betas, s.config.skip_prk_steps,
            s.config.set_alpha_to_one, s.config.prediction_type, s.config.steps_offset, s.config.rescale_betas_zero_snr) == (1000, 0.0001, 0.02, "linear", None, False,
                                                                                                                           False, "epsilon", 0, False)
    assert s.order == 1 and len(s) == 1000 and isinstance(s.engine_config, PNDMConfig) and s.init_noise_sigma == 1.0 and s.pndm_order == 4
    assert s.timesteps is None and s.prk_timesteps is None and s.plms_timesteps is None and s.counter == 0 and s.ets == [] and s.cur_sample is None
    assert s.final_alpha_cumprod.item() == s.alphas_cumprod[0].item() and PNDMScheduler(set_alpha_to_one=True).final_alpha_cumprod.item() == 1.0
    # foreign keys (thresholding, a DDIM's clip_sample, a solver's order) are dropped; the SD-1.5 file loads
    kept = PNDMScheduler.from_config(dict(ZERO_SNR, skip_prk_steps=True, steps_offset=1, clip_sample=False, solver_order=3, thresholding=True, timestep_spacing="leading"))
    assert kept.engine_config.rescale_betas_zero_snr and kept.config.skip_prk_steps and not hasattr(kept.config, "thresholding")
    (tmp_path / "sd15" / "scheduler").mkdir(parents=True)
    (tmp_path / "sd15" / "scheduler" / "scheduler_config.json").write_text(json.dumps(SD15))
    sd = PNDMScheduler.from_pretrained(str(tmp_path / "sd15"), subfolder="scheduler")
    assert (sd.config.beta_schedule, sd.config.skip_prk_steps, sd.config.steps_offset, sd.config.prediction_type) == ("scaled_linear", True, 1, "epsilon")
    assert PNDMScheduler.from_pretrained(str(tmp_path / "sd15"), subfolder="scheduler", prediction_type="v_prediction").config.prediction_type == "v_prediction"
    with pytest.raises(EnvironmentError):
        PNDMScheduler.from_pretrained(str(tmp_path / "absent"))
    sd.set_timesteps(50)
    assert sd.timesteps.dtype == torch.int64 and len(sd.timesteps) == 51 and sd.timesteps[:4].tolist() == [981, 961, 961, 941] and len(sd.prk_timesteps) == 0
    assert np.array_equal(sd.plms_timesteps, sd.timesteps.numpy())
    x = torch.randn(1, 4, 2, 2)
    assert sd.scale_model_input(x, sd.timesteps[0]) is x
    abar = sd.alphas_cumprod[sd.timesteps[2:3]]
    assert torch.equal(sd.add_noise(x, torch.ones_like(x), sd.timesteps[2:3]), abar ** 0.5 * x + (1 - abar) ** 0.5 * torch.ones_like(x))
    for skip in (True, False):
        s = PNDMScheduler(skip_prk_steps=skip, **YAML)
        v = torch.randn(14, 1, 4, 2, 2)

        def run():          # the state: set_timesteps resets it, two runs give the same bits
            s.set_timesteps(5)
            y = x
            for i, tt in enumerate(s.timesteps):
                y = s.step(v[i], tt, y).prev_sample
            return y
        y1, y2 = run(), run()
        assert torch.equal(y1, y2) and torch.isfinite(y1).all() and s.counter == (6 if skip else 14) and len(s.ets) == 4
        assert len(s.prk_timesteps) == (0 if skip else 12) and len(s.plms_timesteps) == (6 if skip else 2)
        s.set_timesteps(5)
        assert s.counter == 0 and s.ets == []
        out = s.step(v[0], s.timesteps[0], x, return_dict=False)
        assert isinstance(out, tuple) and out[0].shape == x.shape


MM = dict(num_attention_heads=8, num_transformer_block=1, attention_block_types=["Temporal_Self", "Temporal_Self"],
          temporal_position_encoding=True, temporal_position_encoding_max_len=24, temporal_attention_dim_div=1, zero_initialize=True)
TINY = dict(sample_size=8, in_channels=4, out_channels=4, block_out_channels=(64, 128, 256, 256), layers_per_block=2,
            cross_attention_dim=64, attention_head_dim=8, use_motion_module=True, motion_module_resolutions=(1, 2, 4, 8),
            unet_use_cross_frame_attention=False, unet_use_temporal_attention=False, use_fps_condition=True,
            use_first_frame_mask_condition_concat=True, motion_module_type="Vanilla", motion_module_kwargs=MM)
POINTERS = ("sample_in", "sample_out", "hist_out", "hist_1", "hist_2", "hist_3", "acc_in", "acc_out")


class Recording:
    """records the launches of an ops object by name (and what a step carries), forwarding everything"""

    def __init__(self, inner):
        self.inner, self.names, self.steps = inner, [], []

    def __getattr__(self, name):
        v = getattr(self.inner, name)
        if not callable(v) or name == "ensure_init":
            return v

        def call(*a, **kw):
            self.names.append(name)
            if name.startswith("cfg_"):
                self.steps.append(dict(name=name, order=kw.get("order"), guidance_rescale=kw.get("guidance_rescale"), latents=a[1].data_ptr(),
                                       **{k: None if kw.get(k) is None else kw[k].data_ptr() for k in POINTERS}))
            return v(*a, **kw)
        return call


def check_pointers(steps, mode, n):
    """which optional pointers every evaluation hands over: the census of a schedule of n steps"""
    assert len(steps) == n + (1 if mode == "plms" else 9) and all(s["name"] == "cfg_pndm_step" for s in steps)
    sample = steps[0]["sample_out"]
    hists = {s["hist_out"] for s in steps} - {None}
    stores = sum(s["hist_out"] is not None for s in steps)
    assert stores == (len(steps) - 1 if mode == "plms" else len(steps) - 9) and len(hists) == min(4, stores)          # four history buffers, their roles rotating
    assert sample is not None and sample not in hists
    prk = 0 if mode == "plms" else 12
    for i, s in enumerate(steps):
        used = {k for k in POINTERS if s[k] is not None}
        if i < prk:
            r = i % 4
            want = [{"sample_out", "hist_out", "acc_out"}, {"sample_in", "acc_in", "acc_out"}, {"sample_in", "acc_in", "acc_out"}, {"sample_in", "hist_1"}][r]
            assert used == want and s["order"] == (2 if r == 3 else 1), (i, used)
            assert r == 0 or s["sample_in"] == sample
            if r in (1, 2):
                assert s["acc_in"] == s["acc_out"] == steps[i - r]["acc_out"]                 # in place
            if r == 3:
                assert s["hist_1"] == steps[i - 1]["acc_out"] and s["hist_1"] not in hists      # the accumulator is the second term
        elif mode == "plms" and i == 0:
            assert used == {"sample_out", "hist_out"} and s["order"] == 1
        elif mode == "plms" and i == 1:
            assert used == {"sample_in", "hist_1"} and s["order"] == 2 and s["sample_in"] == sample and s["hist_1"] == steps[0]["hist_out"]
        else:
            stored = [t["hist_out"] for t in steps[:i] if t["hist_out"] is not None]
            order = min(4, len(stored) + 1)
            assert used == {"hist_out"} | {f"hist_{k}" for k in range(1, order)} and s["order"] == order, (i, used)
            assert [s[f"hist_{k}"] for k in range(1, order)] == stored[::-1][:order - 1] and s["hist_out"] not in stored[::-1][:order - 1]
        assert all(s[k] != s["latents"] for k in POINTERS)


def test_pipeline_routes_by_the_scheduler(dropin, monkeypatch):
    from animatediff.models.unet import UNet3DConditionModel
    from animatediff.pipelines.pipeline_animation import AnimationPipeline
    from diffusers import AutoencoderKL, DDIMScheduler, DPMSolverMultistepScheduler, PNDMScheduler
    from followyourclick_amd import ops as ops_mod
    from oracle import stubs
    assert type(make_sampler(None, DDIMConfig())) is DDIMSampler and type(make_sampler(None, SolverConfig())) is SolverSampler
    assert type(make_sampler(None, SigmaConfig())) is SigmaSampler and type(make_sampler(None, PNDMConfig())) is PNDMSampler
    with pytest.raises(TypeError, match="PNDMConfig"):
        make_sampler(None, object())
    monkeypatch.delenv("FYC_GUIDANCE_RESCALE", raising=False)
    monkeypatch.setattr(AnimationPipeline, "decode_latents", lambda self, latents: np.zeros((1, 3, 2, 64, 64), np.float32))      # routing only: no VAE run
    vae = AutoencoderKL(block_out_channels=(64, 128, 128, 128), layers_per_block=2, latent_channels=4)
    bars = []

    class Bar:
        def __init__(self, total):
            self.total, self.n = total, 0
            bars.append(self)

        def update(self):
            self.n += 1

    def run(scheduler, ops, steps=4, **kw):
        pipe = AnimationPipeline(vae=vae, text_encoder=stubs.StubTextEncoder(64), tokenizer=stubs.FakeTokenizer(), unet=UNet3DConditionModel(**TINY), scheduler=scheduler)
        monkeypatch.setattr(pipe, "progress_bar", lambda iterable=None, total=None: Bar(total), raising=False)
        rec = Recording(ops)
        monkeypatch.setattr(ops_mod, "impl", rec)
        pipe("a corgi", video_length=2, height=64, width=64, num_inference_steps=steps, guidance_scale=8.0, use_first_frame_mask_condition_concat=True,
             first_image_latents=torch.zeros(1, 4, 8, 8), generator=torch.Generator().manual_seed(0), **kw)
        return rec

    # the other schedulers: the launches are the ones they were (their emulators lack the new op: nobody asks for it)
    ddim = run(DDIMScheduler(steps_offset=1, clip_sample=False, **ZERO_SNR), EmuOps())
    assert [s["name"] for s in ddim.steps] == ["cfg_ddim_step"] * 4 and (bars[-1].total, bars[-1].n) == (4, 4)
    sol = run(DPMSolverMultistepScheduler(**ZERO_SNR), SolverEmuOps())
    assert [s["name"] for s in sol.steps] == ["cfg_solver_step"] * 4
    assert [n for n in sol.names if not n.startswith("cfg_")] == [n for n in ddim.names if not n.startswith("cfg_")]

    def evaluations(names):
        """the launches from one input build to the next"""
        at = [i for i, n in enumerate(names) if n == "unet_input"]
        return [names[a:b] for a, b in zip(at, at[1:] + [len(names)])]
    per_step = evaluations(ddim.names)
    assert len(per_step) == 4 and all(e == per_step[0] for e in per_step) and per_step[0][-1] == "cfg_ddim_step"
    for mode, evals in (("plms", 5), ("prk", 13)):
        called = []
        sched = PNDMScheduler(skip_prk_steps=mode == "plms", **ZERO_SNR)                 # steps_offset 0: both pipelines patch it to 1, as the reference's do
        rec = run(sched, PNDMEmuOps(), eta=0.5, callback=lambda i, t, lat: called.append((i, int(t))))      # eta is accepted and unused, as in the reference
        assert sched.config.steps_offset == 1 and sched.engine_config.steps_offset == 1 and sched.timesteps[-1].item() == 1
        check_pointers(rec.steps, mode, 4)
        assert [s["guidance_rescale"] for s in rec.steps] == [0.0] * evals
        # one input build, one forward and one step per evaluation: the launches of a DDIM step with the update kernel replaced, once per entry of the timestep list
        assert evaluations(rec.names) == [per_step[0][:-1] + ["cfg_pndm_step"]] * evals
        # the progress count follows the timestep list; the caller's callback is held back over the warm-up evaluations as the reference holds it
        assert (bars[-1].total, bars[-1].n) == (evals, evals)
        assert called == [(i, int(sched.timesteps[i])) for i in range(evals - 4, evals)]
    with pytest.raises(ValueError, match="at least 4"):
        run(PNDMScheduler(**ZERO_SNR), PNDMEmuOps(), steps=3)


def test_sd_pipeline_with_the_checkpoints_own_scheduler_config(dropin, monkeypatch):
    """the 2-D first-image path with scheduler/scheduler_config.json of Stable Diffusion 1.5: PLMS, n + 1 evaluations"""
    from diffusers import AutoencoderKL, PNDMScheduler, StableDiffusionPipeline, UNet2DConditionModel
    from followyourclick_amd import ops as ops_mod
    from oracle import stubs
    monkeypatch.setattr(StableDiffusionPipeline, "decode_latents", lambda self, latents: np.zeros((1, 64, 64, 3), np.float32))      # routing only: no VAE run
    vae = AutoencoderKL(block_out_channels=(64, 128, 128, 128))
    unet = dict(sample_size=8, block_out_channels=(64, 128, 256, 256), cross_attention_dim=64)
    for cfg, mode in ((SD15, "plms"), (dict(SD15, skip_prk_steps=False), "prk")):
        rec, called = Recording(PNDMEmuOps()), []
        monkeypatch.setattr(ops_mod, "impl", rec)
        pipe = StableDiffusionPipeline(vae, stubs.StubTextEncoder(64), stubs.FakeTokenizer(), UNet2DConditionModel(**unet), PNDMScheduler.from_config(cfg), safety_checker=None)
        pipe("a corgi", height=64, width=64, num_inference_steps=4, guidance_scale=8.0, generator=torch.Generator().manual_seed(0), output_type="np",
             callback=lambda i, t, lat: called.append(i))
        check_pointers(rec.steps, mode, 4)
        assert called == list(range(len(rec.steps) - 4, len(rec.steps)))
    with pytest.raises(TypeError, match="PNDMScheduler"):
        StableDiffusionPipeline(vae, stubs.StubTextEncoder(64), stubs.FakeTokenizer(), UNet2DConditionModel(**unet), type("Foreign", (), dict(config=type("C", (), {})()))(),
                                safety_checker=None)("a corgi", height=64, width=64, num_inference_steps=2)


# ---- the sampler on the emulator ---------------------------------------------------------------------------------------------------------------------------
def tiny_cfg(**kw):
    return UNet3DConfig(block_out_channels=(64, 128, 256, 256), cross_attention_dim=64, sample_size=8, **kw)


@pytest.mark.parametrize("mode", SP.MODES)
def test_sampler_launch_census(mode):
    """PNDMSampler on the emulator: one unet_input and one cfg_pndm_step per evaluation, n + 1 / n + 9 evaluations, time embeddings and callbacks by the timestep list;
    use_graph, eta, generator and use_clipped_model_output are accepted and unused"""
    sd = W.make_weights(W.unet_state_shapes(Fn.tiny_unet_config()), 0)
    inp = W.seeded_inputs(Fn.tiny_unet_config(), 1, 4, 8, 8, seed=7)
    rec = Recording(PNDMEmuOps())
    smp = PNDMSampler(UNet3DEngine(pack_unet(sd, tiny_cfg(), torch.float32, "cpu"), ops=rec), PNDMConfig(skip_prk_steps=mode == "plms", steps_offset=1, **ZERO_SNR))
    seen = []
    out = smp.sample(inp["latents"], inp["text"], 5, 8.0, inp["first_image_latents"], inp["first_images_mask"], fps=[2], flow=[4],
                     callback=lambda i, t, l: seen.append((i, t)), use_graph=True, eta=0.3, generator=torch.Generator().manual_seed(5), use_clipped_model_output=True,
                     guidance_rescale=0.7)
    ts = smp.tables.timesteps(5).tolist()
    assert seen == list(enumerate(ts)) and len(ts) == (6 if mode == "plms" else 14) and torch.isfinite(out).all()
    assert rec.names.count("unet_input") == rec.names.count("cfg_pndm_step") == len(ts) and [s["guidance_rescale"] for s in rec.steps] == [0.7] * len(ts)
    check_pointers(rec.steps, mode, 5)
    st = smp.prepare(inp["text"], 5, 1, 8.0, [2], [4])
    assert st["temb"].shape[0] == st["coef"].shape[0] == len(st["plan"]) == len(ts) and st["coef"].shape[1] == 6 and st["steps"] == 5


def run_tiny_pipeline(g, mode, dtype, ops, device="cpu"):
    """the reference pipeline's run of tests/golden/pipeline_tiny_pndm.npz on an engine -> per-evaluation relative L2 against its trajectory"""
    sd = W.make_weights(W.unet_state_shapes(Fn.tiny_unet_config()), int(g["unet_weight_seed"]))
    eng = UNet3DEngine(pack_unet(sd, tiny_cfg(), dtype, device), ops=ops)
    traj, seen = [], []
    lat = PNDMSampler(eng, PNDMConfig(skip_prk_steps=mode == "plms", steps_offset=1, **YAML)).sample(
        g["latents"], g["text_embeddings"], 5, 8.0, g["first_image_latents"], g["first_images_mask"], fps=[2], flow=[4],
        callback=lambda i, t, l: (traj.append(l.detach().cpu().clone()), seen.append(t)))
    assert lat.dtype == torch.float32 and seen == g[f"timesteps_{mode}"].tolist()
    ref = g[f"trajectory_{mode}"]
    return (torch.stack(traj) - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)


@pytest.mark.parametrize("mode", SP.MODES)
def test_sampler_trajectory_matches_reference_pipeline(pipe_golden, mode):
    """5 steps (6 / 14 evaluations) of the real AnimationPipeline with the reference's PNDMScheduler, CFG 8, mask + first-frame concat, fps / flow conditioning, on the
    emulator in f32: per-evaluation rel-L2 < 5e-4, the bound of the DDIM and sigma runs of the same model"""
    err = run_tiny_pipeline(pipe_golden, mode, torch.float32, PNDMEmuOps())
    print(f"{mode} f32 pipeline trajectory on the emulator: per-evaluation rel-L2 {[f'{e:.2e}' for e in err.tolist()]}")
    assert err.max().item() < 5e-4, err


@pytest.mark.parametrize("mode", SP.MODES)
def test_dropin_pipeline_trajectory_matches_reference_pipeline(pipe_golden, dropin, monkeypatch, mode):
    """the same run through the drop-in AnimationPipeline with the drop-in PNDMScheduler: the latents of the evaluations the reference's callback is called for (the
    others are held back as there) against the golden trajectory under the same bound"""
    from animatediff.models.unet import UNet3DConditionModel
    from animatediff.pipelines.pipeline_animation import AnimationPipeline
    from diffusers import AutoencoderKL, PNDMScheduler
    from followyourclick_amd import ops as ops_mod
    from oracle import stubs
    g = pipe_golden
    monkeypatch.delenv("FYC_GUIDANCE_RESCALE", raising=False)
    monkeypatch.setattr(AnimationPipeline, "decode_latents", lambda self, latents: np.zeros((1, 3, 4, 64, 64), np.float32))
    monkeypatch.setattr(ops_mod, "impl", PNDMEmuOps())
    unet = UNet3DConditionModel(**TINY, compute_dtype=torch.float32)
    assert not any(unet.load_state_dict(W.make_weights(W.unet_state_shapes(Fn.tiny_unet_config()), int(g["unet_weight_seed"])), strict=False))
    pipe = AnimationPipeline(vae=AutoencoderKL(block_out_channels=(64, 128, 128, 128), layers_per_block=2, latent_channels=4), text_encoder=stubs.StubTextEncoder(64),
                             tokenizer=stubs.FakeTokenizer(), unet=unet, scheduler=PNDMScheduler(skip_prk_steps=mode == "plms", **YAML))
    got = {}
    pipe("a corgi waving its tail", video_length=4, height=64, width=64, num_inference_steps=5, guidance_scale=8.0, negative_prompt="blurry",
         latents=g["latents"].clone(), first_image_latents=g["first_image_latents"], first_images_mask=g["first_images_mask"],
         use_first_frame_mask_condition_concat=True, use_fps_condition=True, fps_tensor=torch.tensor([2]), flow_control=torch.tensor([4]),
         callback=lambda i, t, l: got.__setitem__(i, l.detach().cpu().clone()), callback_steps=1)
    assert sorted(got) == g[f"callback_indices_{mode}"].tolist()
    ref = g[f"trajectory_{mode}"]
    err = [((got[i] - ref[i]).norm() / ref[i].norm()).item() for i in sorted(got)]
    print(f"{mode} f32 drop-in pipeline on the emulator: rel-L2 at the callbacks {[f'{e:.2e}' for e in err]}")
    assert max(err) < 5e-4, err
