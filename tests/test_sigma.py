"""The sigma-space samplers - Euler, Euler ancestral, LMS - without a GPU: SigmaTables against the golden vectors of the reference's own classes
(tests/golden/sigma_samplers.npz, written by tools/make_golden_sigma.py), the golden, the drop-in's step() and the emulator (tests/emu_ops_sigma.py) against the
f64 specification (tests/sigma_spec.py) inside the bounds derived there, the zero-terminal-SNR table, the C surface of fyc_cfg_sigma_step and fyc_unet_input_scaled
(layout, refusals), the routing through the two pipelines, the sampler on the emulator against a hand loop and the reference pipeline's trajectories."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sigma_spec as SP
from emu_ops import EmuOps
from emu_ops_sigma import SigmaEmuOps
from emu_ops_solver import SolverEmuOps
from followyourclick_amd.engine import DDIMConfig, SigmaConfig, SolverConfig, UNet3DConfig
from followyourclick_amd.engine.sampler import DDIMSampler, SigmaSampler, SolverSampler, make_sampler
from followyourclick_amd.engine.scheduler import SigmaTables
from followyourclick_amd.engine.unet3d import UNet3DEngine
from followyourclick_amd.engine.weights import pack_unet
from oracle import functional as Fn
from oracle import weights as W


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "sigma_samplers.npz"))


@pytest.fixture(scope="module")
def pipe_golden(golden_dir):
    return {k: torch.from_numpy(v) if v.shape else v for k, v in np.load(os.path.join(golden_dir, "pipeline_tiny_sigma.npz")).items()}


def config_of(betas, kind, **kw):
    return SigmaConfig(kind=kind, **SP.BETA_SETS[betas], rescale_betas_zero_snr=betas == "zsnr", **kw)


# ---- tables, timesteps, LMS coefficients ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("betas", list(SP.BETA_SETS))
def test_tables_and_timesteps_are_the_reference_bits(golden, betas):
    for kind in SP.KINDS:
        tb = SigmaTables(config_of(betas, kind))
        assert np.float32(tb.init_noise_sigma) == golden[f"{betas}/{kind}/init_noise_sigma"] and np.isfinite(tb.init_noise_sigma)
        for n in SP.STEP_COUNTS:
            sg, ts = tb.sigmas(n), tb.timesteps(n)
            assert sg.dtype == torch.float32 and ts.dtype == torch.float64
            assert np.array_equal(sg.numpy(), golden[f"{betas}/{kind}/sigmas_n{n}"]) and np.array_equal(ts.numpy(), golden[f"{betas}/{kind}/timesteps_n{n}"])
            assert np.array_equal(SP.timesteps(n), ts.numpy()) and sg[-1].item() == 0.0
            den = tb.input_denominators(n)
            assert len(den) == n and all(d == float((s ** 2 + 1) ** 0.5) for d, s in zip(den, sg[:-1]))
    assert SigmaTables(config_of("linear", "euler")).timesteps(25)[1].item() == 957.375          # fractional: the UNet's embedding gets them as they are
    assert (abs(SigmaTables(config_of("zsnr", "euler")).init_noise_sigma - 4096.0) < 1e-3)


@pytest.mark.parametrize("betas", list(SP.BETA_SETS))
def test_lms_coefficients_against_the_reference_quadrature(golden, betas):
    """closed form in f64 against what the reference's scipy quadrature of its f32 integrand returned: within 12 x 2^-24 x max_k |c_k| of the step (the integrand's
    roundings, four per factor and three factors; sigma_spec.LMS_COEF_UNITS)"""
    tb, worst = SigmaTables(config_of(betas, "lms")), 0.0
    for n in SP.STEP_COUNTS:
        sg, ref = tb.sigmas(n), golden[f"{betas}/lms_coeffs_n{n}"]
        tab = tb.coefficient_table(n)
        for i in range(n):
            o = min(i + 1, 4)
            mine = tb.lms_coefficients(sg, i, o)
            scale = 2.0 ** -24 * np.abs(ref[i]).max()
            units = max(abs(a - b) for a, b in zip(mine, ref[i, :o])) / scale
            worst = max(worst, units)
            assert units <= SP.LMS_COEF_UNITS, (betas, n, i, units)
            assert not ref[i, o:].any() and tab[i, 3 + o:7].tolist() == [0.0] * (4 - o) and tab[i, 7].item() == 0.0
            assert tab[i, 3:3 + o].tolist() == torch.tensor(mine, dtype=torch.float64).float().tolist()
        assert abs(tab[0, 3].item() - float(sg[1] - sg[0])) <= 2.0 ** -23 * abs(float(sg[0]))          # first order: the Euler step
    print(f"{betas}: closed-form LMS coefficients at most {worst:.2f} x 2^-24 max|c_k| from the reference's quadrature (bound {SP.LMS_COEF_UNITS})")


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


def dropin_classes():
    from diffusers import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler, LMSDiscreteScheduler
    return {"euler": EulerDiscreteScheduler, "euler_ancestral": EulerAncestralDiscreteScheduler, "lms": LMSDiscreteScheduler}


@pytest.mark.parametrize("betas", list(SP.BETA_SETS))
def test_golden_dropin_and_emulator_inside_their_bounds(golden, dropin, betas, monkeypatch):
    """Every step of every case starts from the reference's own previous output.  The golden (the reference's f32 result) lies inside the K_REFERENCE bound of the
    specification; the drop-in's step() and the emulator's cfg_sigma_step inside the K_KERNEL bound, gamma(19) S per element."""
    emu, classes = SigmaEmuOps(), dropin_classes()
    B, C, F, h, w = (SP.LATENT_SHAPE[0], SP.LATENT_SHAPE[1], 1, *SP.LATENT_SHAPE[2:])
    worst = dict(golden=0.0, dropin=0.0, emu=0.0)
    cases = [c for c in SP.golden_cases() if c.betas == betas]
    assert len(cases) == 18
    randn = torch.randn
    for case in cases:
        tag = "/".join(map(str, case))
        prev = torch.from_numpy(golden[SP.case_key(case)])
        tb = SigmaTables(config_of(betas, case.kind, prediction_type=case.prediction_type))
        sig, ts, coef = tb.sigmas(case.n), tb.timesteps(case.n), tb.coefficient_table(case.n)
        xs, (_, vs, noise) = SP.case_samples(case, prev, tb.init_noise_sigma), SP.case_inputs(case)
        sched = classes[case.kind](**SP.BETA_SETS[betas], rescale_betas_zero_snr=betas == "zsnr", prediction_type=case.prediction_type)
        sched.set_timesteps(case.n)
        assert torch.equal(sched.sigmas, sig) and torch.equal(sched.timesteps, ts) and sched.init_noise_sigma.item() == tb.init_noise_sigma
        hist = [torch.full(SP.LATENT_SHAPE, float("nan")) for _ in range(4)]
        lms_ref = golden[f"{betas}/lms_coeffs_n{case.n}"] if case.kind == "lms" else None
        for i, t in enumerate(ts):
            order = tb.order(i)
            ref, S = SP.schedule_step(case.kind, case.prediction_type, sig, i, xs, vs, noise=noise[i], lms_coeffs=None if lms_ref is None else lms_ref[i, :order])
            b_ref, b_ker = SP.gamma(SP.K_REFERENCE) * S, SP.gamma(SP.K_KERNEL) * S
            worst["golden"] = max(worst["golden"], SP.inside(prev[i], ref, b_ref, f"golden {tag} step {i}"))
            if case.kind == "lms" and i > 0:          # the drop-in's history is its own: hand it the derivative of the reference's previous sample
                sched.derivatives[-1] = SP.derivative(case.prediction_type, sig[i - 1], xs[i - 1], vs[i - 1]).v.float()
                for k in range(2, min(len(sched.derivatives), order) + 1):
                    sched.derivatives[-k] = SP.derivative(case.prediction_type, sig[i - k], xs[i - k], vs[i - k]).v.float()
            monkeypatch.setattr(torch, "randn", lambda *a, _i=i, **k: noise[_i].clone())
            got = sched.step(vs[i], t, xs[i]).prev_sample
            monkeypatch.setattr(torch, "randn", randn)
            assert got.dtype == torch.float32
            worst["dropin"] = max(worst["dropin"], SP.inside(got, ref, b_ker, f"drop-in {tag} step {i}"))
            lat = xs[i].clone()
            hk = {}
            if case.kind == "lms":
                for k in range(1, order):           # the derivatives of the reference's own earlier samples, rounded once to f32 as a stored history is
                    hist[(i - k) % 4] = SP.derivative(case.prediction_type, sig[i - k], xs[i - k], vs[i - k]).v.float()
                hk = dict(hist_out=hist[i % 4], hist_1=hist[(i - 1) % 4], hist_2=hist[(i - 2) % 4], hist_3=hist[(i - 3) % 4], order=order)
            emu.cfg_sigma_step(channels_last(vs[i].reshape(B, C, F, h, w)), lat, coef[i], noise=noise[i] if case.kind == "euler_ancestral" else None,
                               B=B, F=F, HW=h * w, c_latent=C, ld=C, cfg=False, guidance=1.0, **hk)
            worst["emu"] = max(worst["emu"], SP.inside(lat, ref, b_ker, f"emulator {tag} step {i}"))
    print(f"{betas}: worst element / bound  golden {worst['golden']:.3f} (K = {SP.K_REFERENCE})  drop-in {worst['dropin']:.3f}  emulator {worst['emu']:.3f} (K = {SP.K_KERNEL})")


def test_zero_snr_first_step_and_refusals(dropin):
    """with the switch the table ends at alphas_cumprod = 2^-24 (sigma_max ~ 4096) and every coefficient is finite; without it a table that reaches 0 is refused at
    set_timesteps with the timestep and the switch named"""
    classes = dropin_classes()
    b = SP.BETA_SETS["zsnr"]
    for kind in SP.KINDS:
        for pred in SP.PREDICTIONS:
            tb = SigmaTables(config_of("zsnr", kind, prediction_type=pred))
            assert tb.alphas_cumprod[-1].item() == 2.0 ** -24
            for n in (4, 25):
                coef, den = tb.coefficient_table(n), tb.input_denominators(n)
                assert torch.isfinite(coef).all() and np.isfinite(den).all() and abs(den[0] - 4096.0) < 1e-2
            sched = classes[kind](**b, rescale_betas_zero_snr=True, prediction_type=pred)
            sched.set_timesteps(4)
            x = torch.randn(1, 4, 2, 2) * sched.init_noise_sigma
            y = sched.step(torch.randn(1, 4, 2, 2), sched.timesteps[0], sched.scale_model_input(x, sched.timesteps[0])).prev_sample
            assert torch.isfinite(y).all()
        # the rescaled betas handed over as trained_betas, the switch off: the table reaches alphas_cumprod = 0
        rescaled = SigmaTables(SigmaConfig(kind=kind, trained_betas=SigmaTables(config_of("zsnr", kind)).betas.tolist()))
        assert rescaled.alphas_cumprod[-1].item() == 0.0
        for call in (lambda: rescaled.sigmas(10), lambda: rescaled.coefficient_table(10)):
            with pytest.raises(ValueError, match="timestep 999.*rescale_betas_zero_snr"):
                call()
        sched = classes[kind](trained_betas=rescaled.betas.tolist())
        with pytest.raises(ValueError, match="timestep 999.*rescale_betas_zero_snr"):
            sched.set_timesteps(10)
        smp = object.__new__(SigmaSampler)                                       # the sampler refuses it before any launch
        smp.unet, smp.tables, smp.clip_sample, smp.kind = None, rescaled, False, kind
        with pytest.raises(ValueError, match="timestep 999"):
            smp.prepare(torch.zeros(2, 77, 64), 10, 1, 8.0)


def test_unsupported_options_are_refused(dropin):
    classes = dropin_classes()
    for kind, cls in classes.items():
        with pytest.raises(ValueError, match="prediction_type"):
            SigmaTables(SigmaConfig(kind=kind, prediction_type="sample"))
        with pytest.raises(ValueError, match="prediction_type"):
            cls(prediction_type="sample")
        with pytest.raises(NotImplementedError, match="squaredcos_cap_v2"):
            SigmaTables(SigmaConfig(kind=kind, beta_schedule="squaredcos_cap_v2"))
        with pytest.raises(NotImplementedError, match="squaredcos_cap_v2"):
            cls(beta_schedule="squaredcos_cap_v2")
        s = cls()
        x = torch.randn(1, 4, 2, 2)
        with pytest.raises(ValueError, match="set_timesteps"):
            s.step(x, 999.0, x)
        s.set_timesteps(5)
        for bad in (3, torch.tensor(3), torch.tensor(3, dtype=torch.int32)):          # integer indices, as the reference refuses them
            with pytest.raises(ValueError, match="integer indices"):
                s.step(x, bad, x)
    with pytest.raises(ValueError, match="kind"):
        SigmaTables(SigmaConfig(kind="heun"))
    lms = classes["lms"]()
    lms.set_timesteps(5)
    with pytest.raises(ValueError, match="order"):
        lms.step(torch.zeros(1), lms.timesteps[0], torch.zeros(1), order=5)


# ---- the emulator on the kernel's cases --------------------------------------------------------------------------------------------------------------------
IDS = ["x".join(map(str, s)) for s in SP.SHAPES]


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape", SP.SHAPES, ids=IDS)
def test_emulator_on_the_kernel_cases(shape, dt):
    emu, nan = SigmaEmuOps(), torch.full((shape[0], shape[3], shape[1], shape[2]), float("nan"))
    o = SP.operands(shape, dt)
    for var in SP.VARIANTS:
        ref, bound, d, d_bound = SP.reference(shape, dt, var)
        lat, out = SP.run_step(emu, shape, dt, var)
        SP.inside(lat, ref, bound, f"emu {shape} {dt} {var}")
        SP.inside(out, d, d_bound, f"emu d {shape} {dt} {var}")
        if var.phi == 0.0 and not var.single:            # the buffers the variant does not read may hold anything
            hs = [o[f"hist_{k}"] if var.order > k else nan for k in (1, 2, 3)]
            lat2, out2 = SP.run_step(emu, shape, dt, var, hist=hs)
            assert torch.equal(lat2, lat) and torch.equal(out2, out)
    assert len(SP.VARIANTS) == 64 and {v.order for v in SP.VARIANTS} == {1, 2, 3, 4}


@pytest.mark.parametrize("case", SP.INPUT_CASES, ids=[f"mode{c.mode}-cond{c.scale_cond}-dup{c.cfg_dup}-mask{int(c.with_mask)}" for c in SP.INPUT_CASES])
def test_emulator_scaled_input(case):
    emu = SigmaEmuOps()
    for shape in SP.INPUT_SHAPES:
        for dtype, u in ((torch.float32, 0.0), (torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)):
            ref = SP.input_reference(shape, case, SP.INPUT_DENOM)
            got = SP.run_input(emu, shape, case, dtype, SP.INPUT_DENOM).double()
            assert ((got - ref).abs() <= (2.0 ** -24 + u) * ref.abs() + 2.0 ** -140).all(), (shape, dtype)
            assert torch.equal(SP.run_input(emu, shape, case, dtype, 1.0), SP.run_input(emu, shape, case, dtype, 1.0, scaled=False))      # denom = 1: unet_input's bits
        CL = shape[3]
        assert not got[..., 2 * CL + (1 if case.mode == 0 else 0):].any()


def test_emulator_plain_input_with_the_reciprocal():
    """the 2-D path: nchw_to_nhwc(scale = the f32 reciprocal) against latents / denom, inside the two roundings of sigma_spec.K_PLAIN_INPUT plus the storage type's"""
    emu = SigmaEmuOps()
    for shape in SP.INPUT_SHAPES:
        ref = SP.plain_input_reference(shape, SP.INPUT_DENOM)
        for dtype, u in ((torch.float32, 0.0), (torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)):
            got = SP.run_plain_input(emu, shape, dtype, SP.INPUT_DENOM).double()
            assert ((got - ref).abs() <= (SP.gamma(SP.K_PLAIN_INPUT) + u) * ref.abs() + 2.0 ** -140).all(), (shape, dtype)
            assert not got[..., shape[3]:].any()


# ---- the C surface, no device --------------------------------------------------------------------------------------------------------------------------------
def _lib():
    from followyourclick_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib, _lib.load()


FIELDS = ["pred", "latents", "coef", "B", "F", "HW", "c_latent", "ld", "cfg", "guidance", "dtype", "pred_single", "video_scale", "hist_out", "hist_1", "hist_2",
          "hist_3", "order", "noise", "guidance_rescale", "workspace", "workspace_bytes"]
INPUT_FIELDS = ["base", "denom", "scale_cond"]


def test_binding_and_python_surface(tmp_path):
    from followyourclick_amd import _lib as L, ops, profiling
    assert [n for n, _ in L.CfgSigmaArgs._fields_] == FIELDS and [n for n, _ in L.UnetInputScaledArgs._fields_] == INPUT_FIELDS
    assert L.FYC_VERSION == 308 and L.OPS["fyc_cfg_sigma_step"] is L.CfgSigmaArgs and L.OPS["fyc_unet_input_scaled"] is L.UnetInputScaledArgs
    assert "fyc_cfg_sigma_workspace_bytes" in L.MISC
    header = os.path.join(os.path.dirname(L.HERE), "include", "fyc.h")
    with open(header) as fh:
        head = fh.read()
    assert "#define FYC_VERSION 308" in head and "} fyc_cfg_sigma_args;" in head and "} fyc_unet_input_scaled_args;" in head
    src = tmp_path / "abi.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{header}"\nint main(void){{'
                   'printf("%zu %zu %zu %zu", sizeof(fyc_cfg_sigma_args), sizeof(fyc_unet_input_scaled_args), sizeof(fyc_cfg_solver_args), sizeof(fyc_unet_input_args));'
                   + "".join(f'printf(" %zu", offsetof(fyc_cfg_sigma_args, {f}));' for f in FIELDS)
                   + "".join(f'printf(" %zu", offsetof(fyc_unet_input_scaled_args, {f}));' for f in INPUT_FIELDS) + "return 0;}")
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    size, isize, solver, uin, *offs = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == ctypes.sizeof(L.CfgSigmaArgs) and isize == ctypes.sizeof(L.UnetInputScaledArgs)
    assert solver == ctypes.sizeof(L.CfgSolverArgs) and uin == ctypes.sizeof(L.UnetInputArgs)          # the existing structs are untouched
    assert offs == [getattr(L.CfgSigmaArgs, f).offset for f in FIELDS] + [getattr(L.UnetInputScaledArgs, f).offset for f in INPUT_FIELDS]
    lib = _lib()[1]
    assert lib.fyc_version() == 308 and all(hasattr(lib, n) for n in ("fyc_cfg_sigma_step", "fyc_cfg_sigma_workspace_bytes", "fyc_unet_input_scaled"))
    for name in ("cfg_sigma_step", "unet_input_scaled"):
        sig = inspect.signature(getattr(ops.HipOps, name)).parameters
        assert list(inspect.signature(getattr(SigmaEmuOps, name)).parameters) == list(sig), name
        assert not hasattr(EmuOps, name) and not hasattr(SolverEmuOps, name)
    sig = inspect.signature(ops.HipOps.cfg_sigma_step).parameters
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("hist_out", "hist_1", "hist_2", "hist_3", "order", "noise", "guidance_rescale"))
    sig = inspect.signature(ops.HipOps.unet_input_scaled).parameters
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("denom", "scale_cond", "mode"))

    class Inner:          # the profiling wrapper forwards both
        name = "inner"

        def cfg_sigma_step(self, *a, **k):
            return ("sigma", a, k)

        def unet_input_scaled(self, *a, **k):
            return ("input", a, k)
    timed = profiling.TimedOps(Inner())
    timed.enabled = False
    assert timed.cfg_sigma_step(1, order=2) == ("sigma", (1,), dict(order=2)) and timed.unet_input_scaled(2, denom=3.0) == ("input", (2,), dict(denom=3.0))


LAT_BYTES = 2 * 4 * 16 * 1031 * 4


def _args(L, fields, shape=(2, 16, 1031, 4, 16)):
    """fyc_cfg_sigma_args around a valid fourth-order problem with noise, with `fields` written over it"""
    a = L.CfgSigmaArgs()
    a.pred, a.latents, a.coef = 0x10000000, 0x20000000, 0x30000000
    a.hist_out, a.hist_1, a.hist_2, a.hist_3, a.noise = 0x50000000, 0x60000000, 0x70000000, 0x80000000, 0x90000000
    a.B, a.F, a.HW, a.c_latent, a.ld = shape
    a.cfg, a.guidance, a.dtype, a.order = 1, 8.0, 1, 4
    a.guidance_rescale, a.workspace, a.workspace_bytes = 0.7, 0x40000000, 1 << 20
    for k, v in fields.items():
        setattr(a, k, v)
    return a


BAD = [(dict(pred=None), b"null"), (dict(latents=None), b"null"), (dict(coef=None), b"null"),
       (dict(B=0), b"dims"), (dict(ld=3), b"dims"), (dict(dtype=7), b"dtype"),
       (dict(order=0), b"order"), (dict(order=5), b"order"), (dict(order=2, hist_1=None), b"hist_1"), (dict(hist_1=None), b"hist_1"), (dict(hist_2=None), b"hist_2"),
       (dict(hist_3=None), b"hist_3"), (dict(order=3, hist_2=None), b"hist_2"),
       (dict(hist_out=0x20000000), b"aliases latents"), (dict(hist_out=0x20000000 + LAT_BYTES - 4), b"aliases latents"), (dict(hist_out=0x60000000), b"aliases hist_1"),
       (dict(hist_out=0x70000000 - LAT_BYTES + 4), b"aliases hist_2"), (dict(hist_out=0x80000000), b"aliases hist_3"),
       (dict(noise=0x50000000 + 4), b"noise aliases hist_out"), (dict(noise=0x20000000), b"noise aliases latents"), (dict(noise=0x60000000 + LAT_BYTES - 4), b"noise aliases hist_1"),
       (dict(noise=0x70000000), b"noise aliases hist_2"), (dict(noise=0x80000000 - 4), b"noise aliases hist_3"),
       (dict(cfg=0, guidance_rescale=0.0, pred_single=0xA0000000), b"pred_single"),
       (dict(guidance_rescale=-0.1), b"guidance_rescale"), (dict(guidance_rescale=1.5), b"guidance_rescale"), (dict(guidance_rescale=float("nan")), b"guidance_rescale"),
       (dict(cfg=0), b"cfg"), (dict(workspace=None), b"workspace"), (dict(workspace_bytes=1095), b"workspace"), (dict(workspace=0x40000004), b"workspace"),
       (dict(F=1, HW=1, c_latent=1, ld=1), b"dims")]


@pytest.mark.parametrize("fields,word", BAD, ids=[",".join(f"{k}={v}" for k, v in b[0].items()) for b in BAD])
def test_bad_arguments_are_refused_by_the_library_without_gpu(fields, word):
    """refused before anything that needs a device or fyc_init (this process never calls fyc_init: a check behind it would report that instead)"""
    L, lib = _lib()
    assert lib.fyc_cfg_sigma_step(ctypes.byref(_args(L, fields)), None) != 0
    msg = lib.fyc_last_error()
    assert word in msg and b"fyc_cfg_sigma_step" in msg and b"fyc_init" not in msg, msg


def test_good_arguments_reach_the_init_check_and_the_query_launches_nothing():
    L, lib = _lib()
    for fields in (dict(), dict(order=1, hist_1=None, hist_2=None, hist_3=None), dict(order=1, hist_out=None, hist_1=None, hist_2=None, hist_3=None, noise=None),
                   dict(order=3, hist_3=None), dict(noise=None), dict(dtype=0), dict(dtype=2, ld=5, c_latent=3), dict(guidance_rescale=0.0, workspace=None, cfg=0),
                   dict(pred_single=0xA0000000, video_scale=0.3), dict(hist_out=0x20000000 + LAT_BYTES), dict(noise=0x50000000 + LAT_BYTES)):
        assert lib.fyc_cfg_sigma_step(ctypes.byref(_args(L, fields)), None) != 0
        assert b"fyc_init" in lib.fyc_last_error(), (fields, lib.fyc_last_error())
    assert lib.fyc_cfg_sigma_step(None, None) != 0 and b"null" in lib.fyc_last_error()
    # the workspace is the DDIM rescale's: 2 samples x 17 runs of 1024 rows x 4 f64, then 2 f32 factors, in 256-byte units
    assert lib.fyc_cfg_sigma_workspace_bytes(ctypes.byref(_args(L, {}))) == 1280
    assert lib.fyc_cfg_sigma_workspace_bytes(ctypes.byref(_args(L, dict(guidance_rescale=0.0)))) == 0
    assert lib.fyc_cfg_sigma_workspace_bytes(ctypes.byref(_args(L, dict(B=0)))) == 0
    assert lib.fyc_cfg_sigma_workspace_bytes(None) == 0


def _input_args(L, fields, **base):
    s = L.UnetInputScaledArgs()
    a = s.base
    a.latents, a.mask, a.first, a.x = 0x10000000, 0x20000000, 0x30000000, 0x40000000
    a.B, a.F, a.HW, a.c_latent, a.c_pad, a.cfg_dup, a.mask_frames, a.dtype, a.mode = 2, 3, 20, 4, 16, 2, 1, 1, 0
    s.denom, s.scale_cond = 2.0, 1
    for k, v in base.items():
        setattr(a, k, v)
    for k, v in fields.items():
        setattr(s, k, v)
    return s


INPUT_BAD = [(dict(denom=0.5), {}, b"denom"), (dict(denom=float("inf")), {}, b"denom"), (dict(denom=float("nan")), {}, b"denom"), (dict(denom=-2.0), {}, b"denom"),
             (dict(scale_cond=2), {}, b"scale_cond"), (dict(scale_cond=1), dict(mode=1), b"scale_cond"), ({}, dict(latents=None), b"null"), ({}, dict(x=None), b"null"),
             ({}, dict(c_pad=8), b"dims"), ({}, dict(mode=2), b"mode"), ({}, dict(cfg_dup=3), b"cfg_dup"), ({}, dict(mask_frames=2), b"mask_frames"), ({}, dict(dtype=9), b"dtype")]


@pytest.mark.parametrize("fields,base,word", INPUT_BAD, ids=[",".join(f"{k}={v}" for k, v in {**b[0], **b[1]}.items()) for b in INPUT_BAD])
def test_bad_input_arguments_are_refused_without_gpu(fields, base, word):
    L, lib = _lib()
    assert lib.fyc_unet_input_scaled(ctypes.byref(_input_args(L, fields, **base)), None) != 0
    msg = lib.fyc_last_error()
    assert word in msg and b"fyc_unet_input_scaled" in msg, msg
    assert lib.fyc_unet_input_scaled(None, None) != 0 and b"null" in lib.fyc_last_error()


# ---- front ends ------------------------------------------------------------------------------------------------------------------------------------------------
YAML = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", prediction_type="v_prediction")
ZERO_SNR = dict(YAML, rescale_betas_zero_snr=True)


def test_dropin_scheduler_surface(dropin, tmp_path):
    import diffusers
    from diffusers import schedulers
    assert "fyc" in diffusers.__version__
    mods = {"euler": "scheduling_euler_discrete", "euler_ancestral": "scheduling_euler_ancestral_discrete", "lms": "scheduling_lms_discrete"}
    for kind, cls in dropin_classes().items():
        mod = __import__(f"diffusers.schedulers.{mods[kind]}", fromlist=[cls.__name__])
        assert getattr(schedulers, cls.__name__) is cls is getattr(mod, cls.__name__)
        s = cls()
        assert (s.config.num_train_timesteps, s.config.beta_start, s.config.beta_end, s.config.beta_schedule, s.config.trained_betas, s.config.prediction_type,
                s.config.rescale_betas_zero_snr) == (1000, 0.0001, 0.02, "linear", None, "epsilon", False)
        assert s.order == 1 and len(s) == 1000 and isinstance(s.engine_config, SigmaConfig) and s.engine_config.kind == kind
        assert s.timesteps.dtype == torch.float64 and s.timesteps[0].item() == 999.0 and s.sigmas.shape == (1001,) and s.sigmas[-1].item() == 0.0
        assert s.init_noise_sigma.item() == s.sigmas.max().item() == SigmaTables(SigmaConfig(kind=kind)).init_noise_sigma
        kept = cls.from_config(dict(ZERO_SNR, skip_prk_steps=True, steps_offset=1, clip_sample=False, solver_order=3))
        assert kept.engine_config.rescale_betas_zero_snr and abs(kept.init_noise_sigma.item() - 4096.0) < 1e-3
        (tmp_path / kind / "scheduler").mkdir(parents=True)
        (tmp_path / kind / "scheduler" / "scheduler_config.json").write_text(
            '{"_class_name": "PNDMScheduler", "beta_schedule": "scaled_linear", "beta_start": 0.00085, "beta_end": 0.012, "skip_prk_steps": true}')
        ld = cls.from_pretrained(str(tmp_path / kind), subfolder="scheduler", prediction_type="v_prediction")
        assert ld.config.beta_schedule == "scaled_linear" and ld.config.prediction_type == "v_prediction"
        kept.set_timesteps(5)
        assert kept.timesteps.tolist() == [999.0, 749.25, 499.5, 249.75, 0.0] and kept.sigmas.shape == (6,)
        x = torch.randn(1, 4, 2, 2)
        t = kept.timesteps[2]
        assert torch.equal(kept.scale_model_input(x, t), x / ((kept.sigmas[2] ** 2 + 1) ** 0.5)) and kept.is_scale_input_called
        assert torch.equal(kept.add_noise(x, torch.ones_like(x), kept.timesteps[2:3]), x + torch.ones_like(x) * kept.sigmas[2])
        v = torch.randn(5, 1, 4, 2, 2)

        def run():          # the state: set_timesteps resets it, two runs give the same bits
            kept.set_timesteps(5)
            g, y = torch.Generator().manual_seed(4), x * kept.init_noise_sigma
            for i, tt in enumerate(kept.timesteps):
                kw = dict(generator=g) if kind != "lms" else {}
                y = kept.step(v[i], tt, y, **kw).prev_sample
            return y
        y1, y2 = run(), run()
        assert torch.equal(y1, y2) and torch.isfinite(y1).all()
        out = kept.step(v[0], kept.timesteps[4], x, return_dict=False)
        assert isinstance(out, tuple) and out[0].shape == x.shape
    euler = dropin_classes()["euler"](**YAML)
    euler.set_timesteps(5)
    x, v, t = torch.randn(1, 4, 2, 2) * 3, torch.randn(1, 4, 2, 2), euler.timesteps[1]
    plain = euler.step(v, t, x).prev_sample
    assert torch.equal(euler.step(v, t, x, s_churn=0.0, s_noise=1.3, generator=torch.Generator().manual_seed(1)).prev_sample, plain)
    assert torch.equal(euler.step(v, t, x, s_churn=2.0, s_tmin=1e6).prev_sample, plain)          # outside [s_tmin, s_tmax]: gamma = 0
    churned = euler.step(v, t, x, s_churn=2.0, generator=torch.Generator().manual_seed(1))
    # the reference's lines with gamma = min(2 / 5, sqrt(2) - 1) and the same noise
    sg, sg_to, gam = euler.sigmas[1], euler.sigmas[2], min(2.0 / 5, 2 ** 0.5 - 1)
    hat = sg * (gam + 1)
    xs = x + torch.randn(v.shape, generator=torch.Generator().manual_seed(1)) * (hat ** 2 - sg ** 2) ** 0.5
    x0 = v * (-sg / (sg ** 2 + 1) ** 0.5) + (xs / (sg ** 2 + 1))
    assert torch.allclose(churned.prev_sample, xs + ((xs - x0) / hat) * (sg_to - hat), rtol=1e-6, atol=1e-6) and not torch.equal(churned.prev_sample, plain)
    lms = dropin_classes()["lms"](**YAML)
    lms.set_timesteps(5)
    y = torch.randn(1, 4, 2, 2)
    for i, tt in enumerate(lms.timesteps):
        y = lms.step(torch.randn(1, 4, 2, 2), tt, y, order=2).prev_sample
        assert len(lms.derivatives) == min(i + 1, 2)
    assert abs(lms.get_lms_coefficient(1, 0, 0) - float(lms.sigmas[1] - lms.sigmas[0])) < 1e-5


MM = dict(num_attention_heads=8, num_transformer_block=1, attention_block_types=["Temporal_Self", "Temporal_Self"],
          temporal_position_encoding=True, temporal_position_encoding_max_len=24, temporal_attention_dim_div=1, zero_initialize=True)
TINY = dict(sample_size=8, in_channels=4, out_channels=4, block_out_channels=(64, 128, 256, 256), layers_per_block=2,
            cross_attention_dim=64, attention_head_dim=8, use_motion_module=True, motion_module_resolutions=(1, 2, 4, 8),
            unet_use_cross_frame_attention=False, unet_use_temporal_attention=False, use_fps_condition=True,
            use_first_frame_mask_condition_concat=True, motion_module_type="Vanilla", motion_module_kwargs=MM)


class Recording:
    """records the launches of an ops object by name (and what a step or an input build carries), forwarding everything"""

    def __init__(self, inner):
        self.inner, self.names, self.steps, self.inputs = inner, [], [], []

    def __getattr__(self, name):
        v = getattr(self.inner, name)
        if not callable(v) or name == "ensure_init":
            return v

        def call(*a, **kw):
            self.names.append(name)
            if name.startswith("cfg_"):
                ptr = lambda k: None if kw.get(k) is None else kw[k].data_ptr()      # noqa: E731
                self.steps.append((name, kw.get("order"), kw.get("guidance_rescale"), ptr("hist_out"), ptr("hist_1"), ptr("hist_3"), kw.get("noise") is not None))
            if name.startswith("unet_input") or name == "nchw_to_nhwc":
                self.inputs.append((name, kw.get("denom"), kw.get("scale_cond"), kw.get("scale")))
            return v(*a, **kw)
        return call


def test_pipeline_routes_by_the_scheduler(dropin, monkeypatch):
    from animatediff.models.unet import UNet3DConditionModel
    from animatediff.pipelines.pipeline_animation import AnimationPipeline
    from diffusers import AutoencoderKL, DDIMScheduler, DPMSolverMultistepScheduler
    from followyourclick_amd import ops as ops_mod
    from oracle import stubs
    classes = dropin_classes()
    assert type(make_sampler(None, DDIMConfig())) is DDIMSampler and type(make_sampler(None, SolverConfig())) is SolverSampler
    assert type(make_sampler(None, SigmaConfig())) is SigmaSampler
    with pytest.raises(TypeError, match="SigmaConfig"):
        make_sampler(None, object())
    monkeypatch.delenv("FYC_GUIDANCE_RESCALE", raising=False)
    monkeypatch.setattr(AnimationPipeline, "decode_latents", lambda self, latents: np.zeros((1, 3, 2, 64, 64), np.float32))      # routing only: no VAE run
    vae = AutoencoderKL(block_out_channels=(64, 128, 128, 128), layers_per_block=2, latent_channels=4)

    def run(scheduler, ops, steps=6, **kw):
        pipe = AnimationPipeline(vae=vae, text_encoder=stubs.StubTextEncoder(64), tokenizer=stubs.FakeTokenizer(), unet=UNet3DConditionModel(**TINY), scheduler=scheduler)
        rec = Recording(ops)
        monkeypatch.setattr(ops_mod, "impl", rec)
        pipe("a corgi", video_length=2, height=64, width=64, num_inference_steps=steps, guidance_scale=8.0, use_first_frame_mask_condition_concat=True,
             first_image_latents=torch.zeros(1, 4, 8, 8), generator=torch.Generator().manual_seed(0), **kw)
        return rec

    # a DDIM or DPM-Solver scheduler: the launches are the ones they were (plain / solver emulators lack the new ops: nobody asks for them)
    ddim = run(DDIMScheduler(steps_offset=1, clip_sample=False, **ZERO_SNR), EmuOps())
    assert [s[0] for s in ddim.steps] == ["cfg_ddim_step"] * 6 and [i[0] for i in ddim.inputs] == ["unet_input"] * 6
    sol = run(DPMSolverMultistepScheduler(**ZERO_SNR), SolverEmuOps())
    assert [s[0] for s in sol.steps] == ["cfg_solver_step"] * 6 and [i[0] for i in sol.inputs] == ["unet_input"] * 6
    other = [n for n in ddim.names if not n.startswith("cfg_")]
    assert [n for n in sol.names if not n.startswith("cfg_")] == other
    for kind, cls in classes.items():
        rec = run(cls(**ZERO_SNR), SigmaEmuOps(), eta=0.5)                    # eta is accepted and unused, as in the reference
        den = SigmaTables(SigmaConfig(kind=kind, **ZERO_SNR)).input_denominators(6)
        assert [s[0] for s in rec.steps] == ["cfg_sigma_step"] * 6 and [s[2] for s in rec.steps] == [0.0] * 6
        assert rec.inputs == [("unet_input_scaled", d, True, None) for d in den]          # one scaled input build per step, mask and first-frame block divided too
        assert [n.replace("unet_input_scaled", "unet_input") for n in rec.names if not n.startswith("cfg_")] == other      # the same forward around it
        assert [s[6] for s in rec.steps] == [kind == "euler_ancestral"] * 6
        if kind == "lms":
            assert [s[1] for s in rec.steps] == [1, 2, 3, 4, 4, 4]
            outs = [s[3] for s in rec.steps]
            assert len(set(outs[:4])) == 4 and outs[4] == outs[0] and outs[5] == outs[1]          # four history buffers, their roles rotating
            assert [s[4] for s in rec.steps[1:]] == outs[:-1] and rec.steps[0][4] is None           # hist_1 is the previous step's hist_out
            assert [s[5] for s in rec.steps] == [None, None, None, outs[0], outs[1], outs[2]]       # hist_3 only at order 4
        else:
            assert [s[1] for s in rec.steps] == [1] * 6 and [s[3] for s in rec.steps] == [None] * 6          # no history is stored
    assert [s[2] for s in run(classes["euler"](**ZERO_SNR), SigmaEmuOps(), guidance_rescale=0.7).steps] == [0.7] * 6
    with pytest.raises(ValueError, match="timestep 999"):
        run(classes["euler"](trained_betas=DDIMScheduler(**ZERO_SNR).betas.tolist()), SigmaEmuOps())


def test_sd_pipeline_routes_by_the_scheduler(dropin, monkeypatch):
    """the 2-D first-image path goes through the same samplers: plain latents, scaled by the f32 reciprocal through nchw_to_nhwc"""
    from diffusers import AutoencoderKL, StableDiffusionPipeline, UNet2DConditionModel
    from followyourclick_amd import ops as ops_mod
    from oracle import stubs
    monkeypatch.setattr(StableDiffusionPipeline, "decode_latents", lambda self, latents: np.zeros((1, 64, 64, 3), np.float32))      # routing only: no VAE run
    vae = AutoencoderKL(block_out_channels=(64, 128, 128, 128))
    sd15 = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
    for kind, cls in dropin_classes().items():
        rec = Recording(SigmaEmuOps())
        monkeypatch.setattr(ops_mod, "impl", rec)
        pipe = StableDiffusionPipeline(vae, stubs.StubTextEncoder(64), stubs.FakeTokenizer(), UNet2DConditionModel(sample_size=8, block_out_channels=(64, 128, 256, 256),
                                                                                                          cross_attention_dim=64), cls(**sd15), safety_checker=None)
        pipe("a corgi", height=64, width=64, num_inference_steps=3, guidance_scale=8.0, generator=torch.Generator().manual_seed(0), output_type="np")
        assert [s[:2] for s in rec.steps] == [("cfg_sigma_step", o) for o in ((1, 2, 3) if kind == "lms" else (1, 1, 1))]
        den = SigmaTables(SigmaConfig(kind=kind, **sd15)).input_denominators(3)
        scales = sorted({i[3] for i in rec.inputs if i[0] == "nchw_to_nhwc"}, reverse=False)
        assert scales == sorted(float(torch.tensor(1.0) / torch.tensor(d)) for d in den)


# ---- the sampler on the emulator ---------------------------------------------------------------------------------------------------------------------------
def tiny_cfg(**kw):
    return UNet3DConfig(block_out_channels=(64, 128, 256, 256), cross_attention_dim=64, sample_size=8, **kw)


# kind -> (the worst step's rel-L2 measured on the emulator against the hand loop, the bound = 1.4 x that)
HAND_LOOP = {"euler": (5.23e-5, 7.3e-5), "euler_ancestral": (6.35e-5, 8.9e-5), "lms": (6.35e-5, 8.9e-5)}


@pytest.mark.parametrize("kind", SP.KINDS)
def test_sigma_sampler_against_a_hand_loop(kind):
    """the tiny UNet of tests/test_engine_gpu.py, f32 on the emulator, 5 steps on the zero-SNR table with v_prediction.  The hand loop takes the emulator's forward
    (DDIMSampler.predict on an engine of its own, with the step's input denominator), forms the guided prediction in f64 and steps with the specification's reference
    formula (LMS: on the engine's closed-form coefficients).  Measured worst step (rel-L2, the errors grow along the trajectory): Euler 5.23e-5, Euler ancestral
    6.35e-5, LMS 6.35e-5; the bound is 1.4 x the measured figure (HAND_LOOP holds both) - a wrong coefficient order is orders of magnitude outside."""
    sd = W.make_weights(W.unet_state_shapes(Fn.tiny_unet_config()), 0)
    inp = W.seeded_inputs(Fn.tiny_unet_config(), 1, 4, 8, 8, seed=7)
    scfg = SigmaConfig(kind=kind, **ZERO_SNR)
    steps, guidance = 5, 8.0
    tb = SigmaTables(scfg)
    start = inp["latents"] * tb.init_noise_sigma

    traj = []
    smp = SigmaSampler(UNet3DEngine(pack_unet(sd, tiny_cfg(), torch.float32, "cpu"), ops=SigmaEmuOps()), scfg)
    out = smp.sample(start, inp["text"], steps, guidance, inp["first_image_latents"], inp["first_images_mask"], fps=[2], flow=[4],
                     callback=lambda i, t, l: traj.append((t, l.clone())), use_graph=True, eta=0.3, generator=torch.Generator().manual_seed(5),
                     use_clipped_model_output=True)          # use_graph, eta and use_clipped_model_output: accepted, unused
    assert [t for t, _ in traj] == [999.0, 749.25, 499.5, 249.75, 0.0] and torch.equal(out, traj[-1][1])

    hand = SigmaSampler(UNet3DEngine(pack_unet(sd, tiny_cfg(), torch.float32, "cpu"), ops=SigmaEmuOps()), scfg)
    st = hand.prepare(inp["text"], steps, 1, guidance, [2], [4])
    assert st["orders"] == ([1, 2, 3, 4, 4] if kind == "lms" else [1] * 5) and st["coef"].shape == (5, 8) and len(st["input_denom"]) == 5
    sig = tb.sigmas(steps)
    lat = start.clone().float()
    B, CL, F, H, Wd = lat.shape
    first, mask = inp["first_image_latents"].reshape(B, CL, H * Wd).float(), inp["first_images_mask"].float()[:, :, 0].reshape(B, 1, H * Wd)
    gen = torch.Generator().manual_seed(5)
    xs, vs, errs = [], [], []
    for i in range(steps):
        noise = torch.randn(lat.shape, generator=gen) if kind == "euler_ancestral" else None
        pred, _ = hand.predict(st, i, lat, first, mask, input_denom=st["input_denom"][i])
        p = pred.reshape(2, B, F, H * Wd, -1)[..., :CL].double()
        v = (p[0] + guidance * (p[1] - p[0])).permute(0, 3, 1, 2).reshape(lat.shape)
        xs.append(lat.clone())
        vs.append(v)
        ref, _ = SP.schedule_step(kind, "v_prediction", sig, i, xs, vs, noise=noise, lms_coeffs=tb.lms_coefficients(sig, i, st["orders"][i]) if kind == "lms" else None)
        errs.append(((traj[i][1].double() - ref).norm() / ref.norm()).item())
        lat = ref.float()
    print(f"{kind} sampler on the emulator vs hand loop: per-step rel-L2 {[f'{e:.2e}' for e in errs]}")
    assert torch.isfinite(out).all() and max(errs) < HAND_LOOP[kind][1], errs


def run_tiny_pipeline(g, kind, dtype, ops, device="cpu"):
    """the reference pipeline's run of tests/golden/pipeline_tiny_sigma.npz on an engine -> per-step relative L2 against its trajectory"""
    sd = W.make_weights(W.unet_state_shapes(Fn.tiny_unet_config()), int(g["unet_weight_seed"]))
    eng = UNet3DEngine(pack_unet(sd, tiny_cfg(), dtype, device), ops=ops)
    traj = []
    lat = SigmaSampler(eng, SigmaConfig(kind=kind, **YAML)).sample(
        g["latents"] * float(g["init_noise_sigma"]), g["text_embeddings"], 5, 8.0, g["first_image_latents"], g["first_images_mask"], fps=[2], flow=[4],
        generator=torch.Generator(device=device).manual_seed(int(g["generator_seed"])), callback=lambda i, t, l: traj.append(l.detach().cpu().clone()))
    assert lat.dtype == torch.float32
    ref = g[f"trajectory_{kind}"]
    return (torch.stack(traj) - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)


@pytest.mark.parametrize("kind", SP.KINDS)
def test_sampler_trajectory_matches_reference_pipeline(pipe_golden, kind):
    """5 steps of the real AnimationPipeline with the reference's scheduler class, CFG 8, mask + first-frame concat, fps / flow conditioning, on the emulator in f32:
    per-step rel-L2 < 5e-4, the bound of the DDIM run of the same model (tests/test_engine_emulated.py)"""
    assert float(pipe_golden["init_noise_sigma"]) == np.float32(SigmaTables(SigmaConfig(kind=kind, **YAML)).init_noise_sigma)
    err = run_tiny_pipeline(pipe_golden, kind, torch.float32, SigmaEmuOps())
    print(f"{kind} f32 pipeline trajectory on the emulator: per-step rel-L2 {[f'{e:.2e}' for e in err.tolist()]}")
    assert err.max().item() < 5e-4, err


# (kind, storage type) -> (the worst step's rel-L2 measured on the emulator against the golden, the bound = 1.4 x that)
TOL_16 = {("euler", "bf16"): (5.99e-2, 8.4e-2), ("euler", "f16"): (8.43e-3, 1.18e-2), ("euler_ancestral", "bf16"): (7.20e-2, 1.01e-1),
          ("euler_ancestral", "f16"): (9.07e-3, 1.27e-2), ("lms", "bf16"): (7.51e-2, 1.05e-1), ("lms", "f16"): (9.22e-3, 1.29e-2)}


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("kind", SP.KINDS)
def test_sampler_trajectory_in_16_bit_modes(pipe_golden, kind, dt):
    """the same run with bf16 / f16 storage on the emulator: the host side of the 16-bit modes (the sampler's f32 latents and histories against a 16-bit scaled UNet
    input and 16-bit predictions).  Measured worst step (the last but one, the errors grow along the trajectory) against the golden: Euler bf16 5.99e-2, f16 8.43e-3;
    Euler ancestral bf16 7.20e-2, f16 9.07e-3; LMS bf16 7.51e-2, f16 9.22e-3; the bound is 1.4 x the measured figure (TOL_16 holds both), the habit of
    test_sampler_and_vae_in_16_bit_modes"""
    err = run_tiny_pipeline(pipe_golden, kind, SP.SS.DT[dt], SigmaEmuOps())
    print(f"{kind} {dt} pipeline trajectory on the emulator: per-step rel-L2 {[f'{e:.2e}' for e in err.tolist()]}")
    assert err.max().item() < TOL_16[(kind, dt)][1], err
