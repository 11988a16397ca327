"""The image-editing pipelines on the CPU emulator (tests/emu_ops_edit.py): the three kernels' emulations against the f64 specification (tests/edit_spec.py), the
schedule tables of a run that starts part-way, add_noise_coefficients against the reference schedulers' add_noise, the three drop-in pipelines against every golden case
of tests/golden/pipeline_tiny_edit.npz (the reference's own pipelines; tools/make_golden_edit.py), their argument checks, refusals and noise draw order, the 9-channel
UNet2DConditionModel, and the launch sequence of a text-to-image call, which is the one it was."""
import hashlib
import sys

import numpy as np
import pytest
import torch

import edit_pipelines as EP
import edit_spec as ES
import trace_ops
from emu_ops_edit import EditEmuOps
from followyourclick_amd.engine import DDIMConfig, PNDMConfig, SigmaConfig, SolverConfig, UNet3DConfig
from followyourclick_amd.engine.sampler import DDIMSampler, PNDMSampler, SigmaSampler, SolverSampler
from followyourclick_amd.engine.scheduler import DDIMTables, PNDMTables, SigmaTables, SolverTables
from followyourclick_amd.engine.unet3d import UNet3DEngine
from followyourclick_amd.engine.weights import pack_unet
from oracle import functional as Fn
from oracle import weights as W


@pytest.fixture(scope="module")
def golden(golden_dir):
    return EP.load_golden(golden_dir)


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


# ---- the kernels' emulations against the specification ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ES.POSTERIOR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_posterior_latents_emulation_inside_the_bound(shape):
    emu = EditEmuOps()
    for var in ES.POSTERIOR_VARIANTS:
        ref = ES.posterior_reference(shape, var)
        lat, clean = ES.run_posterior(emu, shape, var, nan_unread=True)
        ES.inside(lat, *ref["latents"], f"posterior_latents latents {shape} {var}")
        if var.clean:
            ES.inside(clean, *ref["clean"], f"posterior_latents clean_out {shape} {var}")
        else:
            assert bool(torch.isnan(clean).all()), var
    # log-variances outside the clamp are clamped, not passed on: the operands hold some on either side, and the specification of the clamped moments is the same
    o = ES.posterior_operands(shape)
    C = shape[1]
    lv = o["moments"][:, C:]
    assert bool((lv < -30).any()) and bool((lv > 20).any())
    clamped = torch.cat([o["moments"][:, :C], lv.clamp(-30.0, 20.0)], dim=1)
    assert torch.equal(ES.posterior_latents(clamped, noise_post=o["noise_post"])["clean"][0], ES.posterior_latents(o["moments"], noise_post=o["noise_post"])["clean"][0])


@pytest.mark.parametrize("shape", ES.PREPARE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_inpaint_prepare_emulation_is_exact(shape):
    o = ES.prepare_operands(shape)
    N, H, Wd = shape
    masked, lat = torch.full((N, 3, H, Wd), float("nan")), torch.full((N, 1, H // 8, Wd // 8), float("nan"))
    EditEmuOps().inpaint_prepare(o["image"], o["mask"], masked=masked, mask_latent=lat)
    ref_masked, ref_lat = ES.inpaint_prepare(o["image"], o["mask"])
    assert torch.equal(masked, ref_masked) and torch.equal(lat, ref_lat)
    # the specification is prepare_mask_and_masked_image + F.interpolate(nearest) of the reference, restated with torch
    m = o["mask"].clone()
    m[m < 0.5] = 0
    m[m >= 0.5] = 1
    assert torch.equal(ref_masked, o["image"] * (m < 0.5)) and torch.equal(ref_lat, torch.nn.functional.interpolate(m, size=(H // 8, Wd // 8)))
    # 0.5 and its upper f32 neighbour repaint, the lower neighbour keeps
    vals = torch.tensor(ES.MASK_VALUES, dtype=torch.float32)
    assert ((vals < 0.5).tolist()) == [True, False, False, True, False, True, False]
    assert set(o["mask"][:, :, ::8, ::8].unique().tolist()) == set(vals.tolist()) or shape == (1, 8, 8)


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("shape", ES.BLEND_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_renoise_blend_emulation_inside_the_bound(shape, full):
    B, C, F, HW = shape
    o = ES.blend_operands(shape, full)
    lat = o["latents"].clone()
    EditEmuOps().renoise_blend(lat, o["orig"], o["noise"], o["mask"], c_x=ES.BLEND_COEF[0], c_n=ES.BLEND_COEF[1], B=B, C_=C, F=F, HW=HW)
    ES.inside(lat, *ES.blend_reference(shape, full), f"renoise_blend {shape} full={full}")
    # where the mask is exactly 0 the latents keep their bits; where it is exactly 1 they are the re-noised original's
    m = o["mask"].reshape(B, 1, 1, HW).expand(B, C, F, HW)
    assert torch.equal(lat[m == 0], o["latents"][m == 0])
    proper = (ES.f32(ES.BLEND_COEF[0]) * o["orig"] + ES.f32(ES.BLEND_COEF[1]) * o["noise"]).expand(B, C, F, HW)
    assert torch.equal(lat[m == 1], proper[m == 1])


# ---- schedules that start part-way ---------------------------------------------------------------------------------------------------------------------------
def tables(name):
    kw = dict(ES.SCHEDULERS[name][1])
    if name == "ddim":
        return DDIMTables(DDIMConfig(**kw))
    if name == "dpmpp2":
        return SolverTables(SolverConfig(**kw))
    if name == "plms":
        return PNDMTables(PNDMConfig(**kw))
    return SigmaTables(SigmaConfig(kind={"euler": "euler", "euler_a": "euler_ancestral", "lms": "lms"}[name], **kw))


@pytest.mark.parametrize("name", list(ES.SCHEDULERS))
def test_add_noise_coefficients_match_the_reference_schedulers(golden, name):
    """(c_x, c_n) = the reference scheduler's add_noise on the unit inputs (1, 0) and (0, 1) at every entry of its 5-step list, bit for bit"""
    tb = tables(name)
    ts, ref = golden[f"add_noise_timesteps/{name}"].tolist(), golden[f"add_noise/{name}"]
    assert [float(t) for t in tb.timesteps(ES.STEPS).tolist()] == ts
    got = torch.tensor([tb.add_noise_coefficients(t, ES.STEPS) for t in ts], dtype=torch.float64).float()
    assert torch.equal(got, ref), (got, ref)
    if name in ("euler", "euler_a", "lms"):
        assert bool((got[:, 0] == 1).all())
        with pytest.raises(ValueError, match="not an entry"):
            tb.add_noise_coefficients(500.5, ES.STEPS)
        with pytest.raises(ValueError, match="num_inference_steps"):
            tb.add_noise_coefficients(ts[0])
    else:
        with pytest.raises(ValueError, match="outside"):
            tb.add_noise_coefficients(1000)


def test_sliced_schedules_follow_the_reference_state_machines():
    # start_index = 0 is the table it was
    for name in ES.SCHEDULERS:
        tb = tables(name)
        full = tb.coefficient_table(ES.STEPS)
        assert torch.equal(tb.coefficient_table(ES.STEPS, 0), full)          # (DDIMTables' second argument is eta: 0 as well)
    # DPM-Solver++: the warm-up starts over at the slice, the lower-order final step is found by its place in the full list
    sol = tables("dpmpp2")
    assert sol.plan(5) == [1, 2, 2, 2, 1] and sol.plan(5, 2) == [1, 2, 1] and sol.plan(5, 4) == [1]
    assert torch.equal(sol.coefficient_table(5, 2)[1], torch.tensor(sol.step_coefficients(sol.timesteps(5).tolist(), 3, 2), dtype=torch.float64).float())
    # LMS: the order of the step's place in the list (min(i + 1, 4)), cut to the derivatives stored since the slice - the first coefficients of the full-order set
    lms = tables("lms")
    assert lms.plan(5) == [1, 2, 3, 4, 4] and lms.plan(5, 2) == [1, 2, 3]
    sig = lms.sigmas(5)
    row = lms.coefficient_table(5, 2)[0]
    want = SigmaTables.lms_coefficients(sig, 2, 3)
    assert abs(float(row[3]) - want[0]) < 1e-6 * abs(want[0]) and row[4:7].tolist() == [0.0, 0.0, 0.0]
    assert abs(want[0] - SigmaTables.lms_coefficients(sig, 2, 1)[0]) > 1e-3 * abs(want[0])          # not the first-order coefficient a fresh run would take
    # Euler: stateless, the rows of the slice
    eu = tables("euler")
    assert torch.equal(eu.coefficient_table(5, 2), eu.coefficient_table(5)[2:])
    # PLMS: the counter starts at the slice - evaluation 1 redoes step 0 from the saved sample although the sliced list [601, 401, 201, 1] repeats nothing
    pn = tables("plms")
    assert pn.timesteps(5).tolist() == [801, 601, 601, 401, 201, 1]
    plan = pn.plan(5, 2)
    assert [(e.timestep, e.prev_timestep, e.order) for e in plan] == [(601, 401, 1), (601, 401, 2), (201, 1, 2), (1, -199, 3)]
    assert plan[0].sample_out and plan[1].sample_in and not plan[2].sample_in
    for bad in (-1, 6):
        with pytest.raises(ValueError, match="start_index"):
            pn.plan(5, bad)
    with pytest.raises(ValueError, match="Runge-Kutta"):
        PNDMTables(PNDMConfig(**dict(ES.SCHEDULERS["plms"][1], skip_prk_steps=False))).plan(5, 2)


# ---- the pipelines against the reference's runs --------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def models(golden, dropin, monkeypatch):
    from followyourclick_amd import ops as ops_mod
    monkeypatch.setattr(ops_mod, "impl", EditEmuOps())
    return EP.build_models(golden)


@pytest.mark.parametrize("case", ES.CASES, ids=ES.case_key)
def test_pipeline_matches_the_reference_run(golden, models, monkeypatch, case):
    """every evaluation's latents against the reference pipeline's, rel-L2 < 5e-4 in f32 (the bound tests/test_pndm.py and the sigma / DDIM runs hold the same tiny model
    to); the final images within 2e-3 (the tolerance of the sd2d_pipeline test); timesteps, callback indices and every noise tensor drawn, in order, bit for bit"""
    key = ES.case_key(case)
    run = EP.run_case(case, golden, EP.build_pipeline(case, models), monkeypatch)
    assert run.timesteps == golden[f"{key}/timesteps"].tolist()
    assert run.callbacks == golden[f"{key}/callbacks"].tolist()
    n_noise = sum(k.startswith(f"{key}/noise_") for k in golden)
    # (the sampler's own per-step draws carry the one-frame clip's frame axis, (1, 4, 1, 8, 8): the same numbers in the same order)
    assert len(run.drawn) == n_noise, "noise draw count"
    for k, t in enumerate(run.drawn):
        ref = golden[f"{key}/noise_{k}"]
        assert t.dtype == ref.dtype and (tuple(t.shape) == tuple(ref.shape) or (k >= 2 and tuple(t.shape) == (1, 4, 1, 8, 8))) and torch.equal(t.reshape(ref.shape), ref), f"noise draw {k}"
    err = EP.trajectory_error(run, golden, case)
    img = (run.images - golden[f"{key}/images"]).abs().max().item()
    print(f"{key} f32 on the emulator: per-evaluation rel-L2 {[f'{e:.2e}' for e in err.tolist()]}, images max abs {img:.2e}")
    assert err.max().item() < 5e-4, err
    assert img < 2e-3


def test_noise_draw_order_and_shapes(golden):
    """what the reference drew, by case: img2img / legacy the posterior's noise then add_noise's, inpaint the initial latents then the posterior's; then one more per
    evaluation with stochastic DDIM and Euler ancestral - and with plain Euler, whose step() draws its churn noise used or not.  All (1, 4, 8, 8) f32; that the drop-in
    draws the same tensors in the same order is asserted per case in test_pipeline_matches_the_reference_run"""
    for case in ES.CASES:
        key = ES.case_key(case)
        n = sum(k.startswith(f"{key}/noise_") for k in golden)
        per_step = len(golden[f"{key}/timesteps"]) if (case.eta or case.scheduler in ("euler", "euler_a")) else 0
        assert n == 2 + per_step, key
        assert all(tuple(golden[f"{key}/noise_{k}"].shape) == (1, 4, 8, 8) and golden[f"{key}/noise_{k}"].dtype == torch.float32 for k in range(n))


def test_argument_checks_and_refusals(golden, models, monkeypatch):
    from diffusers import StableDiffusionImg2ImgPipeline, StableDiffusionInpaintPipeline, StableDiffusionInpaintPipelineLegacy  # noqa: F401
    import diffusers.pipelines
    import diffusers.pipelines.stable_diffusion as SD
    for name in ("StableDiffusionImg2ImgPipeline", "StableDiffusionInpaintPipeline", "StableDiffusionInpaintPipelineLegacy"):
        assert getattr(diffusers.pipelines, name) is getattr(SD, name)
    img = EP.build_pipeline(ES.Case("img2img", "ddim", 0.6, 0.0), models)
    kw = dict(image=golden["image"], num_inference_steps=5, output_type="np")
    with pytest.raises(ValueError, match="strength"):
        img("a corgi", strength=1.5, **kw)
    with pytest.raises(ValueError, match="zero steps"):
        img("a corgi", strength=0.1, **kw)
    with pytest.raises(ValueError, match="`prompt`"):
        img(3, strength=0.6, **kw)
    with pytest.raises(ValueError, match="callback_steps"):
        img("a corgi", strength=0.6, callback_steps=0, **kw)
    with pytest.raises(ValueError, match="Cannot duplicate"):
        img(["a", "b", "c"], strength=0.6, **dict(kw, image=torch.cat([golden["image"]] * 2)))
    with pytest.raises(ValueError, match="generators"):
        img("a corgi", strength=0.6, generator=[torch.Generator(), torch.Generator()], **kw)
    with pytest.raises(ValueError, match="components"):
        StableDiffusionImg2ImgPipeline.from_pretrained("unused", vae=models["vae"])
    # PNDM in Runge-Kutta mode cannot start part-way; from the start (strength 1) it runs
    prk = EP.build_pipeline(ES.Case("img2img", "plms", 0.6, 0.0), models)
    prk.scheduler = type(prk.scheduler)(**dict(ES.SCHEDULERS["plms"][1], skip_prk_steps=False))
    with pytest.raises(ValueError, match="Runge-Kutta"):
        prk("a corgi", strength=0.6, **kw)
    leg = EP.build_pipeline(ES.Case("legacy", "ddim", 0.6, 0.0), models)
    with pytest.raises(NotImplementedError, match="add_predicted_noise"):
        leg("a corgi", image=golden["image"], mask_image=torch.zeros(1, 4, 8, 8), add_predicted_noise=True, num_inference_steps=5)
    inp = EP.build_pipeline(ES.Case("inpaint", "ddim", None, 0.0), models)
    with pytest.raises(TypeError, match="mask"):
        inp("a corgi", image=golden["image"], mask_image=np.zeros((64, 64), np.float32), height=64, width=64)
    with pytest.raises(ValueError, match=r"\[-1, 1\]"):
        inp("a corgi", image=golden["image"] * 3, mask_image=golden["mask"], height=64, width=64)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        inp("a corgi", image=golden["image"], mask_image=golden["mask"] * 2, height=64, width=64)
    with pytest.raises(ValueError, match="divisible by 8"):
        inp("a corgi", image=golden["image"], mask_image=golden["mask"], height=60, width=64)
    four = EP.build_pipeline(ES.Case("inpaint", "ddim", None, 0.0), dict(models, unet9=models["unet"]))
    with pytest.raises(ValueError, match="Incorrect configuration"):
        four("a corgi", image=golden["image"], mask_image=golden["mask"], height=64, width=64, num_inference_steps=2)


def test_eta_reaches_the_ddim_sampler_in_the_text_to_image_pipeline(golden, models, monkeypatch):
    from diffusers import DDIMScheduler, StableDiffusionPipeline
    from oracle import stubs
    pipe = StableDiffusionPipeline(models["vae"], stubs.StubTextEncoder(64), stubs.FakeTokenizer(), models["unet"], DDIMScheduler(**ES.SCHEDULERS["ddim"][1]), safety_checker=None)
    lat = torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(1))
    call = lambda **kw: pipe("a corgi", height=64, width=64, num_inference_steps=3, latents=lat.clone(), output_type="np", **kw).images      # noqa: E731
    a, b = call(), call(eta=0.0, generator=torch.Generator().manual_seed(2))
    c, d = call(eta=0.5, generator=torch.Generator().manual_seed(2)), call(eta=0.5, generator=torch.Generator().manual_seed(2))
    assert np.array_equal(a, b) and np.array_equal(c, d) and not np.array_equal(a, c)


def test_unet2d_with_nine_input_channels(dropin, monkeypatch):
    from diffusers import UNet2DConditionModel
    from followyourclick_amd.engine.schema import unet_schema
    monkeypatch.delenv("FYC_UNET_VARIANTS", raising=False)
    m = UNet2DConditionModel(in_channels=9, **EP.UNET_KW, compute_dtype=torch.float32)
    assert m.config.in_channels == 9 and m.in_channels == 9 and m.config.out_channels == 4
    ec = m.engine_config
    assert ec.in_channels == 4 and ec.conv_in_channels == 9 and ec.use_first_frame_mask_condition_concat and not ec.use_motion_module
    sd = m.state_dict()
    assert tuple(sd["conv_in.weight"].shape) == (64, 9, 3, 3) and tuple(sd["conv_out.weight"].shape) == (4, 64, 3, 3)
    # the schema is the reference 2-D module's: the names and shapes of the oracle's restatement, 9 input channels
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(W.unet_state_shapes(EP.cfg_2d(concat=True))) == dict(unet_schema(ec))
    w = W.make_weights(W.unet_state_shapes(EP.cfg_2d(concat=True)), 5)
    assert not any(m.load_state_dict(w, strict=True))
    assert all(torch.equal(v, w[k]) for k, v in m.state_dict().items())
    # a 4-channel model is what it was
    m4 = UNet2DConditionModel(**EP.UNET_KW, compute_dtype=torch.float32)
    assert m4.engine_config.conv_in_channels == 4 and not m4.engine_config.use_first_frame_mask_condition_concat
    # the SD-2 inpainting config.json: 9 input channels, linear projections, one head count per level - behind the variants switch, as the SD-2.1 family is
    # (its keys as they are, the widths cut to a quarter so that the test builds 1/16 of the parameters; conv_in.weight is (320, 9, 3, 3) at full width)
    sd2 = dict(_class_name="UNet2DConditionModel", _diffusers_version="0.8.0", act_fn="silu", attention_head_dim=[5, 10, 20, 20], block_out_channels=[80, 160, 320, 320],
               center_input_sample=False, cross_attention_dim=1024, down_block_types=["CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"],
               downsample_padding=1, dual_cross_attention=False, flip_sin_to_cos=True, freq_shift=0, in_channels=9, layers_per_block=2, mid_block_scale_factor=1,
               norm_eps=1e-05, norm_num_groups=16, out_channels=4, sample_size=64, up_block_types=["UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"],
               use_linear_projection=True, upcast_attention=False)
    with pytest.raises(NotImplementedError, match="FYC_UNET_VARIANTS"):
        UNet2DConditionModel.from_config(sd2)
    monkeypatch.setenv("FYC_UNET_VARIANTS", "1")
    big = UNet2DConditionModel.from_config(sd2)
    assert big.engine_config.conv_in_channels == 9 and big.engine_config.use_linear_projection and tuple(big.conv_in.weight.shape) == (80, 9, 3, 3)
    assert tuple(big.engine_config.attention_head_dim) == (5, 10, 20, 20) and big.config.in_channels == 9


# ---- a text-to-image call launches what it launched ----------------------------------------------------------------------------------------------------------
# sha256 over the lines of the recording backend's log (tests/trace_ops.py: every launch with its scalars and its buffers by storage, offset, shape and stride) of
# text_to_image_trace() below, recorded on the parent commit of the image-editing change, and the number of launches in it
PARENT_TRACE = ("e9d70142401dd700cd22515f70943cb092f72167dfcf986ee38e604379ba65e2", 1177)


def text_to_image_trace():
    """DDIMSampler.sample on the tiny 2-D model (no concat conditioning) in bf16 on the recording backend: 3 steps, CFG 8, start_index and blend left at their defaults"""
    cfg = UNet3DConfig(block_out_channels=(64, 128, 256, 256), cross_attention_dim=64, sample_size=8, use_motion_module=False, use_fps_condition=False,
                       use_first_frame_mask_condition_concat=False)
    ops = trace_ops.TraceOps(fused=True)
    eng = UNet3DEngine(pack_unet(W.make_weights(W.unet_state_shapes(EP.cfg_2d()), 0), cfg, torch.bfloat16, "cpu"), ops=ops)
    smp = DDIMSampler(eng, DDIMConfig(**ES.SCHEDULERS["ddim"][1]))
    ops.reset()
    smp.sample(torch.zeros(1, 4, 1, 8, 8), torch.zeros(2, 77, 64), 3, 8.0)
    lines = ops.lines()
    return hashlib.sha256("\n".join(lines).encode()).hexdigest(), len(lines)


def test_text_to_image_launches_are_the_parents():
    assert text_to_image_trace() == PARENT_TRACE


def test_start_index_zero_is_the_full_run_and_blend_runs_one_launch_per_entry(golden):
    """on the emulator's sampler: start_index = 0 gives the bits of a call without it; a blend adds one renoise_blend behind every step kernel, with the coefficients of
    that entry's own timestep"""
    sd = W.make_weights(W.unet_state_shapes(EP.cfg_2d()), int(golden["unet_weight_seed"]))
    cfg = UNet3DConfig(block_out_channels=(64, 128, 256, 256), cross_attention_dim=64, sample_size=8, use_motion_module=False, use_fps_condition=False,
                       use_first_frame_mask_condition_concat=False)
    calls = []

    class Rec(EditEmuOps):
        def renoise_blend(self, *a, **k):
            calls.append(("blend", k["c_x"], k["c_n"]))
            return super().renoise_blend(*a, **k)

        def cfg_ddim_step(self, *a, **k):
            calls.append(("step",))
            return super().cfg_ddim_step(*a, **k)
    eng = UNet3DEngine(pack_unet(sd, cfg, torch.float32, "cpu"), ops=Rec())
    smp = DDIMSampler(eng, DDIMConfig(**ES.SCHEDULERS["ddim"][1]))
    g = torch.Generator().manual_seed(3)
    lat, text = torch.randn(1, 4, 1, 8, 8, generator=g), golden["text_embeddings"]
    assert torch.equal(smp.sample(lat, text, 3, 8.0), smp.sample(lat, text, 3, 8.0, start_index=0, blend=None))
    orig, noise = torch.randn(1, 4, 8, 8, generator=g), torch.randn(1, 4, 8, 8, generator=g)
    mask = (torch.rand(1, 1, 8, 8, generator=g) < 0.5).float().expand(1, 4, 8, 8)
    calls.clear()
    out = smp.sample(lat, text, 5, 8.0, start_index=2, blend=(orig, noise, mask))
    ts = smp.tables.timesteps(5).tolist()[2:]
    assert calls == [c for t in ts for c in (("step",), ("blend", *smp.tables.add_noise_coefficients(t)))]
    # after the last blend the kept region is the original noised to the LAST entry's own timestep (1), not to a clean image
    c_x, c_n = smp.tables.add_noise_coefficients(ts[-1])
    keep = mask[:, :, None] == 1
    assert torch.equal(out[keep], (ES.f32(c_x) * orig + ES.f32(c_n) * noise)[:, :, None][keep])
    with pytest.raises(ValueError, match="channels differ"):
        smp.sample(lat, text, 5, 8.0, start_index=2, blend=(orig, noise, torch.rand(1, 4, 8, 8, generator=g)))
    for cls, conf in ((SolverSampler, SolverConfig(**ES.SCHEDULERS["dpmpp2"][1])), (SigmaSampler, SigmaConfig(kind="lms", **ES.SCHEDULERS["lms"][1])),
                      (PNDMSampler, PNDMConfig(**ES.SCHEDULERS["plms"][1]))):
        with pytest.raises(ValueError, match="start_index"):
            cls(eng, conf).sample(lat, text, 5, 8.0, start_index=7)
