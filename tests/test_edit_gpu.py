"""The image-editing front end on the MI355X: fyc_posterior_latents, fyc_inpaint_prepare and fyc_renoise_blend per element against the f64 specification
(tests/edit_spec.py) inside the bounds derived there, in guarded buffers; their bit-level properties; the three drop-in pipelines against the same run on the emulator
and against the reference's own runs (tests/golden/pipeline_tiny_edit.npz).  Reads tests/golden/ and the specification only."""
import sys

import pytest
import torch

import edit_pipelines as EP
import edit_spec as ES
import kernel_compare as KC
from emu_ops_edit import EditEmuOps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64          # f32 elements on either side of an output: 256 bytes, so the output keeps the allocation's 16-byte alignment; GUARD + 1 breaks it (the scalar path)
LABELS = KC.Labels(row=lambda i: f"row {i}", col=lambda j: f"element {j}")


@pytest.fixture(scope="module")
def hip():
    from followyourclick_amd import ops
    return ops.get()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return EP.load_golden(golden_dir)


class Guarded:
    """an f32 device tensor of a shape inside a buffer with `lead` and GUARD elements of NaN around it"""

    def __init__(self, shape, init=None, lead=GUARD):
        n = int(torch.Size(shape).numel())
        self.buf = torch.full((lead + n + GUARD,), float("nan"), device=DEV)
        self.t = self.buf[lead: lead + n].view(shape)
        if init is not None:
            self.t.copy_(init)
        self.before = self.buf.clone()
        self.mask = torch.zeros(lead + n + GUARD, dtype=torch.bool)
        self.mask[lead: lead + n] = True

    def guard(self):
        return KC.Guard(self.before, self.buf, self.mask)


def judge(out: Guarded, ref, bound, tag):
    """every element inside its bound, nothing outside the output written -> worst |got - ref| / bound"""
    torch.cuda.synchronize()
    got = out.t.detach().cpu().reshape(1, -1)
    fig = KC.compare(got, ref.reshape(1, -1), dtype="f32", bound=bound.reshape(1, -1).clamp_min(1e-300), rtol=KC.RTOL["f32"], labels=LABELS, guard=out.guard(), tag=tag)
    return fig["elem_ratio"]


def untouched(out: Guarded):
    torch.cuda.synchronize()
    return torch.equal(KC._bits(out.buf), KC._bits(out.before))


def dev(t, lead=GUARD):
    """a device copy of an operand; lead != GUARD: at an address that is not 16-byte aligned"""
    return Guarded(t.shape, t, lead).t


# ---- fyc_posterior_latents -----------------------------------------------------------------------------------------------------------------------------------
def launch_posterior(hip, shape, var, lead=GUARD, moments=None):
    o = ES.posterior_operands(shape)
    lat, clean = Guarded(shape, lead=lead), Guarded(shape, lead=lead)
    hip.posterior_latents(dev(o["moments"] if moments is None else moments, lead), lat.t, noise_post=dev(o["noise_post"], lead) if var.post else None,
                          noise_add=dev(o["noise_add"], lead) if var.add else None, clean_out=clean.t if var.clean else None, scale=ES.VAE_SCALE,
                          c_x=ES.POSTERIOR_COEF[0], c_n=ES.POSTERIOR_COEF[1])
    return lat, clean


@pytest.mark.parametrize("lead", [GUARD, GUARD + 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("shape", ES.POSTERIOR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_posterior_latents_inside_the_bound(hip, shape, lead):
    """|got - ref| <= gamma(7) S per element of the latents, gamma(5) S' of clean_out (edit_spec.K_LATENTS, K_CLEAN: expf charged its documented ulp), over every
    combination of noise_post / noise_add / clean_out handed over or not, log-variances on both sides of the clamp; clean_out stays NaN when it is not handed over"""
    worst = dict(latents=0.0, clean=0.0)
    for var in ES.POSTERIOR_VARIANTS:
        ref = ES.posterior_reference(shape, var)
        lat, clean = launch_posterior(hip, shape, var, lead)
        worst["latents"] = max(worst["latents"], judge(lat, *ref["latents"], f"posterior_latents latents {shape} {var}"))
        if var.clean:
            worst["clean"] = max(worst["clean"], judge(clean, *ref["clean"], f"posterior_latents clean_out {shape} {var}"))
        else:
            assert untouched(clean), var
    assert len(ES.POSTERIOR_VARIANTS) == 8
    print(f"posterior_latents {shape} lead {lead}: worst element at {worst['latents']:.3f} x its bound, clean_out at {worst['clean']:.3f} x")


@pytest.mark.parametrize("shape", ES.POSTERIOR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_posterior_latents_bit_level_properties(hip, shape):
    C = shape[1]
    for var in ES.POSTERIOR_VARIANTS:
        a, b = launch_posterior(hip, shape, var), launch_posterior(hip, shape, var)
        torch.cuda.synchronize()
        assert torch.equal(KC._bits(a[0].buf), KC._bits(b[0].buf)) and torch.equal(KC._bits(a[1].buf), KC._bits(b[1].buf)), var      # the same call: the same bits
        u = launch_posterior(hip, shape, var, lead=GUARD + 1)             # the scalar path gives the bits of the 16-byte path
        torch.cuda.synchronize()
        assert torch.equal(KC._bits(u[0].t), KC._bits(a[0].t)) and torch.equal(KC._bits(u[1].t), KC._bits(a[1].t)), var
        if not var.post:      # the mode does not load the log-variance: NaN there changes nothing
            m = ES.posterior_operands(shape)["moments"].clone()
            m[:, C:] = float("nan")
            c = launch_posterior(hip, shape, var, moments=m)
            torch.cuda.synchronize()
            assert torch.isfinite(c[0].t).all() and torch.equal(KC._bits(c[0].buf), KC._bits(a[0].buf)), var
    o = ES.posterior_operands(shape)
    with pytest.raises(Exception, match="aliases"):
        x = dev(o["noise_add"])
        hip.posterior_latents(dev(o["moments"]), x, noise_add=x, scale=ES.VAE_SCALE)


# ---- fyc_inpaint_prepare -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ES.PREPARE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_inpaint_prepare_is_exact(hip, shape):
    """both outputs bit for bit the specification's (no rounding on the path), mask values exactly 0, 0.5, 1 and the f32 neighbours of 0.5, nothing outside the outputs
    written; an output that is not handed over stays NaN, the image is not read without the masked output, the same call gives the same bits"""
    N, H, Wd = shape
    o = ES.prepare_operands(shape)
    ref_masked, ref_lat = ES.inpaint_prepare(o["image"], o["mask"])
    image, mask = dev(o["image"]), dev(o["mask"])
    runs = []
    for want_masked, want_lat in ((True, True), (True, False), (False, True), (True, True)):
        masked, lat = Guarded((N, 3, H, Wd)), Guarded((N, 1, H // 8, Wd // 8))
        nan_image = torch.full_like(image, float("nan"))
        hip.inpaint_prepare(image if want_masked else nan_image, mask, masked=masked.t if want_masked else None, mask_latent=lat.t if want_lat else None)
        torch.cuda.synchronize()
        for out, ref, want in ((masked, ref_masked, want_masked), (lat, ref_lat, want_lat)):
            if want:
                assert torch.equal(KC._bits(out.t), KC._bits(ref)), (shape, want_masked, want_lat)
                assert torch.equal(KC._bits(out.buf)[~out.mask], KC._bits(out.before)[~out.mask]), "written outside the output"
            else:
                assert untouched(out)
        runs.append((masked, lat))
    assert torch.equal(KC._bits(runs[0][0].buf), KC._bits(runs[3][0].buf)) and torch.equal(KC._bits(runs[0][1].buf), KC._bits(runs[3][1].buf))
    with pytest.raises(Exception, match="neither output"):
        hip.inpaint_prepare(image, mask)


# ---- fyc_renoise_blend ---------------------------------------------------------------------------------------------------------------------------------------
def launch_blend(hip, shape, full, lead=GUARD):
    B, C, F, HW = shape
    o = ES.blend_operands(shape, full)
    lat = Guarded(shape, o["latents"], lead)
    hip.renoise_blend(lat.t, dev(o["orig"], lead), dev(o["noise"], lead), dev(o["mask"], lead), c_x=ES.BLEND_COEF[0], c_n=ES.BLEND_COEF[1], B=B, C_=C, F=F, HW=HW)
    return lat


@pytest.mark.parametrize("full", [False, True], ids=["per_clip", "per_frame"])
@pytest.mark.parametrize("shape", ES.BLEND_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_renoise_blend_inside_the_bound(hip, shape, full):
    """|got - ref| <= gamma(4) S per element (edit_spec.K_BLEND) on the project's step-kernel shapes, original and noise per clip (B, C, HW) or per frame; where the mask
    is exactly 0 the latents keep their bits; the same call gives the same bits, on the 16-byte and on the scalar path"""
    B, C, F, HW = shape
    ref, bound = ES.blend_reference(shape, full)
    lat = launch_blend(hip, shape, full)
    worst = judge(lat, ref, bound, f"renoise_blend {shape} full={full}")
    o = ES.blend_operands(shape, full)
    m = o["mask"].reshape(B, 1, 1, HW).expand(B, C, F, HW)
    got = lat.t.cpu()
    assert torch.equal(got[m == 0], o["latents"][m == 0])
    again, scalar = launch_blend(hip, shape, full), launch_blend(hip, shape, full, lead=GUARD + 1)
    torch.cuda.synchronize()
    assert torch.equal(KC._bits(again.buf), KC._bits(lat.buf)) and torch.equal(KC._bits(scalar.t), KC._bits(lat.t))
    print(f"renoise_blend {shape} full={full}: worst element at {worst:.3f} x its bound")


# ---- the pipelines -------------------------------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("case", [ES.Case("img2img", "lms", ES.STRENGTH, 0.0), ES.Case("inpaint", "euler", None, 0.0), ES.Case("legacy", "plms", ES.STRENGTH, 0.0)],
                         ids=ES.case_key)
def test_pipeline_against_the_emulator(hip, golden, dropin, monkeypatch, case):
    """the drop-in pipeline on the MI355X in f32 against the same call on the emulator: per-evaluation rel-L2 < 1e-3, the margin of tests/test_pndm_gpu.py's
    sampler-against-emulator run; the same timesteps, callbacks and noise"""
    from followyourclick_amd import ops as ops_mod
    with monkeypatch.context() as m:
        m.setattr(ops_mod, "impl", EditEmuOps())
        ref = EP.run_case(case, golden, EP.build_pipeline(case, EP.build_models(golden)), monkeypatch)
    assert ops_mod.get().name == "hip"
    got = EP.run_case(case, golden, EP.build_pipeline(case, EP.build_models(golden, torch.float32, DEV), DEV), monkeypatch)
    assert got.timesteps == ref.timesteps and got.callbacks == ref.callbacks and len(got.drawn) == len(ref.drawn)
    assert all(torch.equal(a, b) for a, b in zip(got.drawn, ref.drawn))
    err = (got.traj - ref.traj).flatten(1).norm(dim=1) / ref.traj.flatten(1).norm(dim=1)
    print(f"{ES.case_key(case)} f32 against the emulator: per-evaluation rel-L2 {[f'{e:.2e}' for e in err.tolist()]}")
    assert torch.isfinite(got.traj).all() and err.max().item() < 1e-3, err


# per-evaluation rel-L2 of the latents / rel-L2 of the images (the metric of tests/test_dropin_gpu.py::test_stable_diffusion_pipeline_call, whose margins these are: in
# bf16 the largest single pixel error is one rounding of the decoder's output).  f32: 5e-4, the bound tests/test_sigma_gpu.py and tests/test_pndm_gpu.py hold
# pipeline_tiny_* to, and the 2e-3 of the sd2d_pipeline images; bf16: 1e-1 / 6e-2, what that test holds the 2-D pipeline of this very tiny model to; f16 has three
# more fraction bits than bf16, so an eighth of its margins
MARGINS = {"f32": (torch.float32, 5e-4, 2e-3), "bf16": (torch.bfloat16, 1e-1, 6e-2), "f16": (torch.float16, 1e-1 / 8, 6e-2 / 8)}


@pytest.mark.parametrize("dt", list(MARGINS))
@pytest.mark.parametrize("case", [ES.Case("img2img", "euler_a", ES.STRENGTH, 0.0), ES.Case("inpaint", "plms", None, 0.0), ES.Case("legacy", "ddim", ES.STRENGTH, 0.0)],
                         ids=ES.case_key)
def test_pipeline_against_the_reference_run(hip, golden, dropin, monkeypatch, case, dt):
    dtype, tol_lat, tol_img = MARGINS[dt]
    key = ES.case_key(case)
    run = EP.run_case(case, golden, EP.build_pipeline(case, EP.build_models(golden, dtype, DEV), DEV), monkeypatch)
    assert run.timesteps == golden[f"{key}/timesteps"].tolist() and run.callbacks == golden[f"{key}/callbacks"].tolist()
    err = EP.trajectory_error(run, golden, case)
    ref = golden[f"{key}/images"]
    img = ((run.images - ref).norm() / ref.norm()).item()
    print(f"{key} {dt} against the reference: per-evaluation rel-L2 {[f'{e:.2e}' for e in err.tolist()]}, images rel-L2 {img:.2e}, max abs {(run.images - ref).abs().max().item():.2e}")
    assert err.max().item() < tol_lat, err
    assert img < tol_img
