"""fyc_cfg_sigma_step and fyc_unet_input_scaled on the MI355X: every element against the f64 specification (tests/sigma_spec.py) inside the bound derived there,
the buffers a variant does not read left alone, hist_out = NULL storing nothing, the same bits on every call, the scaled UNet input against fyc_unet_input and the
emulator, the three samplers against the same run on the emulator (tests/emu_ops_sigma.py) and the reference pipeline's trajectories."""
import os

import numpy as np
import pytest
import torch

import sigma_spec as SP
from emu_ops_sigma import SigmaEmuOps
from followyourclick_amd.engine import SigmaConfig, UNet3DConfig
from followyourclick_amd.engine.sampler import SigmaSampler
from followyourclick_amd.engine.unet3d import UNet3DEngine
from followyourclick_amd.engine.weights import pack_unet
from oracle import functional as Fn
from oracle import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = ["x".join(map(str, s)) for s in SP.SHAPES]
YAML = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", prediction_type="v_prediction")


@pytest.fixture(scope="module")
def hip():
    from followyourclick_amd import ops
    return ops.get()


def launch(hip, shape, dt, var, **kw):
    """one launch on device copies of the shared operands -> (latents, hist_out) [B c_latent][F HW] on the host"""
    lat, out = SP.run_step(hip, shape, dt, var, on=lambda t: t.to(DEV), **kw)
    torch.cuda.synchronize()
    return lat.cpu(), out.cpu()


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape", SP.SHAPES, ids=IDS)
def test_kernel_inside_the_bound_of_the_specification(hip, shape, dt):
    """|got - ref| <= gamma(16) S per element of the new latents, gamma(9) S' per element of hist_out - the stored derivative d - (the roundings on the kernel's
    longest paths with the coefficient row taken as given, counted beside sigma_spec.K_KERNEL_GIVEN / K_D_GIVEN), over orders 1..4 x with / without noise x with / without pred_single x guidance_rescale 0 / 0.7 x both
    prediction types.  The pad channels hold 1e4: a pass that counts them is far outside."""
    worst = worst_d = 0.0
    for var in SP.VARIANTS:
        ref, bound, d, d_bound = SP.reference(shape, dt, var)
        lat, out = launch(hip, shape, dt, var)
        worst = max(worst, SP.inside(lat, ref, bound, f"cfg_sigma_step {shape} {dt} {var}"))
        worst_d = max(worst_d, SP.inside(out, d, d_bound, f"cfg_sigma_step hist_out {shape} {dt} {var}"))
    print(f"cfg_sigma_step {shape} {dt}: worst element at {worst:.3f} x its bound, hist_out at {worst_d:.3f} x, over {len(SP.VARIANTS)} variants")


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape", SP.SHAPES, ids=IDS)
def test_bit_level_properties(hip, shape, dt):
    B, F, HW, CL, ld = shape
    nan = torch.full((B, CL, F, HW), float("nan"))
    o = SP.operands(shape, dt)
    for order in SP.ORDERS:            # the histories an order does not read are handed over full of NaN, the noise pointer is NULL: never loaded
        var = SP.Variant(order, False, False, 0.0, "v_prediction")
        lat, out = launch(hip, shape, dt, var)
        hs = [o[f"hist_{k}"] if order > k else nan for k in (1, 2, 3)]
        lat2, out2 = launch(hip, shape, dt, var, hist=hs)
        assert torch.isfinite(lat2).all() and torch.equal(lat2, lat) and torch.equal(out2, out), order
        # hist_out = None: nothing is stored (the buffer this helper returns was never handed over and stays NaN), the latents are the same bits
        lat3, out3 = launch(hip, shape, dt, var, store=False)
        assert torch.equal(lat3, lat) and bool(torch.isnan(out3).all())
    # the longest variant: fourth order, noise, pred_single, guidance rescale
    var = SP.Variant(4, True, True, 0.7, "epsilon")
    first, again = launch(hip, shape, dt, var), launch(hip, shape, dt, var)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])          # the same call twice: the same bits
    assert not torch.equal(first[0], launch(hip, shape, dt, var._replace(noise=False))[0])
    # nothing is read from the workspace before it is written
    assert hip._rescale_ws is not None and hip._rescale_ws.numel() >= B * ((F * HW + 1023) // 1024) * 32 + 4 * B
    hip._rescale_ws.fill_(0xFF)
    assert torch.equal(launch(hip, shape, dt, var)[0], first[0])
    # the pad columns of pred are ignored: other values there, the same bits
    pred = o["pred"].clone()
    pred[:, CL:] = -3.0e4
    padded = launch(hip, shape, dt, var, pred=pred)
    assert torch.equal(padded[0], first[0]) and torch.equal(padded[1], first[1])


@pytest.mark.parametrize("case", SP.INPUT_CASES, ids=[f"mode{c.mode}-cond{c.scale_cond}-dup{c.cfg_dup}-mask{int(c.with_mask)}" for c in SP.INPUT_CASES])
def test_unet_input_scaled(hip, case):
    """denom = 1 is fyc_unet_input bit for bit; the f32 output is the emulator's bits (one IEEE division); 16-bit storage within one more rounding of the f64
    reference; the mask and first-frame channels are divided exactly when scale_cond = 1; mode 1 leaves the repeated first-frame latents undivided; pads are 0"""
    emu, on = SigmaEmuOps(), (lambda t: t.to(DEV))
    for shape in SP.INPUT_SHAPES:
        B, F, HW, CL, cp = shape
        ref = SP.input_reference(shape, case, SP.INPUT_DENOM)
        for dtype, u in ((torch.float32, 0.0), (torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)):
            got = SP.run_input(hip, shape, case, dtype, SP.INPUT_DENOM, on=on).cpu()
            one, plain = SP.run_input(hip, shape, case, dtype, 1.0, on=on).cpu(), SP.run_input(hip, shape, case, dtype, 1.0, on=on, scaled=False).cpu()
            assert torch.equal(one, plain) and not torch.isnan(got).any(), (shape, dtype)
            assert torch.equal(got, SP.run_input(emu, shape, case, dtype, SP.INPUT_DENOM)), (shape, dtype)
            assert ((got.double() - ref).abs() <= (2.0 ** -24 + u) * ref.abs() + 2.0 ** -140).all(), (shape, dtype)
            first_cols = slice(CL, 2 * CL) if case.mode == 1 else slice(CL, 2 * CL + 1)
            assert not got[..., first_cols.stop:].any()                                                    # pads
            same = torch.equal(got[..., first_cols], plain[..., first_cols])                               # the conditioning channels against the unscaled build
            assert same == (not case.scale_cond), (shape, dtype)
            assert not torch.equal(got[..., :CL], plain[..., :CL])                                         # the latents are always divided
        if case.mode == 1:
            f32 = SP.run_input(hip, shape, case, torch.float32, SP.INPUT_DENOM, on=on).cpu().reshape(case.cfg_dup, B, F, HW, cp)
            want = SP.input_operands(shape)["first"].reshape(B, 1, CL, HW).permute(0, 1, 3, 2).expand(B, F, HW, CL)
            assert all(torch.equal(f32[d, ..., CL:2 * CL], want) for d in range(case.cfg_dup))


def tiny_cfg():
    return UNet3DConfig(block_out_channels=(64, 128, 256, 256), cross_attention_dim=64, sample_size=8)


@pytest.mark.parametrize("kind", SP.KINDS)
def test_sigma_sampler_against_the_emulator(kind):
    """the tiny engine of tests/test_engine_gpu.py, f32, 5 steps on the zero-SNR table with v_prediction and guidance_rescale 0.7, against the same run on the
    emulator under the rel-L2 bound of that file's f32 sampler test (1e-3 per step).  The ancestral noise is drawn on the host and is the same in both runs."""
    sd = W.make_weights(W.unet_state_shapes(Fn.tiny_unet_config()), 0)
    inp = W.seeded_inputs(Fn.tiny_unet_config(), 1, 4, 8, 8, seed=7)
    scfg = SigmaConfig(kind=kind, rescale_betas_zero_snr=True, **YAML)

    def run(eng):
        smp, traj = SigmaSampler(eng, scfg), []
        lat = (inp["latents"] * smp.tables.init_noise_sigma).to(eng.device)
        first = inp["first_image_latents"].to(eng.device, torch.float32).reshape(1, 4, 64).contiguous()
        mask = inp["first_images_mask"].to(eng.device, torch.float32)[:, :, 0].reshape(1, 1, 64).contiguous()
        st = smp.prepare(inp["text"], 5, 1, 8.0, [2], [4], guidance_rescale=0.7)
        g = torch.Generator().manual_seed(5)
        for i in range(5):
            noise = torch.randn(lat.shape, generator=g).to(eng.device) if kind == "euler_ancestral" else None
            smp.step(st, i, lat, first, mask, variance_noise=noise, guidance_rescale=0.7)
            traj.append(lat.detach().cpu().clone())
        return torch.stack(traj)
    ref = run(UNet3DEngine(pack_unet(sd, tiny_cfg(), torch.float32, "cpu"), ops=SigmaEmuOps()))
    eng = UNet3DEngine(pack_unet(sd, tiny_cfg(), torch.float32, DEV))
    assert eng.ops.name == "hip"
    got = run(eng)
    err = (got - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)
    print(f"{kind} + guidance rescale, f32: per-step rel-L2 vs the emulator {[f'{e:.2e}' for e in err.tolist()]}")
    assert torch.isfinite(got).all() and err.max().item() < 1e-3, err


def test_plain_input_with_the_reciprocal(hip):
    """the 2-D path: nchw_to_nhwc(scale = the f32 reciprocal) against latents / denom, inside the two roundings of sigma_spec.K_PLAIN_INPUT plus the storage type's,
    and the emulator's bits in f32"""
    for shape in SP.INPUT_SHAPES:
        ref = SP.plain_input_reference(shape, SP.INPUT_DENOM)
        for dtype, u in ((torch.float32, 0.0), (torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)):
            got = SP.run_plain_input(hip, shape, dtype, SP.INPUT_DENOM, on=lambda t: t.to(DEV)).cpu()
            assert ((got.double() - ref).abs() <= (SP.gamma(SP.K_PLAIN_INPUT) + u) * ref.abs() + 2.0 ** -140).all(), (shape, dtype)
            assert not got[..., shape[3]:].any()
            if dtype == torch.float32:
                assert torch.equal(got, SP.run_plain_input(SigmaEmuOps(), shape, dtype, SP.INPUT_DENOM))


@pytest.mark.parametrize("kind", SP.KINDS)
def test_pipeline_trajectory_matches_the_reference(golden_dir, kind):
    """the reference AnimationPipeline's 5-step run with its own scheduler class (tests/golden/pipeline_tiny_sigma.npz) in f32: per-step rel-L2 < 5e-4, the bound of
    the DDIM run of the same model.  The clip is driven through prepare and step: the golden run was handed its latents, so its generator served the step noise
    alone, and the ancestral kind's noise is that host stream, drawn here from a host generator with the golden's seed and moved to the device."""
    g = {k: torch.from_numpy(v) if v.shape else v for k, v in np.load(os.path.join(golden_dir, "pipeline_tiny_sigma.npz")).items()}
    sd = W.make_weights(W.unet_state_shapes(Fn.tiny_unet_config()), int(g["unet_weight_seed"]))
    eng = UNet3DEngine(pack_unet(sd, tiny_cfg(), torch.float32, DEV))
    smp, traj = SigmaSampler(eng, SigmaConfig(kind=kind, **YAML)), []
    lat = (g["latents"] * float(g["init_noise_sigma"])).to(DEV).contiguous()
    first = g["first_image_latents"].to(DEV, torch.float32).reshape(1, 4, 64).contiguous()
    mask = g["first_images_mask"].to(DEV, torch.float32)[:, :, 0].reshape(1, 1, 64).contiguous()
    st = smp.prepare(g["text_embeddings"], 5, 1, 8.0, [2], [4])
    gen = torch.Generator().manual_seed(int(g["generator_seed"]))
    for i in range(5):
        noise = torch.randn(lat.shape, generator=gen).to(DEV) if kind == "euler_ancestral" else None
        smp.step(st, i, lat, first, mask, variance_noise=noise)
        traj.append(lat.detach().cpu().clone())
    ref = g[f"trajectory_{kind}"]
    err = (torch.stack(traj) - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)
    print(f"{kind} f32 pipeline trajectory: per-step rel-L2 vs the reference {[f'{e:.2e}' for e in err.tolist()]}")
    assert err.max().item() < 5e-4, err
