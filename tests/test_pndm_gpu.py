"""fyc_cfg_pndm_step on the MI355X: every element of the latents, hist_out and acc_out against the f64 specification (tests/pndm_spec.py) inside the bound derived
there and sample_out as an exact copy, the buffers a variant does not read left alone and the outputs it is not handed left unwritten, the same bits on every call,
the sampler in both modes against the same run on the emulator (tests/emu_ops_pndm.py) and the reference pipeline's trajectories."""
import os

import numpy as np
import pytest
import torch

import pndm_spec as SP
from emu_ops_pndm import PNDMEmuOps
from followyourclick_amd.engine import PNDMConfig, UNet3DConfig
from followyourclick_amd.engine.sampler import PNDMSampler
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
    """one launch on device copies of the shared operands -> {lat, hist, sample, acc} [B c_latent][F HW] on the host"""
    out = SP.run_step(hip, shape, dt, var, on=lambda t: t.to(DEV), **kw)
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in out.items()}


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape", SP.SHAPES, ids=IDS)
def test_kernel_inside_the_bound_of_the_specification(hip, shape, dt):
    """|got - ref| <= gamma(11) S per element of the new latents, gamma(6) S' per element of hist_out - the guided prediction -, gamma(8) S'' per element of acc_out (the
    roundings on the kernel's longest paths with the coefficient row taken as given, counted beside pndm_spec.K_KERNEL_GIVEN), sample_out the latents' bits as they were,
    over orders 1..4 x with / without sample_in x accumulator none / write / read-write / in place x with / without pred_single x guidance_rescale 0 / 0.7.  The pad
    channels hold 1e4: a pass that counts them is far outside."""
    worst = dict(lat=0.0, hist=0.0, acc=0.0)
    before = SP.operands(shape, dt)["latents"].reshape(shape[0] * shape[3], -1)
    for var in SP.VARIANTS:
        ref, got = SP.reference(shape, dt, var), launch(hip, shape, dt, var)
        for k, (val, bound) in ref.items():
            worst[k] = max(worst[k], SP.inside(got[k], val, bound, f"cfg_pndm_step {k} {shape} {dt} {var}"))
        assert torch.equal(got["sample"], before), var
        assert var.acc != "none" or bool(torch.isnan(got["acc"]).all()), var
    assert len(SP.VARIANTS) == 128
    print(f"cfg_pndm_step {shape} {dt}: worst element at {worst['lat']:.3f} x its bound, hist_out at {worst['hist']:.3f} x, acc_out at {worst['acc']:.3f} x, over {len(SP.VARIANTS)} variants")


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape", SP.SHAPES, ids=IDS)
def test_bit_level_properties(hip, shape, dt):
    B, F, HW, CL, ld = shape
    nan = torch.full((B, CL, F, HW), float("nan"))
    o = SP.operands(shape, dt)
    for order in SP.ORDERS:
        for sample_in in (False, True):
            # the histories the order does not read are handed over full of NaN, acc_in is NULL, and with sample_in (and no sample_out, which would copy them) the
            # latents are NaN too: never loaded
            var = SP.Variant(order, sample_in, "write", False, 0.0)
            got = launch(hip, shape, dt, var)
            hs = [o[f"hist_{k}"] if order > k else nan for k in (1, 2, 3)]
            got2 = launch(hip, shape, dt, var, hist=hs, latents=nan if sample_in else None, save=not sample_in)
            assert torch.isfinite(got2["lat"]).all() and torch.equal(got2["lat"], got["lat"]) and torch.equal(got2["hist"], got["hist"]), (order, sample_in)
            assert torch.isfinite(got2["acc"]).all() and torch.equal(got2["acc"], got["acc"])
            # outputs not handed over: nothing is stored (the buffers this helper returns stay NaN), the latents are the same bits
            got3 = launch(hip, shape, dt, var._replace(acc="none"), store=False)
            assert torch.equal(got3["lat"], got["lat"]) and all(bool(torch.isnan(got3[k]).all()) for k in ("hist", "sample", "acc")), (order, sample_in)
    # acc_in == acc_out gives the bits of acc_in != acc_out
    for order in (1, 4):
        a, b = launch(hip, shape, dt, SP.Variant(order, True, "read_write", True, 0.7)), launch(hip, shape, dt, SP.Variant(order, True, "in_place", True, 0.7))
        assert all(torch.equal(a[k], b[k]) for k in SP.OUTPUTS)
    # the longest variant: fourth order, a saved sample, the accumulator in place, pred_single, guidance rescale
    var = SP.Variant(4, True, "in_place", True, 0.7)
    first, again = launch(hip, shape, dt, var), launch(hip, shape, dt, var)
    assert all(torch.equal(first[k], again[k]) for k in SP.OUTPUTS)                       # the same call twice: the same bits
    assert not torch.equal(first["lat"], launch(hip, shape, dt, var._replace(sample_in=False))["lat"])
    # nothing is read from the workspace before it is written
    assert hip._rescale_ws is not None and hip._rescale_ws.numel() >= B * ((F * HW + 1023) // 1024) * 32 + 4 * B
    hip._rescale_ws.fill_(0xFF)
    assert torch.equal(launch(hip, shape, dt, var)["lat"], first["lat"])
    # the pad columns of pred are ignored: other values there, the same bits
    pred = o["pred"].clone()
    pred[:, CL:] = -3.0e4
    padded = launch(hip, shape, dt, var, pred=pred)
    assert all(torch.equal(padded[k], first[k]) for k in SP.OUTPUTS)


def tiny_cfg():
    return UNet3DConfig(block_out_channels=(64, 128, 256, 256), cross_attention_dim=64, sample_size=8)


@pytest.mark.parametrize("mode", SP.MODES)
def test_pndm_sampler_against_the_emulator(mode):
    """the tiny engine of tests/test_engine_gpu.py, f32, 5 steps (6 / 14 evaluations) on the zero-SNR table with v_prediction and guidance_rescale 0.7, against the same
    run on the emulator under the rel-L2 bound of that file's f32 sampler test (1e-3 per evaluation)"""
    sd = W.make_weights(W.unet_state_shapes(Fn.tiny_unet_config()), 0)
    inp = W.seeded_inputs(Fn.tiny_unet_config(), 1, 4, 8, 8, seed=7)
    pcfg = PNDMConfig(skip_prk_steps=mode == "plms", steps_offset=1, rescale_betas_zero_snr=True, **YAML)

    def run(eng):
        smp, traj = PNDMSampler(eng, pcfg), []
        lat = inp["latents"].to(eng.device, torch.float32).contiguous().clone()
        first = inp["first_image_latents"].to(eng.device, torch.float32).reshape(1, 4, 64).contiguous()
        mask = inp["first_images_mask"].to(eng.device, torch.float32)[:, :, 0].reshape(1, 1, 64).contiguous()
        st = smp.prepare(inp["text"], 5, 1, 8.0, [2], [4], guidance_rescale=0.7)
        for i in range(len(st["timesteps"])):
            smp.step(st, i, lat, first, mask, guidance_rescale=0.7)
            traj.append(lat.detach().cpu().clone())
        return torch.stack(traj)
    ref = run(UNet3DEngine(pack_unet(sd, tiny_cfg(), torch.float32, "cpu"), ops=PNDMEmuOps()))
    eng = UNet3DEngine(pack_unet(sd, tiny_cfg(), torch.float32, DEV))
    assert eng.ops.name == "hip" and len(ref) == (6 if mode == "plms" else 14)
    got = run(eng)
    err = (got - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)
    print(f"PNDM {mode} + guidance rescale, f32: per-evaluation rel-L2 vs the emulator {[f'{e:.2e}' for e in err.tolist()]}")
    assert torch.isfinite(got).all() and err.max().item() < 1e-3, err


@pytest.mark.parametrize("mode", SP.MODES)
def test_pipeline_trajectory_matches_the_reference(golden_dir, mode):
    """the reference AnimationPipeline's 5-step run with its own PNDMScheduler (tests/golden/pipeline_tiny_pndm.npz) in f32: per-evaluation rel-L2 < 5e-4, the bound of
    the DDIM and sigma runs of the same model"""
    g = {k: torch.from_numpy(v) if v.shape else v for k, v in np.load(os.path.join(golden_dir, "pipeline_tiny_pndm.npz")).items()}
    sd = W.make_weights(W.unet_state_shapes(Fn.tiny_unet_config()), int(g["unet_weight_seed"]))
    eng = UNet3DEngine(pack_unet(sd, tiny_cfg(), torch.float32, DEV))
    traj, seen = [], []
    lat = PNDMSampler(eng, PNDMConfig(skip_prk_steps=mode == "plms", steps_offset=1, **YAML)).sample(
        g["latents"], g["text_embeddings"], 5, 8.0, g["first_image_latents"], g["first_images_mask"], fps=[2], flow=[4],
        callback=lambda i, t, l: (traj.append(l.detach().cpu().clone()), seen.append(t)))
    assert lat.dtype == torch.float32 and seen == g[f"timesteps_{mode}"].tolist()
    ref = g[f"trajectory_{mode}"]
    err = (torch.stack(traj) - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)
    print(f"PNDM {mode} f32 pipeline trajectory: per-evaluation rel-L2 vs the reference {[f'{e:.2e}' for e in err.tolist()]}")
    assert err.max().item() < 5e-4, err
