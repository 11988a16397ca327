"""fyc_cfg_ddim_step_rescaled on the MI355X: every element against the f64 specification (tests/sampling_spec.py) inside the bound derived there, the bit-level
properties of the two-pass reduction (same bits on every call, nothing read from the workspace before it is written, guidance_rescale = 0 and a factor of exactly 1
are the plain step), the first trailing step at alphas_cumprod = 0, and the sampler against the same run on the emulator (tests/emu_ops_sampling.py)."""
import pytest
import torch

import kernel_compare as KC
import sampling_spec as SS
from emu_ops_sampling import SamplingEmuOps
from followyourclick_amd.engine import DDIMConfig, UNet3DConfig
from followyourclick_amd.engine.sampler import DDIMSampler
from followyourclick_amd.engine.unet3d import UNet3DEngine
from followyourclick_amd.engine.weights import pack_unet
from kernel_compare import compare
from oracle import functional as Fn
from oracle import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
def labels(shape):
    return KC.Labels(row=lambda i: f"sample {i // shape[3]}, channel {i % shape[3]}", col=lambda j: f"frame-pixel {j}")
IDS = ["x".join(map(str, s)) for s in SS.SHAPES]


@pytest.fixture(scope="module")
def hip():
    from followyourclick_amd import ops
    return ops.get()


def launch(hip, shape, dt, var, *, phi=None, pred=None, coef=None, rescaled=True):
    """one launch on device copies of the shared operands -> the latents (B, c_latent, F, HW) on the host"""
    o = SS.operands(shape, dt)
    lat = o["latents"].clone().to(DEV)
    kw = dict(pred_single=o["single"].to(DEV) if var.single else None, variance_noise=o["noise"].to(DEV) if var.noise else None, **SS.step_kwargs(shape, var))
    args = ((o["pred"] if pred is None else pred).to(DEV), lat, (o["coef"] if coef is None else coef).to(DEV))
    if rescaled:
        hip.cfg_ddim_step_rescaled(*args, guidance_rescale=var.phi if phi is None else phi, **kw)
    else:
        hip.cfg_ddim_step(*args, **kw)
    torch.cuda.synchronize()
    return lat.cpu()


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape", SS.SHAPES, ids=IDS)
def test_kernel_inside_the_bound_of_the_specification(hip, shape, dt):
    """|got - ref| <= ((1 + 2^-24)^15 - 1) S per element, S the sum of the absolute values of all terms of the step (sampling_spec.guided_step; 15 = the f32 roundings
    on the kernel's longest path, counted beside K_ROUNDINGS, the one of the factor included).  The pad channels hold 1e4: a pass that counts them is far outside."""
    B, F, HW, CL, ld = shape
    worst = 0.0
    for var in SS.VARIANTS:
        ref, bound = SS.reference(shape, dt, var)
        fig = compare(launch(hip, shape, dt, var).reshape(B * CL, F * HW), ref, dtype="f32", bound=bound, rtol=KC.RTOL["f32"], labels=labels(shape),
                      tag=f"cfg_ddim_step_rescaled {shape} {dt} {var}")
        worst = max(worst, fig["elem_ratio"])
    print(f"cfg_ddim_step_rescaled {shape} {dt}: worst element at {worst:.3f} x its bound over {len(SS.VARIANTS)} variants")


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape", SS.SHAPES, ids=IDS)
def test_bit_level_properties(hip, shape, dt):
    B, F, HW, CL, ld = shape
    var = SS.Variant(1, 0.7, True, True, False)
    # guidance_rescale = 0: fyc_cfg_ddim_step, call for call
    plain = launch(hip, shape, dt, var, rescaled=False)
    assert torch.equal(launch(hip, shape, dt, var, phi=0.0), plain)
    # the same call twice: the same bits (fixed runs of rows per block, a fixed tree in the block, partials folded in index order)
    first = launch(hip, shape, dt, var)
    assert torch.equal(launch(hip, shape, dt, var), first) and not torch.equal(first, plain)
    # nothing is read from the workspace before it is written
    assert hip._rescale_ws is not None and hip._rescale_ws.numel() >= B * ((F * HW + 1023) // 1024) * 32 + 4 * B
    hip._rescale_ws.fill_(0xFF)
    assert torch.equal(launch(hip, shape, dt, var), first)
    hip._rescale_ws.zero_()
    assert torch.equal(launch(hip, shape, dt, var), first)


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_uniform_sample_keeps_the_factor_one(hip, dt):
    """sample 0 gets c == u: v == c value for value, the two variances are the same number and the factor is exactly 1 - that sample is the plain step bit for bit,
    the other sample is not"""
    shape, var = SS.SHAPES[2], SS.Variant(1, 0.7, False, False, False)
    B, F, HW, CL, ld = shape
    pred = SS.operands(shape, dt)["pred"].clone().reshape(2, B, F * HW, ld)
    pred[1, 0] = pred[0, 0]
    pred = pred.reshape(-1, ld)
    got, plain = launch(hip, shape, dt, var, pred=pred), launch(hip, shape, dt, var, pred=pred, rescaled=False)
    assert torch.equal(got[0], plain[0]) and not torch.equal(got[1], plain[1])


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_first_trailing_step(hip, dt):
    """coef = (0, 1, sap, sbp), what the trailing spacing gives a zero-terminal-SNR table at t = 999: v_prediction holds without a division"""
    from followyourclick_amd.engine.scheduler import DDIMTables
    shape, var = SS.SHAPES[1], SS.Variant(1, 0.7, False, False, False)
    B, F, HW, CL, ld = shape
    c = DDIMTables(DDIMConfig(timestep_spacing="trailing")).step_coefficients(999, 25)
    assert c[0] == 0.0 and c[1] == 1.0
    coef = torch.tensor(c[:4], dtype=torch.float32)
    o, kw = SS.operands(shape, dt), SS.step_kwargs(shape, var)
    del kw["cfg"]
    ref, bound, _ = SS.guided_step(o["pred"], o["latents"], coef, guidance_rescale=0.7, **kw)
    got = launch(hip, shape, dt, var, coef=coef)
    assert torch.isfinite(got).all()
    compare(got.reshape(B * CL, F * HW), ref.reshape(B * CL, F * HW), dtype="f32", bound=bound.reshape(B * CL, F * HW), rtol=KC.RTOL["f32"], labels=labels(shape),
            tag=f"first trailing step {dt}")


def test_sampler_with_trailing_steps_and_guidance_rescale():
    """the tiny engine of tests/test_engine_gpu.py, f32, 3 trailing steps with guidance_rescale 0.7, against the same run on the emulator under the rel-L2 bound of that
    file's f32 sampler test (1e-3 per step)"""
    ocfg = Fn.tiny_unet_config()
    cfg = UNet3DConfig(block_out_channels=(64, 128, 256, 256), cross_attention_dim=64, sample_size=8)
    sd = W.make_weights(W.unet_state_shapes(ocfg), 0)
    inp = W.seeded_inputs(ocfg, 1, 4, 8, 8, seed=7)

    def run(eng):
        traj = []
        DDIMSampler(eng, DDIMConfig(timestep_spacing="trailing")).sample(
            inp["latents"], inp["text"], 3, 8.0, inp["first_image_latents"], inp["first_images_mask"], fps=[2], flow=[4],
            callback=lambda i, t, l: traj.append(l.detach().cpu().clone()), guidance_rescale=0.7)
        return torch.stack(traj)
    ref = run(UNet3DEngine(pack_unet(sd, cfg, torch.float32, "cpu"), ops=SamplingEmuOps()))
    eng = UNet3DEngine(pack_unet(sd, cfg, torch.float32, DEV))
    assert eng.ops.name == "hip"
    got = run(eng)
    err = (got - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)
    print(f"trailing + guidance rescale, f32: per-step rel-L2 vs the emulator {[f'{e:.2e}' for e in err.tolist()]}")
    assert torch.isfinite(got).all() and err.max().item() < 1e-3, err
