"""fyc_cfg_solver_step on the MI355X: every element against the f64 specification (tests/solver_spec.py) inside the bound derived there, the histories an order does
not read left alone, the same bits on every call, guidance_rescale = 0 as the un-rescaled launch, the first zero-terminal-SNR step, and the multistep sampler against
the same run on the emulator (tests/emu_ops_solver.py)."""
import pytest
import torch

import solver_spec as SP
from emu_ops_solver import SolverEmuOps
from followyourclick_amd.engine import SolverConfig, UNet3DConfig
from followyourclick_amd.engine.sampler import SolverSampler
from followyourclick_amd.engine.scheduler import SolverTables
from followyourclick_amd.engine.unet3d import UNet3DEngine
from followyourclick_amd.engine.weights import pack_unet
from oracle import functional as Fn
from oracle import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = ["x".join(map(str, s)) for s in SP.SHAPES]


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
    """|got - ref| <= ((1 + 2^-24)^14 - 1) S per element of the new latents, ((1 + 2^-24)^9 - 1) S' per element of hist_out (the roundings on the kernel's longest
    paths, counted beside solver_spec.K_KERNEL / K_M0).  The pad channels hold 1e4: a pass that counts them is far outside.  The histories an order does not read
    are handed over full of NaN: the result is finite and the same bits as with finite ones."""
    nan = torch.full((shape[0], shape[3], shape[1], shape[2]), float("nan"))
    o = SP.operands(shape, dt)
    worst = worst_m0 = 0.0
    for var in SP.VARIANTS:
        ref, bound, m0, m0_bound = SP.reference(shape, dt, var)
        lat, out = launch(hip, shape, dt, var)
        worst = max(worst, SP.inside(lat, ref, bound, f"cfg_solver_step {shape} {dt} {var}"))
        worst_m0 = max(worst_m0, SP.inside(out, m0, m0_bound, f"cfg_solver_step hist_out {shape} {dt} {var}"))
        if var.order < 3:
            lat2, out2 = launch(hip, shape, dt, var, hist=(o["hist_1"] if var.order == 2 else nan, nan))
            assert torch.isfinite(lat2).all() and torch.equal(lat2, lat) and torch.equal(out2, out), var
    print(f"cfg_solver_step {shape} {dt}: worst element at {worst:.3f} x its bound, hist_out at {worst_m0:.3f} x, over {len(SP.VARIANTS)} variants")


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape", SP.SHAPES, ids=IDS)
def test_bit_level_properties(hip, shape, dt):
    B, F, HW, CL, ld = shape
    var = SP.Variant(3, True, 0.7, "v_prediction")
    first = launch(hip, shape, dt, var)
    again = launch(hip, shape, dt, var)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])          # the same call twice: the same bits
    # nothing is read from the workspace before it is written
    assert hip._rescale_ws is not None and hip._rescale_ws.numel() >= B * ((F * HW + 1023) // 1024) * 32 + 4 * B
    hip._rescale_ws.fill_(0xFF)
    assert torch.equal(launch(hip, shape, dt, var)[0], first[0])
    # guidance_rescale = 0 launches no moments pass (the workspace keeps what it held) and is the un-rescaled call bit for bit
    plain_var = var._replace(phi=0.0)
    plain = launch(hip, shape, dt, plain_var)
    hip._rescale_ws.fill_(0x5A)
    zero = launch(hip, shape, dt, var, phi=0.0)
    assert bool((hip._rescale_ws == 0x5A).all())
    assert torch.equal(zero[0], plain[0]) and torch.equal(zero[1], plain[1]) and not torch.equal(plain[0], first[0])


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_first_zero_snr_step(hip, dt):
    """the coefficients SolverTables gives the first step of a zero-terminal-SNR table (t = 999, lambda = -inf): x' = sigma_prev x + alpha_prev x0, finite"""
    shape, var = SP.SHAPES[1], SP.Variant(1, False, 0.7, "v_prediction")
    tb = SolverTables(SolverConfig(**SP.BETAS, rescale_betas_zero_snr=True, prediction_type="v_prediction"))
    assert tb.timesteps(10)[0].item() == 999 and tb.plan(10)[0] == 1
    coef = tb.coefficient_table(10)[0]
    assert coef[:2].tolist() == [0.0, -1.0] and coef[4:].tolist() == [0.0] * 4 and torch.isfinite(coef).all()
    ref, bound, m0, m0_bound = SP.reference(shape, dt, var, coef=coef)
    lat, out = launch(hip, shape, dt, var, coef=coef)
    SP.inside(lat, ref, bound, f"first zero-SNR step {dt}")
    SP.inside(out, m0, m0_bound, f"first zero-SNR step hist_out {dt}")


def test_solver_sampler_against_the_emulator():
    """the tiny engine of tests/test_engine_gpu.py, f32, 4 steps of DPM-Solver++(2M) on the zero-SNR betas with v_prediction and guidance_rescale 0.7, against the
    same run on the emulator under the rel-L2 bound of that file's f32 sampler test (1e-3 per step)"""
    ocfg = Fn.tiny_unet_config()
    cfg = UNet3DConfig(block_out_channels=(64, 128, 256, 256), cross_attention_dim=64, sample_size=8)
    sd = W.make_weights(W.unet_state_shapes(ocfg), 0)
    inp = W.seeded_inputs(ocfg, 1, 4, 8, 8, seed=7)
    scfg = SolverConfig(**SP.BETAS, rescale_betas_zero_snr=True, prediction_type="v_prediction", solver_order=2)

    def run(eng):
        traj = []
        SolverSampler(eng, scfg).sample(inp["latents"], inp["text"], 4, 8.0, inp["first_image_latents"], inp["first_images_mask"], fps=[2], flow=[4],
                                        callback=lambda i, t, l: traj.append(l.detach().cpu().clone()), guidance_rescale=0.7)
        return torch.stack(traj)
    ref = run(UNet3DEngine(pack_unet(sd, cfg, torch.float32, "cpu"), ops=SolverEmuOps()))
    eng = UNet3DEngine(pack_unet(sd, cfg, torch.float32, DEV))
    assert eng.ops.name == "hip"
    got = run(eng)
    err = (got - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)
    print(f"DPM-Solver++(2M) + guidance rescale, f32: per-step rel-L2 vs the emulator {[f'{e:.2e}' for e in err.tolist()]}")
    assert torch.isfinite(got).all() and err.max().item() < 1e-3, err
