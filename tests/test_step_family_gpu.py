"""fyc_cfg_solver_step, fyc_cfg_sigma_step and fyc_cfg_pndm_step on the MI355X are one kernel: where include/fyc.h gives two of them the same expression,
summed in the same order, they give the same bits.  Nothing here is measured against a tolerance or a recorded value - the per-element judgement against the f64
specifications is tests/test_solver_gpu.py, test_sigma_gpu.py and test_pndm_gpu.py."""
import pytest
import torch

import sigma_spec as SP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = SP.SHAPES[0], SP.SHAPES[3]          # (2, 3, 20, 4, 8); (2, 2, 37, 3, 5): three latent channels in rows of five
assert SHAPES == ((2, 3, 20, 4, 8), (2, 2, 37, 3, 5))
IDS = ["x".join(map(str, s)) for s in SHAPES]
GUIDED = [(phi, single) for phi in (0.0, 0.7) for single in (False, True)]          # guidance_rescale, with / without pred_single


@pytest.fixture(scope="module")
def hip():
    from followyourclick_amd import ops
    return ops.get()


def launch(step, shape, dt, coef, order, phi, single, hists=(1, 2, 3), **buffers):
    """one launch of a step on device copies of sigma_spec's operands (hist_k for k in hists), hist_out full of NaN -> (latents, hist_out) on the host"""
    B, F, HW, CL, ld = shape
    o = SP.operands(shape, dt)
    lat, out = o["latents"].clone().to(DEV), torch.full((B, CL, F, HW), float("nan"), device=DEV)
    hist = {f"hist_{k}": o[f"hist_{k}"].to(DEV) for k in hists}
    step(o["pred"].to(DEV), lat, torch.tensor(coef, dtype=torch.float64).float().to(DEV), hist_out=out, order=order, B=B, F=F, HW=HW, c_latent=CL, ld=ld,
         cfg=True, guidance=SP.GUIDANCE, pred_single=o["single"].to(DEV) if single else None, video_scale=SP.VIDEO_SCALE if single else 0.0,
         guidance_rescale=phi, **hist, **buffers)
    torch.cuda.synchronize()
    assert torch.isfinite(lat).all() and torch.isfinite(out).all()
    return lat.cpu(), out.cpu()


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_solver_step_is_the_sigma_step_without_noise(hip, shape, dt):
    """m0 = a_x x + a_v v, x' = c_x x + c_0 m0 + c_1 hist_1 + c_2 hist_2 is the sigma step of the same order with hist_out given and noise = NULL, on the same
    8-float row (c_3 and c_n are then never read)"""
    row = (*SP.CONVERT["v_prediction"], *SP.UPDATE)
    for order in (1, 2, 3):
        for phi, single in GUIDED:
            # (the solver takes no hist_3: it is handed to neither)
            sol = launch(hip.cfg_solver_step, shape, dt, row, order, phi, single, hists=(1, 2))
            sig = launch(hip.cfg_sigma_step, shape, dt, row, order, phi, single, hists=(1, 2), noise=None)
            assert torch.equal(sol[0], sig[0]) and torch.equal(sol[1], sig[1]), (order, phi, single)


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_pndm_step_is_the_sigma_step_with_the_identity_conversion(hip, shape, dt):
    """x' = c_x x + c_0 g + c_1 hist_1 + c_2 hist_2 + c_3 hist_3 without sample and accumulator buffers is the sigma step with a_x = 0, a_v = 1:
    d = 0 x + 1 v = v exactly for finite x"""
    cx, *c = SP.UPDATE[:5]
    for order in SP.ORDERS:
        for phi, single in GUIDED:
            pndm = launch(hip.cfg_pndm_step, shape, dt, (cx, *c, 0.0), order, phi, single)
            sig = launch(hip.cfg_sigma_step, shape, dt, (0.0, 1.0, cx, *c, 0.0), order, phi, single, noise=None)
            assert torch.equal(pndm[0], sig[0]) and torch.equal(pndm[1], sig[1]), (order, phi, single)
