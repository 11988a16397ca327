"""The bits of the four sampler-step families on one MI355X, as digests: the yardstick of a change that must not move a number (profiles/step_kernels_one_body.txt).

  python tools/step_bits.py                                   the library of this tree
  FYC_LIB_PATH=/path/to/libfyc_hip.so python tools/step_bits.py      another build of the same ABI (followyourclick_amd/_lib.py), e.g. the parent commit's

Every launch is one of the kernel tests' own: the seeded operands of tests/sampling_spec.py, solver_spec.py, sigma_spec.py and pndm_spec.py through their run_step /
step_kwargs, over every SHAPES x dtype x VARIANTS (the DDIM step with and without the guidance rescale; the sigma and PNDM steps with and without their optional
stores).  One sha256 per family over the bytes of everything a launch writes or could have written, in launch order, plus the number of launches.  The digests are
a property of one compiler version and one device: two builds are compared in two runs of this tool, nothing is kept as a golden value.
"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import pndm_spec as PS          # noqa: E402
import sampling_spec as SS      # noqa: E402
import sigma_spec as GS         # noqa: E402
import solver_spec as VS        # noqa: E402

DEV = "cuda:0"
DTYPES = ("bf16", "f16", "f32")


def on(t):
    return t.to(DEV)


def ddim(hip, shape, dt, var):
    """the launch of tests/test_sampling_gpu.py, rescaled and plain -> the latents of each"""
    o = SS.operands(shape, dt)
    kw = dict(pred_single=on(o["single"]) if var.single else None, variance_noise=on(o["noise"]) if var.noise else None, **SS.step_kwargs(shape, var))
    lat, plain = on(o["latents"].clone()), on(o["latents"].clone())
    hip.cfg_ddim_step_rescaled(on(o["pred"]), lat, on(o["coef"]), guidance_rescale=var.phi, **kw)
    hip.cfg_ddim_step(on(o["pred"]), plain, on(o["coef"]), **kw)
    return [(lat,), (plain,)]


FAMILIES = {
    "ddim": (SS, ddim),
    "solver": (VS, lambda hip, s, dt, v: [VS.run_step(hip, s, dt, v, on=on)]),
    "sigma": (GS, lambda hip, s, dt, v: [GS.run_step(hip, s, dt, v, on=on, store=store) for store in (True, False)]),
    "pndm": (PS, lambda hip, s, dt, v: [tuple(PS.run_step(hip, s, dt, v, on=on, store=store).values()) for store in (True, False)]),
}


def main():
    from followyourclick_amd import _lib, ops
    hip = ops.get()
    print(f"library {_lib.LIB_PATH}, ABI {hip.lib.fyc_version()}, {torch.cuda.get_device_name(0)}")
    for name, (spec, run) in FAMILIES.items():
        h, launches = hashlib.sha256(), 0
        for shape in spec.SHAPES:
            for dt in DTYPES:
                for var in spec.VARIANTS:
                    for outs in run(hip, shape, dt, var):
                        torch.cuda.synchronize()
                        launches += 1
                        for t in outs:
                            h.update(t.contiguous().cpu().numpy().tobytes())
        print(f"{name:7s} sha256 {h.hexdigest()}  {launches} cases ({len(spec.SHAPES)} shapes x {len(DTYPES)} dtypes x {len(spec.VARIANTS)} variants)", flush=True)


if __name__ == "__main__":
    main()
