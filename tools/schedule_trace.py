#!/usr/bin/env python3
"""Print the launch sequence of the engines over the trace matrix of tests/trace_ops.py: op, scalar arguments and the dataflow
identity of every tensor argument, one launch per line.  Two trees whose outputs are byte-identical run the same schedule.

    python tools/schedule_trace.py > new.txt
    PYTHONPATH=/path/to/another/tree python tools/schedule_trace.py > old.txt && diff old.txt new.txt

The engines (and the oracle's weight shapes) come from PYTHONPATH when it names a tree, the recording backend always from this one."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
sys.path.append(os.path.join(ROOT, "tests"))

import trace_ops  # noqa: E402


def variant_cases():
    """(id, UNet3DConfig options, (B, F, H, W), shared_prefix): the per-frame GroupNorm / temporal-conv variants of the tiny UNet"""
    out = []
    for tag, opts in (("inflated_gn", dict(use_inflated_groupnorm=True)), ("tconv", dict(use_temporal_conv=True)),
                      ("inflated_gn+tconv", dict(use_inflated_groupnorm=True, use_temporal_conv=True))):
        for shape in trace_ops.UNET_SHAPES[:2]:
            for share in (1, 2):
                out.append(("x".join(map(str, shape)) + f"-{tag}-share{share}", opts, shape, share))
    return out


def run_variant(case) -> "trace_ops.TraceOps":
    import torch
    import tconv_spec
    from followyourclick_amd.engine import unet3d
    from followyourclick_amd.engine.weights import pack_unet
    _, opts, (B, F, H, Wd), share = case
    cfg = tconv_spec.tconv_cfg(**dict(dict(use_inflated_groupnorm=False, use_temporal_conv=False), **opts))
    sd = tconv_spec.tconv_weights(0, 11)
    if not cfg.use_temporal_conv:
        sd = {k: v for k, v in sd.items() if ".temporal_conv." not in k}
    ops = trace_ops.TraceOps(fused=True)
    eng = unet3d.UNet3DEngine(pack_unet(sd, cfg, torch.bfloat16, "cpu"), ops=ops)
    eng.prepare_context(torch.zeros(B, 77, 64))
    _, temb = eng.prepare_time_embeddings([500], [2] * B, [4] * B, B)
    ops.reset()
    eng.forward(torch.zeros(B // share * F * H * Wd, 64, dtype=torch.bfloat16), temb, B, F, H, Wd, shared_prefix=share)
    return ops


def main():
    import followyourclick_amd
    from followyourclick_amd.engine import UNet3DConfig
    print(f"# engines from {os.path.dirname(os.path.abspath(followyourclick_amd.__file__))}", file=sys.stderr)
    for case in trace_ops.unet_cases():
        print(f"== unet {case[0]}")
        print("\n".join(trace_ops.run_unet(case).lines()))
    if hasattr(UNet3DConfig, "use_temporal_conv"):      # (a tree from before these options prints the cases above and below only)
        for case in variant_cases():
            print(f"== unet {case[0]}")
            print("\n".join(run_variant(case).lines()))
    for case in trace_ops.vae_cases():
        print(f"== vae {case[0]}")
        print("\n".join(trace_ops.run_vae(case).lines()))


if __name__ == "__main__":
    main()
