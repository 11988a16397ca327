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


def main():
    import followyourclick_amd
    print(f"# engines from {os.path.dirname(os.path.abspath(followyourclick_amd.__file__))}", file=sys.stderr)
    for case in trace_ops.unet_cases():
        print(f"== unet {case[0]}")
        print("\n".join(trace_ops.run_unet(case).lines()))
    for case in trace_ops.vae_cases():
        print(f"== vae {case[0]}")
        print("\n".join(trace_ops.run_vae(case).lines()))


if __name__ == "__main__":
    main()
