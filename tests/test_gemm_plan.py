"""The host decisions of fyc_gemm, pinned without a GPU: csrc/gemm.hip and csrc/api.hip are linked with tests/gemm_plan_harness.hip, whose
fycg::run_* stubs record the launch they are asked for, and the program's table - per case the three host queries (workspace bytes,
row_parts tiles, chan_parts layout), the launch (family, tile config, ring depth, wide, colc, splitk, cs_slots, batch) and the return
code - must equal tests/golden/gemm_plan_table.txt (equal rows folded, see compact()).  The table was recorded from the commit before the planner (gemm_plan.h) existed;
the rows that differ from that recording are the ones where the old code broke an invariant the harness asserts for every successful
call (see the head of gemm_plan_harness.hip): chan_parts next to ln_stats / row_parts on a split-K shape is now refused (the sums used
to be written in another layout than fyc_gemm_stat_layout announced), and fyc_gemm_workspace_bytes answers 0 for a problem whose
operands rule out the split.

To re-record after an intended change of a rule: run the program this test builds and review the diff of the table row by row."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "followyourclick_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_table.txt")
RETIRED = os.path.join(ROOT, "tests", "golden", "gemm_retired_ids.txt")
# the program passes made-up pointers: no device may be visible to it (it checks, and hides them itself as well)
NO_GPU = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    from followyourclick_amd import _build
    try:
        hipcc = _build._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    exe = tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_harness"
    cmd = [hipcc, *_build._flags("gemm.hip"), os.path.join(ROOT, "tests", "gemm_plan_harness.hip"), os.path.join(CSRC, "gemm.hip"), os.path.join(CSRC, "api.hip"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(exe)


@pytest.fixture(scope="module")
def table(harness):
    r = subprocess.run([harness], capture_output=True, text=True, env=dict(os.environ, **NO_GPU))
    return r.returncode, r.stdout.splitlines(), r.stderr


def test_invariants_hold_for_every_successful_call(table):
    rc, lines, err = table
    broken = [ln for ln in lines if " !" in ln]
    assert not broken, "\n".join(broken[:20])
    assert rc == 0, err[-2000:]


def compact(lines):
    """The table with equal rows folded, lossless for the harness's fixed case list: cases that got the same queries, launch and return code
    share a line.  Default-flag cases fold per M x N over (dtype / mode, K); the feature cases per mode and shape over (dtype: features).  The
    16-bit entries differ by their dtype prefix only, which is checked here and written `16_`."""
    groups = {}
    for ln in lines:
        key, queries, launch, rc = ln.split(" | ", 3)
        dtype, mode, shape, var = key.split(" ", 3)
        fam = launch.split(" ", 1)[0]
        assert not fam.startswith(("bf16_", "f16_")) or fam.startswith(dtype + "_"), ln
        res = f"{queries} | {re.sub('^(bf16|f16)_', '16_', launch)} | {rc}"
        if var == "base":
            M, N, K = shape.split("x")
            groups.setdefault(f"base {M}x{N}", {}).setdefault(res, {}).setdefault(f"{dtype}/{mode}", []).append(K)
        else:
            groups.setdefault(f"{mode} {shape}", {}).setdefault(res, {}).setdefault(dtype, []).append(var)
    out = []
    for head, by_res in groups.items():
        for res, who in by_res.items():
            by_list = {}
            for name, items in who.items():
                by_list.setdefault(",".join(items), []).append(name)
            out.append(f"{head} | {' ; '.join(','.join(names) + ': ' + items for items, names in by_list.items())} | {res}")
    return out


def test_table_equals_the_recorded_one(table):
    _, lines, _ = table
    got, want = compact(lines), open(GOLDEN).read().splitlines()
    diff = [f"- {w}\n+ {g}" for w, g in zip(want, got) if w != g]
    assert len(got) == len(want) and not diff, f"{len(diff)} lines differ ({len(got)} vs {len(want)} lines):\n" + "\n".join(diff[:20])


def retired_id_cases():
    """the harness's file-mode lines for the ids of retired experiments, 16-bit PLAIN on a small and a large shape: the one-phase tiles 5 / 6 / 7, the
    32x32x16 twins 12 / 13 / 14 (retired, never built: planned under their own number, which gemm_kernel.h::dispatch_tiles - a stub here - refuses), the main-loop experiments' 21 / 22 /
    23 / 31 (run their one-phase twins), the reserved tuning keys 8 / 9 / 14, and the forced tiles next to output statistics"""
    out = []
    for dtype in (1, 2):
        for M, N, K in ((300, 320, 320), (16384, 640, 640)):
            shape = f"dtype={dtype} mode=0 M={M} N={N} K={K} lda={K} ldw={K} ldo={N} ldr={N}"
            out += [f"d{dtype}-{M}-tile{t} {shape} tile={t}" for t in (5, 6, 7, 12, 13, 14, 21, 22, 23, 31)]
            out += [f"d{dtype}-{M}-key{k}={v} {shape} tile=0 tune={k}:{v}" for k, v in ((8, 1), (9, 2), (9, 3), (14, 1))]
            if M == 16384:
                out += [f"d{dtype}-{M}-chan-tile{t} {shape} chan=1 cs_rows=4096 tile={t}" for t in (5, 12, 21, 31)]
    return out


def test_retired_ids_answer_as_recorded(harness, tmp_path):
    """tests/golden/gemm_retired_ids.txt was recorded from the last commit that could still build the experiments (in its product build, which had
    them compiled out): what a caller gets for their tile ids and tuning keys has not moved since"""
    path = tmp_path / "cases.txt"
    path.write_text("".join(ln + "\n" for ln in retired_id_cases()))
    r = subprocess.run([harness, str(path)], capture_output=True, text=True, env=dict(os.environ, **NO_GPU))
    # (the recording predates the last field of an answer line, the launch decisions: tests/test_gemm_cases.py checks those)
    got, want = [ln.rsplit(" | ", 1)[0] for ln in r.stdout.splitlines()], open(RETIRED).read().splitlines()
    assert r.returncode == 0, r.stderr[-2000:]
    diff = [f"- {w}\n+ {g}" for w, g in zip(want, got) if w != g]
    assert len(got) == len(want) and not diff, f"{len(diff)} lines differ ({len(got)} vs {len(want)} lines):\n" + "\n".join(diff[:20])
