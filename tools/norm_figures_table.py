"""The tables of profiles/norm_bound_coverage.txt from the figures tests/test_norm_bounds_gpu.py appends to FYC_NORM_FIGURES=<file>:
    FYC_NORM_FIGURES=figures.txt pytest -m gpu tests/test_norm_bounds_gpu.py && python tools/norm_figures_table.py figures.txt
Per comparison: the case, the launch it makes (tests/norm_cases.py traits()), its global relative L2 (and the tolerance asserted) and its worst |got - ref| / bound; then the worst
ratio per entry point and type, and the global error of GroupNorm / LayerNorm by mean / std and by where the statistics came from, against the project's RTOL."""
import collections
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import norm_cases as N  # noqa: E402
from kernel_compare import RTOL  # noqa: E402

by_name = {c.name: c for c in N.CASES}
rows = []
for line in open(sys.argv[1]):
    f = line.split()
    op, dt, name, ms, rel, ratio = f[:6]
    rows.append((op, dt, name, float(ms[3:]), float(rel), float(ratio), " ".join(f[6:])))


def short(c):
    t = N.traits(c)
    if c.op == "gn_stats":
        return f"nthr {t['nthr']} rpi {t['rpi']} idle {t['idle']} chunks {t['chunks']}x{t['rpb']} last {t['last_rows']} {'U' if t['unroll'] else '-'}{'T' if t['tail'] else '-'} glaps {t['group_laps']}"
    if c.op == "gn_apply":
        return f"blocks {t['blocks']} laps {t['laps']} {'straddle' if t['straddle'] else 'aligned'}"
    if c.op == "gn_apply_cs":
        s = f"nthr {t['nthr']} rpi {t['rpi']} chunks {t['chunks']}x{t['rpb']} {'U' if t['unroll'] else '-'}{'T' if t['tail'] else '-'} ss {t['stat_samples']} {'straddle' if t['straddle'] else 'aligned'}"
        if c.path == "parts":
            s += " " + " ".join(f"[bm {f['bm']} slots {f['slots']} {'fast' if f['fast'] else 'general'} tiles {f['tiles']}{' partial-last' if f['partial_last_tile'] else ''}]" for f in t["fold"])
        return s
    if c.op == "chan_stats_reduce":
        return f"slots {t['slots']} tiles {t['tiles']} group {t['group']}{' partial-last' if t['partial_last_tile'] else ''}"
    if c.op in ("layernorm", "row_stats"):
        return f"MAXCH {t['maxch']} need {t['need']} idle-lanes {t['idle_lanes']}{' partial-block' if t['partial_block'] else ''}"
    return f"laps {t['laps']} idle-waves {t['idle_waves']}"


ops = []
for r in rows:
    if r[0] not in ops:
        ops.append(r[0])
for op in ops:
    print(f"fyc_{op}\n" + "-" * (4 + len(op)))
    for o, dt, name, ms, rel, ratio, note in rows:
        if o == op:
            c = by_name[name]
            tol = N.rtol(c)
            print(f"   {name[len(op) + 1:]:58s} {short(c):96s} {rel:.3e} ({'recorded' if tol == float('inf') else f'{tol:.1e}'})  {ratio:.4f} {note}".rstrip())
    print()

print("Worst |got - ref| / bound per entry point and type")
print("--------------------------------------------------")
worst = collections.defaultdict(float)
for o, dt, name, ms, rel, ratio, note in rows:
    worst[(o, dt)] = max(worst[(o, dt)], ratio)
for (o, dt), v in worst.items():
    print(f"   {o:20s} {dt:5s} {v:.4f}")
print()
print("Global relative L2 by mean / std (worst case of each), against the project's RTOL")
print("---------------------------------------------------------------------------------")
g = collections.defaultdict(float)
for o, dt, name, ms, rel, ratio, note in rows:
    if o in ("gn_apply", "gn_apply_cs", "layernorm"):
        src = "own row sums" if o == "layernorm" else "fyc_gn_stats' own" if getattr(by_name[name], "chained", False) else "exact statistics"
        g[(o, src, dt, ms)] = max(g[(o, src, dt, ms)], rel)
for (o, src, dt, ms), v in sorted(g.items()):
    print(f"   {o:14s} {src:18s} {dt:5s} mean/std {ms:5g}  {v:.3e}  RTOL {RTOL[dt]:.1e}  {'LEAVES' if v > RTOL[dt] else 'inside'}")
print(f"\n{len(rows)} comparisons")
