"""Is a change of the kernel sources codegen-neutral?  Compiles each named source of csrc/ twice - from the tree of a git revision and from the
working tree - to gfx950 device assembly (the build's flags for that source, --cuda-device-only -S) and counts the lines that differ.
    python tools/device_asm_diff.py REV [source.hip ...]      # default: every source of the build; exit status 1 if any source differs

Identical instruction streams are the proof a refactor of a kernel file owes: behaviour and speed are then unchanged by construction and no
timing run is needed.  The comparison is on text lines and knows no instruction.  Left out before comparing: comment lines, `.file`, `.ident`, and
the lines that name __hip_cuid_* (a hash per translation unit).  A template kernel whose parameter struct was renamed or moved to another
namespace keeps its name and template arguments and differs in the mangled parameter list behind them (..E v <parameters>): lines that differ
in nothing else are counted apart and reported with both manglings, they do not fail the run.  A template that lost or gained a parameter
renames every instantiation: for the same comparison every mangled symbol (_Z...) is replaced by its index of first appearance in its file, the
lines that differ in such spellings only are counted with the others, and the two sides must define equally many kernels."""
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from followyourclick_amd import _build  # noqa: E402

CSRC_REL = os.path.relpath(_build.CSRC, ROOT)
DROPPED = re.compile(r"^\s*(;|//|\.file\b|\.ident\b)|__hip_cuid_")
PARAMS = re.compile(r"\b(_Z\w*Ev)(\w*)")      # greedy: the last `Ev` of a symbol closes the template arguments and names the void return type
SYMBOL = re.compile(r"(?<!\w)(?:\.L)?_Z\w+")      # (.L_Z...: the resource-usage symbols of a function that was not inlined)
KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")


def by_index(lines):
    """the lines with every mangled symbol replaced by its index of first appearance"""
    seen = {}
    return [SYMBOL.sub(lambda m: f"<symbol {seen.setdefault(m.group(0), len(seen))}>", x) for x in lines]


def device_asm(csrc, src, out):
    """the normalised assembly lines of csrc/src, or None where that tree has no such file"""
    if not os.path.exists(os.path.join(csrc, src)):
        return None
    r = subprocess.run([_build._hipcc(), *_build._flags(src), "--cuda-device-only", "-S", os.path.join(csrc, src), "-o", out], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {os.path.join(csrc, src)}:\n{r.stderr[-4000:]}")
    with open(out) as f:
        return [line.rstrip() for line in f if line.strip() and not DROPPED.search(line)]


def differing(old, new, tmp, tag):
    """lines of `diff old new` that belong to one side only"""
    if old == new:
        return 0
    paths = []
    for side, lines in (("old", old), ("new", new)):
        paths.append(os.path.join(tmp, f"{tag}.{side}.txt"))
        with open(paths[-1], "w") as f:
            f.write("\n".join(lines) + "\n")
    out = subprocess.run(["diff", *paths], capture_output=True, text=True).stdout
    return sum(line.startswith(("<", ">")) for line in out.split("\n"))


def compare(src, old, new, tmp):
    """-> (lines of the new assembly, differing lines, lines that differ in the spelling of symbols only, what was respelt)"""
    n = differing(old, new, tmp, src)
    if n == 0:
        return len(new), 0, 0, ""
    params = n - differing([PARAMS.sub(r"\1<parameters>", x) for x in old], [PARAMS.sub(r"\1<parameters>", x) for x in new], tmp, src + ".noparams")
    rest = differing(by_index(old), by_index(new), tmp, src + ".nosymbols")
    kernels = [len({m.group(1) for x in side for m in [KERNEL.match(x)] if m}) for side in (old, new)]
    if kernels[0] != kernels[1]:
        rest = max(rest, 1)
    types = [" | ".join(sorted({m.group(2) for x in side for m in PARAMS.finditer(x)})) for side in (old, new)]
    what = (f"{params} in kernel parameter types: {types[0]} -> {types[1]}; " if params else "") + f"kernel symbols {kernels[0]} -> {kernels[1]}"
    return len(new), rest, n - rest, what


def main(argv):
    if not argv:
        raise SystemExit(__doc__)
    rev, srcs = argv[0], argv[1:] or _build.SOURCES
    with tempfile.TemporaryDirectory() as tmp:
        ar = subprocess.run(["git", "-C", ROOT, "archive", rev, CSRC_REL, "include/fyc.h"], capture_output=True)
        if ar.returncode != 0:
            raise SystemExit(f"git archive {rev}: {ar.stderr.decode()[-2000:]}")
        os.makedirs(os.path.join(tmp, "rev"))
        subprocess.run(["tar", "-x", "-C", os.path.join(tmp, "rev")], input=ar.stdout, check=True)
        trees = {"old": os.path.join(tmp, "rev", CSRC_REL), "new": _build.CSRC}
        with cf.ThreadPoolExecutor(max_workers=16) as ex:
            jobs = {(s, side): ex.submit(device_asm, csrc, s, os.path.join(tmp, f"{s}.{side}.s")) for s in srcs for side, csrc in trees.items()}
        bad = 0
        for s in srcs:
            old, new = jobs[s, "old"].result(), jobs[s, "new"].result()
            if old is None or new is None:
                print(f"{s:28s} only in {'the working tree' if old is None else rev}")
                bad += 1
                continue
            lines, diff, params, types = compare(s, old, new, tmp)
            print(f"{s:28s} {lines:7d} lines  {diff:7d} differing" + (f"  ({params} more in symbol spelling only; {types})" if params else ""))
            bad += diff != 0
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
