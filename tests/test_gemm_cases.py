"""Which kernel every case of tests/gemm_cases.py launches, proven without a GPU: the cases are written in the line format of
tests/gemm_plan_harness.hip's second mode (the planner and fyc_gemm linked with recording stubs, as in tests/test_gemm_plan.py) and the
recorded launch - the tile config after the narrow-epilogue rewrite, ring depth, wide, split or not - must equal the intent the case declares, and so
must what csrc/gemm_plan.h::gemm_launch_plan decides for that launch (pre-staged epilogue inputs, the epilogue form).
The GPU tests (tests/test_gemm_epilogues_gpu.py) parametrise from the same list, so a case there cannot silently run another kernel than
its name says: that is what had happened to the 16-bit sweeps of test_gemm_plain / test_gemm_conv, whose arguments are pinned here too."""
import os
import subprocess
from dataclasses import replace

import pytest

import gemm_cases as G
from test_kernels_gpu import CONV_TILES, F16_TILES, PLAIN_TILES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "followyourclick_amd", "csrc")
CASES = G.CASES


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    from followyourclick_amd import _build
    try:
        hipcc = _build._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("gemm_cases")
    exe = tmp / "gemm_plan_harness"
    cmd = [hipcc, *_build._flags("gemm.hip"), os.path.join(ROOT, "tests", "gemm_plan_harness.hip"), os.path.join(CSRC, "gemm.hip"), os.path.join(CSRC, "api.hip"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    cases = CASES + G.OLD_PLAIN_SWEEP
    path = tmp / "cases.txt"
    path.write_text("".join(G.harness_line(c) + "\n" for c in cases))
    # the program passes made-up pointers: no device may be visible to it (it checks, and hides them itself as well)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, env=env)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and len(lines) == len(cases), (r.returncode, r.stderr[-2000:], lines[-3:])
    out = {}
    for c, ln in zip(cases, lines):
        name, launch, executed, rest = ln.split(" | ", 3)
        rc, decided = rest.rsplit(" | ", 1)
        assert name == c.name, (name, c.name)
        fam, cfg, ns, wide, colc, splitk, cs_slots, batch = launch.split()
        decided = None if decided == "-" else {k: int(v) for k, v in (f.split("=") for f in decided.split())}      # gemm_launch_plan's answer for the recorded launch
        out[c.name] = dict(fam=fam, asked_cfg=int(cfg), cfg=int(executed.split()[0]), ring=int(ns), wide=int(wide), splitk=int(splitk), rc=int(rc.split()[0]), decided=decided,
                           line=ln)
    return out


def table(recorded):
    """the table of profiles/gemm_epilogue_coverage.txt"""
    return [f"{c.name:34s} {r['fam']:10s} tile {r['cfg']:2d}  ring {r['ring']:2d}  wide {r['wide']}  splitk {r['splitk']}" for c in CASES for r in [recorded[c.name]]]


@pytest.mark.parametrize("case", CASES, ids=G.case_ids(CASES))
def test_case_launches_what_it_declares(recorded, case):
    r = recorded[case.name]
    assert r["rc"] == 0, r["line"]
    got = (r["cfg"], r["ring"], r["wide"], r["splitk"] > 1)
    assert got == (case.want_cfg, case.want_ring, case.want_wide, case.want_split), f"(tile, ring, wide, split) {got} recorded: {r['line']}"
    if case.want_wide and case.tile in (8, 10) and not (case.rowbias and case.rpb % 128 != 0):
        assert r["cfg"] == case.tile, r["line"]      # (with row-bias groups to stage, the 128-byte twins 6 / 1 run: gemm_cases.py)
    fam = {"f32": "f32", "bf16": "bf16_", "f16": "f16_"}[case.dt]
    ends = ("act", "f32") if case.act else {G.PLAIN: ("plain", "f32"), G.CONV: ("conv", "f32"), G.UP2: ("conv", "f32"), G.T3: ("t3",)}[case.mode]
    assert r["fam"].startswith(fam) and r["fam"].endswith(ends), r["line"]
    if case.group == "geglu" and case.want_wide and case.tile in G.GEGLU_REPLACED:
        assert r["asked_cfg"] == r["cfg"] == G.GEGLU_REPLACED[case.tile], r["line"]      # (the planner replaces the tile: gemm_plan.h::GEMM_TILES, column `geglu`)
    if case.group == "act" and case.want_wide:
        assert r["cfg"] == G.ACT_WIDE_TILES.get(r["asked_cfg"], 2), r["line"]             # (the family builds 1, 2 and 6: the entry folds the planned tile)
    assert r["decided"] is not None and r["decided"]["pre"] == int(case.want_pre), r["line"]      # what the library decides, against gemm_cases.pre_staged
    if case.want_form:
        assert form_of(case, r) == case.want_form, r["line"]


def form_of(case, r):
    """the epilogue form the kernel takes (csrc/gemm_kernel.h::gemm_epilogue) for what the library decided: wide, the epilogue, fast1 and heads_pk"""
    d = r["decided"]
    if not r["wide"]:
        return "narrow"
    if case.act:
        return "staged"
    if case.epilogue == G.HEADS:
        return "packed" if d["fast1"] and d["heads_pk"] else "staged"
    if case.epilogue == G.GEGLU:
        return "packed" if d["fast1"] else "staged"
    return "packed"


@pytest.mark.parametrize("mode,tiles,extra", [(G.PLAIN, PLAIN_TILES, G.EXTRA_PLAIN_RINGS), (G.CONV, CONV_TILES, []), (G.UP2, CONV_TILES, [])])
def test_every_tile_of_the_sweeps_is_executed_wide(recorded, mode, tiles, extra):
    """across the wide, unsplit cases of a mode the executed (tile config, ring depth) are exactly the sweep's list (tile 0 being the automatic
    choice) and the f16 subset's (F16_TILES has (1, 2) and (2, 2), which CONV_TILES leaves out), plus in PLAIN mode the two deeper rings of the 128x64 linears"""
    sweep = [c for c in CASES if c.group in G.LINEAR_GROUPS]      # (the groups of the other epilogues: test_new_groups_execute_exactly_their_declared_wide_tiles)
    executed = {(recorded[c.name]["cfg"], recorded[c.name]["ring"]) for c in sweep if c.mode == mode and recorded[c.name]["wide"] == 1 and recorded[c.name]["splitk"] <= 1}
    want = {(t if t else G.AUTO_TILE, r if t else 2) for t, r in tiles + F16_TILES} | set(extra)
    assert executed == want, (sorted(executed - want), sorted(want - executed))
    bf16 = {(recorded[c.name]["cfg"], recorded[c.name]["ring"]) for c in sweep if c.mode == mode and c.dt == "bf16" and recorded[c.name]["wide"] == 1 and recorded[c.name]["splitk"] <= 1}
    assert {(t if t else G.AUTO_TILE, r if t else 2) for t, r in tiles} <= bf16
    for t in (8, 10):      # and the 64-byte K-tile configs by cases that ASKED for them
        assert any(c.tile == t and recorded[c.name]["cfg"] == t and recorded[c.name]["wide"] == 1 for c in sweep if c.mode == mode), t


def test_every_group_and_dtype_has_cases():
    have = {(c.group, c.dt) for c in CASES}
    want = ({(g, dt) for g in ("plain", "conv", "pixel", "stripes") + G.EPILOGUE_GROUPS for dt in ("bf16", "f16", "f32")} |
            {(g, dt) for g in ("narrow", "alias", "splitk") for dt in ("bf16", "f16")})
    assert have == want
    assert {c.group for c in CASES} == set(G.LINEAR_GROUPS) | set(G.EPILOGUE_GROUPS)


# the wide tiles each new group declares (the issue's lists; tile 0 = the automatic choice at that shape), after the replacements the planner and the act entries make
WIDE_TILES = {
    "geglu": {1, 2, 3, 4, 5, 7, 8, 10},                 # 0 -> 1 at N = 672; 6 and 11 -> 5
    "heads": {1, 2, 5, 6, 11},                          # 0 -> 1 at N = 600 / 384, 2 at N = 400 / 200 / 256 / 128
    "act": {1, 2, 6},                                   # what the family builds
    "lnfold": {1, 2, 5, 6},
    "dualk": {1, 2, 5, 6},
    "t3": {(t if t else G.AUTO_TILE) for t, _ in CONV_TILES + F16_TILES},
}


@pytest.mark.parametrize("group", G.EPILOGUE_GROUPS)
def test_new_groups_execute_exactly_their_declared_wide_tiles(recorded, group):
    cases = G.by_group(group)
    executed = {recorded[c.name]["cfg"] for c in cases if recorded[c.name]["wide"] == 1}
    assert executed == WIDE_TILES[group], (sorted(executed - WIDE_TILES[group]), sorted(WIDE_TILES[group] - executed))
    assert {c.want_cfg for c in cases if c.want_wide} == WIDE_TILES[group]
    for dt in ("bf16", "f16"):      # both 16-bit types reach the narrow form as well, f32 has no other
        assert any(recorded[c.name]["wide"] == 0 for c in cases if c.dt == dt) or group in ("dualk", "t3"), (group, dt)
    assert all(recorded[c.name]["wide"] == 0 for c in cases if c.dt == "f32")
    assert not any(recorded[c.name]["splitk"] > 1 for c in cases)


def test_forms_chosen_inside_launch(recorded):
    """pre, fast1 and heads_pk are decided by gemm_plan.h::gemm_launch_plan, which the harness calls for the recorded launch: the conditions are restated in
    gemm_cases.pre_staged (and its head), the cases meant for a form must satisfy them, and the library must decide what the restatement says"""
    new = G.by_group(*G.EPILOGUE_GROUPS)
    for c in new:
        keys = dict(c.tuning)
        r = recorded[c.name]
        assert r["decided"] is not None and r["decided"]["pre"] == int(c.want_pre) and form_of(c, r) == c.want_form, r["line"]
        assert r["decided"]["fast1"] == (0 if keys.get(G.TUNE_GENERIC_PASS1) == 1 else 1), r["line"]
        if keys.get(G.TUNE_HEADS_PACKED) in (1, 2):
            assert r["decided"]["heads_pk"] == (1 if keys[G.TUNE_HEADS_PACKED] == 1 else 0), r["line"]
        if c.want_pre:
            cfg = c.want_cfg
            assert c.want_wide == 1 and G.k_tiles(c, cfg) >= 2 and c.ln <= 1 and (c.ln == 0 or c.M % 2 == 0) and keys.get(G.TUNE_NO_PRESTAGE, 0) == 0, c.name
        if c.group == "lnfold" and (c.M % 2 == 1 or c.ln > 1):
            assert not c.want_pre, c.name                                   # an odd M and ln_nparts load in the epilogue without any key
        if c.group == "heads" and c.want_wide:
            assert keys.get(G.TUNE_HEADS_PACKED) in (1, 2), c.name          # never left to the M <= 8192 default
            assert c.want_form == ("packed" if keys[G.TUNE_HEADS_PACKED] == 1 and not keys.get(G.TUNE_GENERIC_PASS1) else "staged"), c.name
        if c.group == "geglu" and c.want_wide:
            assert c.want_form == ("staged" if keys.get(G.TUNE_GENERIC_PASS1) else "packed"), c.name
        if not c.want_wide:
            assert c.want_form == "narrow" and c.want_cfg in (1, 2), c.name
    # the wide problems of these four groups have a key-12 twin on the automatic tile, and a twin differs from its case by that key alone
    by_name = {c.name: c for c in new}
    twins = [c for c in new if c.name.endswith("-k12")]
    assert {c.group for c in twins} == {"geglu", "heads", "act", "lnfold"}
    for t in twins:
        c = by_name[t.name[:-4]]
        assert c.want_pre and not t.want_pre and c.tile == t.tile == 0
        assert replace(t, name=c.name, tuning=c.tuning, want_pre=True) == c and t.tuning == c.tuning + ((G.TUNE_NO_PRESTAGE, 1),), t.name
    for c in new:      # every wide problem (operands and shape) of the four groups is covered by a twin
        if c.group in ("geglu", "heads", "act", "lnfold") and c.want_wide and c.want_pre and c.tile == 0 and not dict(c.tuning).get(G.TUNE_GENERIC_PASS1):
            assert c.name + "-k12" in by_name, c.name
    # the other keyed cases: the same problem as an unkeyed (or otherwise keyed) case of the group
    problems = {}
    for c in new:
        problems.setdefault(G.problem_key(replace(c, want_wide=0)), []).append(c)
    for c in new:
        if c.tuning:
            assert len(problems[G.problem_key(replace(c, want_wide=0))]) >= 2, c.name


def test_narrow_and_split_cases_are_what_they_say(recorded):
    for c in G.by_group("narrow"):
        assert recorded[c.name]["wide"] == 0 and recorded[c.name]["cfg"] in (1, 2), recorded[c.name]["line"]
    for c in G.by_group("splitk"):
        assert recorded[c.name]["splitk"] > 1 and recorded[c.name]["wide"] == 1, recorded[c.name]["line"]


@pytest.mark.parametrize("case", G.OLD_PLAIN_SWEEP, ids=G.case_ids(G.OLD_PLAIN_SWEEP))
def test_old_plain_sweep_takes_the_narrow_epilogue(recorded, case):
    """THE FINDING, pinned: test_gemm_plain's arguments (rows_per_batch = 50: row-bias groups the packed epilogue cannot stage) make every 16-bit case
    narrow, and the narrow epilogue only exists for configs 1 / 2 - tile 5 is asked for and never runs.  If a planner change turns this sweep into
    a real one (or hollows out the new one: test_case_launches_what_it_declares), it shows here"""
    r = recorded[case.name]
    assert r["rc"] == 0 and r["asked_cfg"] == 5 and r["wide"] == 0 and r["cfg"] in (1, 2) and r["cfg"] == case.want_cfg, r["line"]
