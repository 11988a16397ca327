"""fyc_gemm's LINEAR epilogues on the tiles they name, with the pitches the engine uses (tests/gemm_cases.py; which kernel each case launches is
proven on the CPU by tests/test_gemm_cases.py).  Every case is one launch into an output that lies inside a larger, prefilled buffer - 64
elements in front, two rows behind, the pad columns [N, ldo) - compared with the emulator accumulating in f64 by kernel_compare.compare: global,
per-row and per-column relative L2 at the project's tolerances, every element within one unit of the storage type plus the f32 accumulation bound,
and nothing outside the output touched.

The GEGLU, head-split, activation, LayerNorm-fold, dual-source-K and unsplit T3 cases (one test per group, below the helpers) run the same way with the bounds of
gemm_cases.analysis (derivation: the head of tests/kernel_compare.py; CPU proof: tests/test_gemm_epilogue_cases.py): every HEADS segment in a guarded buffer of its own,
every form behind a tuning key (6, 7, 12, 13, 15) set and reset around the launch, and the key-12 twins also bit for bit against the pre-staged launch.

FYC_EPILOGUE_FIGURES=<file>: append the figures of every comparison to that file (profiles/gemm_epilogue_coverage.txt was made from it)."""
import os

import pytest
import torch

import gemm_cases as G
from kernel_compare import BoundTerms, Guard, compare
from test_kernels_gpu import hip  # noqa: F401  (the module-scoped library fixture)

pytestmark = pytest.mark.gpu

FIGURES = os.environ.get("FYC_EPILOGUE_FIGURES")
_ref_cache = {}


def reference(c):
    """operands, f64-accumulated reference buffer and bound terms of a case's PROBLEM: computed once and shared by all its tiles, never modified"""
    from dataclasses import replace
    key = replace(c, name="", group="", tile=0, ring=0, tuning=(), chan=False, cs_rows=0, want_cfg=0, want_ring=0, want_wide=0, want_split=False)
    if key not in _ref_cache:
        ops = G.operands(c)
        _ref_cache[key] = (ops, G.run_emulator(c, ops, torch.float64), G.bound_terms(c, ops))
    return _ref_cache[key]


def launch(hip, c, ops, *, residual_buf=None, **extra):  # noqa: F811
    """one launch of the case into a fresh copy of its guarded buffer; returns that buffer (GPU)"""
    buf = ops.buf.cuda()
    a, w, out, kw = G.gemm_kwargs(c, ops, buf, to=lambda t: t.cuda(), residual_buf=residual_buf)
    for k, v in c.all_tuning:
        hip.set_tuning(k, v)
    try:
        hip.gemm(a, w, out, **kw, **extra)
        torch.cuda.synchronize()
    finally:
        for k, _ in c.all_tuning:
            hip.set_tuning(k, 0)
    return buf


def check(c, ops, got_buf, ref_buf, S):
    got_buf = got_buf.cpu()
    fig = compare(G.logical(c, got_buf), G.logical(c, ref_buf), dtype=c.dt, bound_terms=BoundTerms(S, c.K, G.tile_shape(c.want_cfg)),
                  guard=Guard(ops.buf, got_buf, ops.mask), tag=c.name)
    if FIGURES:
        with open(FIGURES, "a") as f:
            f.write(f"{c.group} {c.dt} {c.name} {fig['global_rel']:.3e} {fig['row_rel']:.3e} {fig['column_rel']:.3e} {fig['elem_ratio']:.4f}\n")
    return got_buf


def _run(hip, c):  # noqa: F811
    ops, ref_buf, S = reference(c)
    return check(c, ops, launch(hip, c, ops), ref_buf, S)


# ---- the other epilogues (tests/gemm_cases.py: EPILOGUE_GROUPS; bounds: the head of tests/kernel_compare.py; CPU proof: tests/test_gemm_epilogue_cases.py) -------------
_epi_cache = {}


def epilogue_reference(c):
    """operands, reference buffers of EmuOps(acc=float64) and per-window bounds of a case's PROBLEM: computed once, shared by its tiles and keys, never modified"""
    key = G.problem_key(c)
    if key not in _epi_cache:
        ops = G.operands(c)
        _epi_cache[key] = (ops,) + G.epilogue_reference(c, ops)
    return _epi_cache[key]


def launch_epilogue(hip, c, ops, tuning=None):  # noqa: F811
    """one launch into fresh copies of the guarded buffers (one per HEADS segment); returns them (GPU)"""
    bufs = [b.cuda() for b in ops.bufs]
    a, w, out, kw = G.gemm_kwargs(c, ops, bufs if c.heads is not None else bufs[0], to=lambda t: t.cuda())
    tuning = c.all_tuning if tuning is None else tuning
    for k, v in tuning:
        hip.set_tuning(k, v)
    try:
        hip.gemm(a, w, out, **kw)
        torch.cuda.synchronize()
    finally:
        for k, _ in tuning:
            hip.set_tuning(k, 0)
    return bufs


def _run_epilogue(hip, c):  # noqa: F811
    ops, ref_bufs, bounds = epilogue_reference(c)
    got = [b.cpu() for b in launch_epilogue(hip, c, ops)]
    figs = G.judge(c, ops, got, ref_bufs, bounds)
    if FIGURES:
        with open(FIGURES, "a") as f:
            for fig in figs:
                f.write(f"{c.group} {c.dt} {fig['tag'].replace(' ', '/')} {fig['global_rel']:.3e} {fig['row_rel']:.3e} {fig['column_rel']:.3e} {fig['elem_ratio']:.4f}\n")
    if dict(c.tuning).get(G.TUNE_NO_PRESTAGE) == 1:
        # pre-staged against self-loaded epilogue inputs: the same values into the same expressions (pre_ln_row / ln_row, the column constants) - bit for bit
        twin = tuple(kv for kv in c.all_tuning if kv[0] != G.TUNE_NO_PRESTAGE)
        pre = [b.cpu() for b in launch_epilogue(hip, c, ops, tuning=twin)]
        for s, (x, y) in enumerate(zip(got, pre)):
            assert torch.equal(x.view(torch.int16 if x.element_size() == 2 else torch.int32), y.view(torch.int16 if y.element_size() == 2 else torch.int32)), \
                f"{c.name}: buffer {s} differs between the pre-staged and the self-loading launch"


GEGLU_CASES, HEADS_CASES, ACT_CASES = G.by_group("geglu"), G.by_group("heads"), G.by_group("act")
LNFOLD_CASES, DUALK_CASES, T3_CASES = G.by_group("lnfold"), G.by_group("dualk"), G.by_group("t3")


@pytest.mark.parametrize("case", GEGLU_CASES, ids=G.case_ids(GEGLU_CASES))
def test_geglu_epilogue_every_form(hip, case):  # noqa: F811
    """M = 300, N = 672 (336 outputs), K = 136, every pitch wider than its row, with and without a folded LayerNorm: the pack-first form on every tile it is built for (6 and 11
    replaced by 5), the LDS-staged form (key 13), the narrow per-lane form with the Abramowitz-Stegun gate (key 6; an output one element off 16 bytes), f32"""
    _run_epilogue(hip, case)


@pytest.mark.parametrize("case", HEADS_CASES, ids=G.case_ids(HEADS_CASES))
def test_heads_epilogue_every_form(hip, case):  # noqa: F811
    """q | k | V^T, k | V^T and q alone into guarded segment buffers of their own: d = 40 (16-column blocks straddle heads, batch elements straddle row tiles) and d = 64 on the
    wide tiles, pack-first (key 15 = 1) and LDS-staged (key 15 = 2, key 13) forms, the narrow form (d = 12 with 77 tokens, key 7, f32); the pad columns [tokens, ld) of V^T
    and everything around a segment must stay as they were"""
    _run_epilogue(hip, case)


@pytest.mark.parametrize("case", ACT_CASES, ids=G.case_ids(ACT_CASES))
def test_activation_epilogue(hip, case):  # noqa: F811
    """erf-GELU and quick-GELU between bias and residual on the three tiles the family builds, narrow through an odd output pitch, f32"""
    _run_epilogue(hip, case)


@pytest.mark.parametrize("case", LNFOLD_CASES, ids=G.case_ids(LNFOLD_CASES))
def test_layernorm_fold_linear_epilogue(hip, case):  # noqa: F811
    """rows with |mean| / std up to 4: stored {mean, rstd} pairs (packed; narrow next to a residual; an odd M that loads them in the epilogue) and three partial sums per row"""
    _run_epilogue(hip, case)


@pytest.mark.parametrize("case", DUALK_CASES, ids=G.case_ids(DUALK_CASES))
def test_dual_source_k(hip, case):  # noqa: F811
    """A = [a | a2] with separate pitches: the switch after one 64-element K tile, and on the border of the second"""
    _run_epilogue(hip, case)


@pytest.mark.parametrize("case", T3_CASES, ids=G.case_ids(T3_CASES))
def test_t3_unsplit_every_tile(hip, case):  # noqa: F811
    """5 clips x 3 frames x 20 rows between NaN guard rows: a tap read across a clip border or past either end shows as a wrong or a non-finite element"""
    _run_epilogue(hip, case)


PLAIN_CASES, NARROW_CASES = G.by_group("plain"), G.by_group("narrow")
CONV_CASES, ALIAS_CASES, STRIPE_CASES, SPLITK_CASES = G.by_group("conv", "pixel"), G.by_group("alias"), G.by_group("stripes"), G.by_group("splitk")


@pytest.mark.parametrize("case", PLAIN_CASES, ids=G.case_ids(PLAIN_CASES))
def test_plain_packed_epilogue_every_tile(hip, case):  # noqa: F811
    """4.1: M = 300, N = 328, K = 136 - ragged in M, N and K for every tile - with bias, residual, out_scale, every pitch larger than its width, and the row bias
    absent / in staged groups of 96 rows read from inside a wider table / one group per row tile"""
    _run(hip, case)


@pytest.mark.parametrize("case", NARROW_CASES, ids=G.case_ids(NARROW_CASES))
def test_plain_narrow_epilogue_odd_pitches(hip, case):  # noqa: F811
    """4.2: the same problem with `out` one element off 16 bytes, ldo = 329 and ldrb = 331: the per-lane epilogue, on config 1 / 2 whatever is asked"""
    _run(hip, case)


@pytest.mark.parametrize("case", CONV_CASES, ids=G.case_ids(CONV_CASES))
def test_conv_every_tile_wide(hip, case):  # noqa: F811
    """4.3: 3 frames of 8 x 12 outputs (M = 288) from every geometry the engine issues - stride 1 / 2, pad 1 / 0, nearest-upsampled 2x and to a forwarded
    size - with one and two K slabs per tap, row bias per frame, residual; and 5 frames of a single pixel"""
    _run(hip, case)


@pytest.mark.parametrize("case", ALIAS_CASES, ids=G.case_ids(ALIAS_CASES))
def test_residual_aliasing_out(hip, case):  # noqa: F811
    """4.4: y = x I + y in place.  The wide epilogues read the residual and write `out` with different lane mappings: the in-place launch must equal
    the out-of-place one bit for bit"""
    ops, ref_buf, S = reference(case)
    in_place = check(case, ops, launch(hip, case, ops), ref_buf, S)
    y = ops.buf.cuda()                                       # the same y, read from a buffer of its own
    apart = launch(hip, case, ops, residual_buf=y).cpu()
    assert torch.equal(in_place.view(torch.int16), apart.view(torch.int16)), "the in-place add differs from the out-of-place one"
    assert torch.equal(y.cpu().view(torch.int16), ops.buf.view(torch.int16)), "the residual was written"


@pytest.mark.parametrize("case", STRIPE_CASES, ids=G.case_ids(STRIPE_CASES))
def test_batched_output_in_column_stripes(hip, case):  # noqa: F811
    """4.5: four heads write 40-column stripes of the same 40 rows (stride_o = d, ldo = C); the whole [40][160] buffer is compared"""
    assert case.cols == case.ldo
    _run(hip, case)


@pytest.mark.parametrize("case", SPLITK_CASES, ids=G.case_ids(SPLITK_CASES))
def test_split_k_finish_with_separate_pitches(hip, case):  # noqa: F811
    """4.6: a small problem made to split (fyc_set_tuning key 10 = 2), ldo = 336, ldr = 344, ldrb = 332: the finish kernels take the three pitches
    separately.  With chan_parts: the statistics against the sums of the values as stored, as test_gemm_split_k_output_statistics does"""
    c = case
    ops, ref_buf, S = reference(c)
    if not c.chan:
        check(c, ops, launch(hip, c, ops), ref_buf, S)
        return
    T = G.DT[c.dt]
    for k, v in c.all_tuning:
        hip.set_tuning(k, v)
    try:
        nt, tile_rows, slots = hip.gemm_stat_layout(T, M=c.M, N=c.N, K=c.K, cs_rows=c.cs_rows, mode=c.mode)
    finally:
        for k, _ in c.all_tuning:
            hip.set_tuning(k, 0)
    assert tile_rows == 128 and nt == (c.M + 127) // 128 and 1 <= slots <= 4, (nt, tile_rows, slots)
    parts = torch.full((nt * slots * c.N * 2,), float("nan"), device="cuda")
    got_buf = check(c, ops, launch(hip, c, ops, chan_parts=parts, cs_rows=c.cs_rows), ref_buf, S)
    cs = torch.zeros(c.M // c.cs_rows, c.N, 2, dtype=torch.float64, device="cuda")
    hip.chan_stats_reduce(parts, cs, rows=c.M, N=c.N, cs_rows=c.cs_rows, tile_rows=tile_rows, slots=slots)
    torch.cuda.synchronize()
    v = G.logical(c, got_buf).double().reshape(c.M // c.cs_rows, c.cs_rows, c.N)
    want = torch.stack([v.sum(dim=1), (v * v).sum(dim=1)], dim=-1)
    rel = ((cs.cpu() - want).norm() / want.norm()).item()
    assert rel <= 2e-6, f"{c.name}: channel statistics rel-L2 {rel:.3e} ({slots} slots)"
