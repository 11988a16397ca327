"""The split-bf16 product rule of fyc_attention for f32 tensors (include/fyc.h: fyc_attn_args.f32_products), without a GPU: the specification emulator against
the bound the GPU cases are judged by (tests/attn_split_spec.py), the two dropped-cross-product defects and the frozen maximum against the same bound, the one-key
identity, the argument checks of the Python and the C entry point, and the engine's call-time choice between the fused call and the materialised sequence."""
import ctypes
import os
from types import SimpleNamespace

import pytest
import torch

import attention_cases as A
import attn_split_spec as S
from f32x3_spec import hip_ops_recorder
from kernel_compare import Guard, compare


@pytest.mark.parametrize("lag", [0.0, 5.7])
@pytest.mark.parametrize("case", S.CASES, ids=A.case_ids(S.CASES))
def test_spec_emulator_inside_the_bound(case, lag):
    """the rule as specified, with the true row maximum and with one that lags it by 5.7 log2 units, on every GPU case: every element inside the bound, global rel-L2
    inside the case's tolerance, nothing outside the output written"""
    c = case
    ops, ref, bound = S.reference(c)
    got = S.emulate(c, ops, lag=lag)
    fig = compare(A.window(c, got), A.window(c, ref), dtype="f32", bound=bound, rtol=c.rtol, labels=S.labels(c), guard=Guard(ops.buf, got, ops.mask), tag=c.name)
    assert fig["elem_ratio"] <= 0.5      # (measured: 0.21 at most - a bound the emulator filled would leave the kernel's other summation order no room)


@pytest.mark.parametrize("case", S.by_group("D"), ids=A.case_ids(S.by_group("D")))
def test_group_d_tolerances_are_the_recorded_ones(case):
    """group D's tolerance is twice the emulator's own rel-L2 on the case: the recorded figure is what the emulator gives here"""
    c = case
    ops, ref, _ = S.reference(c)
    rel = S.rel_l2(c, S.emulate(c, ops), ref)
    assert c.rtol == 2 * S.D_SPEC_REL[c.name]
    assert abs(rel - S.D_SPEC_REL[c.name]) <= 0.01 * S.D_SPEC_REL[c.name], f"{c.name}: the emulator is at {rel:.3e}, the file records {S.D_SPEC_REL[c.name]:.3e}"


DEFECT_PAIRS = [(c, d) for c in S.CASES for d in c.defects + tuple(n for n, _ in c.unchanged)]


@pytest.mark.parametrize("case,defect", DEFECT_PAIRS, ids=[f"{c.name}-{d}" for c, d in DEFECT_PAIRS])
def test_defects_leave_the_bound(case, defect):
    """hi(q') lo(k) or lo(p) hi(v) dropped: an error of 2^-9 per product, outside the bound; where a case declares the defect `unchanged` (one key, selection) the
    output keeps its bits.  freeze_max: non-finite or outside the bound where 2^height overflows f32"""
    c = case
    ops, ref, bound = S.reference(c)
    got = A.window(c, S.emulate(c, ops, defect=defect))
    if defect in dict(c.unchanged):
        assert torch.equal(got.contiguous().view(torch.int32), A.window(c, S.emulate(c, ops)).contiguous().view(torch.int32))
        return
    over = torch.nan_to_num((got.double() - A.window(c, ref).double()).abs() / bound, nan=float("inf"))
    assert over.max().item() > 1.0, f"{c.name}: {defect} stays at {over.max().item():.3f} of the bound"


ONE_KEY = [c for c in S.CASES if c.n_k == 1]


@pytest.mark.parametrize("case", ONE_KEY, ids=A.case_ids(ONE_KEY))
def test_one_key_returns_hi_plus_lo(case):
    """what the GPU test of the split kernel asserts bit for bit, on the specification: n_k = 1 makes the output hi(v) + lo(v), which is not v"""
    c = case
    ops = S.reference(c)[0]
    want, v = S.hi_plus_lo_of_v(c, ops)
    got = A.window(c, S.emulate(c, ops))
    assert torch.equal(got.contiguous().view(torch.int32), want.view(torch.int32))
    assert (got != v).float().mean().item() >= 0.5


def test_case_list_reaches_every_instantiation():
    """every (DP32, DVT, QT) the library builds, each head dim 8 .. 160, ragged and full key tiles, one to nine ring stages, ragged and several query blocks, both block
    orders, the ring above and below 64 KB; pad keys that are finite after the split and Inf before it in attention_cases' own form"""
    t = [S.split_traits(c) for c in S.CASES]
    assert {x["instance"] for x in t} == S.built()
    assert {c.d for c in S.CASES} == set(range(8, 161, 8))
    assert {x["ragged_tile"] for x in t} == {True, False} and {x["tiles"] for x in t} >= {1, 2, 3, 4, 5, 9}
    assert {(x["instance"][2], x["query_blocks"], x["ragged_queries"]) for x in t} >= {(2, 2, True), (4, 1, True), (4, 2, True)}
    assert any(c.qt == 0 and S.effective_qt(c) == 4 for c in S.CASES) and any(c.qt == 0 and S.effective_qt(c) == 2 and c.d <= 80 for c in S.CASES)      # the dispatch's own rule, both ways
    assert {x["xcd"] for x in t} == {True, False} and {x["lds_bytes"] > 65536 for x in t} == {True, False}
    assert {c.accumulate for c in S.CASES} == {True, False} and {c.div for c in S.CASES} == {1, 2, 3} and {c.mod for c in S.CASES} == {0, 2}
    c = next(c for c in S.CASES if c.ldvt > c.n_k)
    pad = S.operands(c).vt[..., c.n_k:]
    assert torch.isfinite(pad.to(torch.bfloat16).float()).all() and pad.abs().min().item() == S.BF16_MAX
    assert not torch.isfinite(A.operands(c).vt[..., c.n_k:].to(torch.bfloat16).float()).any()


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------------
KW = dict(batch=1, heads=1, n_q=2, n_k=8, d=8, ldo=8, ldvt=8, scale=1.0)


def _tensors(dtype):
    return torch.zeros(2, 8, dtype=dtype), torch.zeros(8, 8, dtype=dtype), torch.zeros(8, 8, dtype=dtype), torch.zeros(2, 8, dtype=dtype)


def test_bad_products_are_refused_without_gpu():
    from followyourclick_amd import _lib, ops
    h = ops.HipOps()      # (not initialised: a check that came after ensure_init would raise FycError("no HIP device") here, there is no GPU)
    for dtype in (torch.float32, torch.bfloat16):
        with pytest.raises(ValueError, match="products"):
            h.attention(*_tensors(dtype), products="f16", **KW)
    for dtype in (torch.bfloat16, torch.float16):
        with pytest.raises(TypeError, match="split"):
            h.attention(*_tensors(dtype), products="split", **KW)
    h.set_f32_products("split")
    with pytest.raises(_lib.FycError, match="materialised"):
        h.attention(*_tensors(torch.float32), products="exact", **KW)
    h.set_f32_products("exact")
    with pytest.raises(_lib.FycError, match="materialised"):
        h.attention(*_tensors(torch.float32), **KW)


@pytest.mark.parametrize("dtype,products", [(1, 1), (2, 1), (0, 0), (0, 2), (1, 2), (0, -1)])
def test_bad_field_is_refused_by_the_library_without_gpu(dtype, products):
    """f32_products = 1 with a 16-bit dtype, 0 with FYC_F32, or a value other than 0 / 1: refused before anything that needs a device or fyc_init, the message names the
    field"""
    from followyourclick_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    lib = _lib.load()
    a = _lib.AttnArgs()
    a.q, a.k, a.vt, a.o = 0x10000000, 0x20000000, 0x30000000, 0x40000000
    a.batch, a.heads, a.n_q, a.n_k, a.d, a.ldo, a.ldvt, a.kv_batch_div, a.scale, a.o_scale = 1, 2, 64, 64, 40, 80, 64, 1, 1.0, 1.0
    a.dtype, a.f32_products = dtype, products
    assert lib.fyc_attention(ctypes.byref(a), None) != 0
    assert b"f32_products" in lib.fyc_last_error()


def test_the_field_follows_keyword_instance_and_dtype(monkeypatch):
    monkeypatch.delenv("FYC_F32_PRODUCTS", raising=False)
    monkeypatch.delenv("FYC_COMPUTE_DTYPE", raising=False)
    h = hip_ops_recorder(monkeypatch)
    assert h.f32_products == "exact"

    def field(dtype, **kw):
        h.attention(*_tensors(dtype), **KW, **kw)
        name, args = h.calls[-1]
        assert name == "fyc_attention"
        return args.f32_products
    assert field(torch.float32, products="split") == 1
    for dtype in (torch.bfloat16, torch.float16):
        assert field(dtype) == 0 and field(dtype, products="exact") == 0
    h.set_f32_products("split")
    assert field(torch.float32) == 1 and field(torch.float32, products="split") == 1
    for dtype in (torch.bfloat16, torch.float16):      # 16-bit tensors: 0 whatever the instance's mode
        assert field(dtype) == 0 and field(dtype, products="exact") == 0
    n = len(h.calls)
    with pytest.raises(Exception, match="materialised"):
        field(torch.float32, products="exact")
    assert len(h.calls) == n


def test_binding_mirrors_the_header():
    """the field is the struct's last and the version is the header's (tests/test_abi.py compiles the header against every struct's layout)"""
    from followyourclick_amd import _lib
    assert _lib.AttnArgs._fields_[-1] == ("f32_products", _lib.i32)
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "fyc.h")).read()
    assert f"#define FYC_VERSION {_lib.FYC_VERSION}\n" in header and _lib.FYC_VERSION >= 307
    assert header.index("int32_t f32_products;\n} fyc_attn_args;") > 0


# ---- the engine's choice -------------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """an `ops` that records the names and keywords of the calls _attend makes"""

    def __init__(self, f32_products=None):
        self.calls = []
        if f32_products is not None:
            self.f32_products = f32_products

    def __getattr__(self, name):
        if name.startswith("_") or name == "f32_products":
            raise AttributeError(name)
        return lambda *a, **kw: self.calls.append((name, kw))


def _attend(ops, dtype, accumulate=False):
    from followyourclick_amd.engine.unet3d import UNet3DEngine
    eng = SimpleNamespace(ops=ops, mat_attn=dtype == torch.float32, zeros=lambda *s, **k: torch.zeros(*s, dtype=dtype), new=lambda *s, **k: torch.empty(*s, dtype=dtype),
                          _axpy=lambda *a: ops.calls.append(("axpy", {})))
    B, H, N, nk, d = 2, 2, 16, 77, 8
    q, k, vt, out = torch.zeros(B, H, N, d, dtype=dtype), torch.zeros(1, H, nk, d, dtype=dtype), torch.zeros(1, H, d, 80, dtype=dtype), torch.zeros(B * N, H * d, dtype=dtype)
    UNet3DEngine._attend(eng, q, k, vt, out, batch=B, n_q=N, n_k=nk, d=d, ldvt=80, C=H * d, kv_div=2, accumulate=accumulate, o_scale=0.5)
    return ops.calls


MATERIALISED = ["gemm", "softmax_rows", "gemm"] * 2
MATERIALISED_ACC = ["gemm", "softmax_rows", "gemm", "axpy"] * 2


def test_attend_goes_fused_in_split_mode_only(monkeypatch):
    monkeypatch.delenv("FYC_F32_FLASH", raising=False)
    calls = _attend(_Recorder("split"), torch.float32)
    assert [n for n, _ in calls] == ["attention"]
    assert calls[0][1]["kv_batch_div"] == 2 and calls[0][1]["n_k"] == 77 and calls[0][1]["ldvt"] == 80 and not calls[0][1]["accumulate"]
    calls = _attend(_Recorder("split"), torch.float32, accumulate=True)
    assert [n for n, _ in calls] == ["attention"] and calls[0][1]["accumulate"] and calls[0][1]["o_scale"] == 0.5
    for ops in (_Recorder("exact"), _Recorder()):      # exact mode; an `ops` without the attribute (the emulators)
        assert [n for n, _ in _attend(ops, torch.float32)] == MATERIALISED
    assert [n for n, _ in _attend(_Recorder("exact"), torch.float32, accumulate=True)] == MATERIALISED_ACC
    for dtype in (torch.bfloat16, torch.float16):       # 16-bit tensors: the fused call whatever the mode
        for mode in ("exact", "split"):
            assert [n for n, _ in _attend(_Recorder(mode), dtype)] == ["attention"]


def test_attend_decides_at_call_time_and_honours_the_switch(monkeypatch):
    """the same engine object follows set_f32_products; FYC_F32_FLASH=0 keeps today's call list in split mode, with today's arguments"""
    monkeypatch.delenv("FYC_F32_FLASH", raising=False)
    ops = _Recorder("exact")
    assert [n for n, _ in _attend(ops, torch.float32)] == MATERIALISED
    ops.calls.clear()
    ops.f32_products = "split"
    assert [n for n, _ in _attend(ops, torch.float32)] == ["attention"]
    monkeypatch.setenv("FYC_F32_FLASH", "0")
    off = _attend(_Recorder("split"), torch.float32)
    exact = _attend(_Recorder("exact"), torch.float32)
    assert [n for n, _ in off] == MATERIALISED
    assert [(n, {k: v for k, v in kw.items()}) for n, kw in off] == [(n, {k: v for k, v in kw.items()}) for n, kw in exact]
    monkeypatch.setenv("FYC_F32_FLASH", "1")
    assert [n for n, _ in _attend(_Recorder("split"), torch.float32)] == ["attention"]
