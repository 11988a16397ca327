"""The split-bf16 product rule of fyc_temporal_attention for f32 tensors (include/fyc.h: fyc_tattn_args.f32_products), without a GPU: the specification
emulator against the bound the GPU cases are judged by (tests/tattn_split_spec.py), the two dropped-cross-product defects against the same bound, the
single-frame identity, the argument checks of the Python and the C entry point, and the environment switches."""
import ctypes
import os
from dataclasses import replace

import pytest
import torch

import attention_cases as A
import tattn_split_spec as S
from f32x3_spec import hip_ops_recorder
from kernel_compare import Guard, compare


@pytest.mark.parametrize("case", S.CASES, ids=A.case_ids(S.CASES))
def test_spec_emulator_inside_the_bound(case):
    """the rule as specified, run in f32 on every GPU case: every element inside the bound, global rel-L2 <= 2e-5, nothing outside the output written"""
    c = case
    ops, ref, bound = S.reference(c)
    got = S.emulate(c, ops)
    fig = compare(A.window(c, got), A.window(c, ref), dtype="f32", bound=bound, rtol=c.rtol, labels=A.labels(c), guard=Guard(ops.buf, got, ops.mask), tag=c.name)
    assert fig["global_rel"] <= 2e-5


@pytest.mark.parametrize("defect", S.DEFECTS)
@pytest.mark.parametrize("case", S.FAMILY_CASES + S.TWO_TASK_CASES, ids=A.case_ids(S.FAMILY_CASES + S.TWO_TASK_CASES))
def test_dropped_cross_product_leaves_the_bound(case, defect):
    """hi(q) lo(k) or lo(p) hi(v) dropped: an error of 2^-9 per product, outside the bound wherever there is more than one frame; with one frame p = 1 has no lo
    half and the scores do not matter: the output is unchanged bit for bit"""
    c = case
    ops, ref, bound = S.reference(c)
    got = A.window(c, S.emulate(c, ops, defect=defect))
    if c.F == 1:
        assert torch.equal(got.view(torch.int32), A.window(c, S.emulate(c, ops)).view(torch.int32))
        return
    over = (got.double() - A.window(c, ref).double()).abs() / bound
    assert over.max().item() > 1.0, f"{c.name}: {defect} stays at {over.max().item():.3f} of the bound"


ONE_FRAME = [c for c in S.FAMILY_CASES if c.F == 1]


@pytest.mark.parametrize("case", ONE_FRAME, ids=A.case_ids(ONE_FRAME))
def test_one_frame_returns_hi_plus_lo(case):
    """what the GPU test of the split kernel asserts bit for bit, on the specification: F = 1 makes the output hi(v) + lo(v), which is not v"""
    c = case
    ops = S.reference(c)[0]
    want, v = S.hi_plus_lo_of_v(c, ops)
    got = A.window(c, S.emulate(c, ops))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert (got != v).float().mean().item() >= 0.5
    exact = ops.buf.clone()
    S.SplitTAttnEmuOps().temporal_attention(ops.qkv, A.out_view(c, exact), clips=c.clips, frames=c.F, pixels=c.P, heads=c.H, d=c.d, scale=c.scale, rope=ops.tables)
    assert torch.equal(A.window(c, exact).view(torch.int32), v.contiguous().view(torch.int32))


def test_case_list_reaches_every_family():
    """13 head dims, every (DP, DVT) family of launch_d with NFT = 1 .. 4 and RoPE off and on; full and ragged last blocks"""
    reached = set()
    for c in S.FAMILY_CASES:
        t = A.ttraits(replace(c, dt="bf16"))      # the split kernel keeps the 16-bit kernel's families
        reached.add((t["family"], t["nft"], c.rope))
    assert reached == {((dp, dvt), nft, rope) for _, dp, dvt in A.FAMILIES for nft in (1, 2, 3, 4) for rope in (False, True)}
    assert {(c.clips * c.P * c.H) % 4 == 0 for c in S.FAMILY_CASES} == {True, False}
    assert {(c.clips * c.P * c.H) % 2 == 0 for c in S.FAMILY_CASES + S.TWO_TASK_CASES if c.d > 128 and c.F > 48} == {True, False}      # the two-task blocks of (DP 160, NFT 4)
    assert {(c.F, c.d) for c in S.SELECT_CASES} == {(F, d) for F in (16, 17, 33, 64) for d in (16, 64, 104, 160)}


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------------
KW = dict(clips=1, frames=2, pixels=1, heads=1, d=8, scale=1.0)


def _tensors(dtype):
    return torch.zeros(2, 24, dtype=dtype), torch.zeros(2, 8, dtype=dtype)


def test_bad_products_are_refused_without_gpu():
    from followyourclick_amd import ops
    h = ops.HipOps()      # (not initialised: a check that came after ensure_init would raise FycError here, there is no GPU)
    for dtype in (torch.float32, torch.bfloat16):
        with pytest.raises(ValueError, match="products"):
            h.temporal_attention(*_tensors(dtype), products="f16", **KW)
    for dtype in (torch.bfloat16, torch.float16):
        with pytest.raises(TypeError, match="split"):
            h.temporal_attention(*_tensors(dtype), products="split", **KW)


@pytest.mark.parametrize("dtype,products", [(1, 1), (2, 1), (0, 2), (1, 2), (0, -1)])
def test_bad_f32_products_are_refused_by_the_library_without_gpu(dtype, products):
    """f32_products = 1 with a 16-bit dtype, or a value other than 0 / 1: refused before anything is launched, the message names the field"""
    from followyourclick_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    lib = _lib.load()
    a = _lib.TAttnArgs()
    a.qkv, a.o = 0x10000000, 0x20000000
    a.clips, a.frames, a.pixels, a.heads, a.d, a.scale = 1, 16, 4, 2, 40, 1.0
    a.dtype, a.f32_products = dtype, products
    assert lib.fyc_temporal_attention(ctypes.byref(a), None) != 0
    assert b"f32_products" in lib.fyc_last_error()


def test_the_field_follows_keyword_instance_and_dtype(monkeypatch):
    monkeypatch.delenv("FYC_F32_PRODUCTS", raising=False)
    monkeypatch.delenv("FYC_COMPUTE_DTYPE", raising=False)
    h = hip_ops_recorder(monkeypatch)
    assert h.f32_products == "exact"

    def field(dtype, **kw):
        h.temporal_attention(*_tensors(dtype), **KW, **kw)
        name, args = h.calls[-1]
        assert name == "fyc_temporal_attention"
        return args.f32_products
    assert field(torch.float32) == 0 and field(torch.float32, products="exact") == 0 and field(torch.float32, products="split") == 1
    h.set_f32_products("split")
    assert field(torch.float32) == 1 and field(torch.float32, products="exact") == 0 and field(torch.float32, products="split") == 1
    for dtype in (torch.bfloat16, torch.float16):      # 16-bit tensors: 0 whatever the instance's mode
        assert field(dtype) == 0 and field(dtype, products="exact") == 0


@pytest.mark.parametrize("env,want", [({}, 0), ({"FYC_F32_PRODUCTS": "split"}, 1), ({"FYC_COMPUTE_DTYPE": "f32x3"}, 1), ({"FYC_COMPUTE_DTYPE": "f32"}, 0),
                                      ({"FYC_COMPUTE_DTYPE": "f32x3", "FYC_F32_PRODUCTS": "exact"}, 0)])
def test_environment_switches_set_the_mode_temporal_attention_uses(monkeypatch, env, want):
    for k in ("FYC_COMPUTE_DTYPE", "FYC_F32_PRODUCTS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h = hip_ops_recorder(monkeypatch)
    h.temporal_attention(*_tensors(torch.float32), **KW)
    assert h.calls[-1][1].f32_products == want
    h.temporal_attention(*_tensors(torch.bfloat16), **KW)
    assert h.calls[-1][1].f32_products == 0


def test_binding_mirrors_the_header():
    """the field is the struct's last and the version is the header's (tests/test_abi.py compiles the header against every struct's layout)"""
    from followyourclick_amd import _lib
    assert _lib.TAttnArgs._fields_[-1] == ("f32_products", _lib.i32)
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "fyc.h")).read()
    assert f"#define FYC_VERSION {_lib.FYC_VERSION}\n" in header and _lib.FYC_VERSION >= 306
    assert header.index("int32_t f32_products;\n} fyc_tattn_args;") > 0
