"""The split-bf16 product rule of fyc_gemm for f32 operands (include/fyc.h: f32_products), without a GPU: the split itself, the specification emulator
against the bound the GPU cases are judged by (tests/f32x3_spec.py), the environment switches, what keyword, instance mode and dtype make of the field in each of the
tier's three entry points, and the argument check of the C entry point."""
import ctypes
import os

import pytest
import torch

import f32x3_spec as X
import gemm_cases as G
from kernel_compare import RTOL, Guard, compare


def _f32(values):
    return torch.tensor(values, dtype=torch.float64).float()


def _split_inputs():
    g = torch.Generator().manual_seed(11)
    rnd = torch.randn(4096, generator=g) * torch.exp2(torch.randint(-40, 40, (4096,), generator=g).float())
    pow2 = torch.exp2(torch.arange(-126, 128).float())
    # bf16 rounding ties: 8 significant bits + exactly half a unit of the 8th, and their f32 neighbours on either side (even and odd 8th bit)
    m = torch.arange(128, 256, dtype=torch.float64)
    tie = torch.cat([(m + 0.5) * 2.0 ** -7 + d for d in (0.0, 2.0 ** -23, -(2.0 ** -23))]).float()
    tiny = _f32([2.0 ** -126 * f for f in (1.0, 1.0 + 2.0 ** -23, 1.5, 1.0 + 2.0 ** -8 + 2.0 ** -9, 2.0 - 2.0 ** -23, 2.0 + 2.0 ** -22, 255.5, 256.0 + 2.0 ** -15)])
    named = _f32([1 + 2.0 ** -10 + 2.0 ** -20, 0.0, 1.0, 3.0, 1 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -23, 1 - 2.0 ** -24, 255.99999])
    x = torch.cat([rnd, pow2, tie, tie * 2.0 ** 40, tiny, named])
    return torch.cat([x, -x])


def test_split_is_exact_to_17_bits():
    """hi + lo is an f32 number (the kernel's accumulator holds it exactly when the weight is 1), and it is within 2^-17 of the power of two below |x|"""
    x = _split_inputs()
    hi, lo = X.split_bf16(x)
    for t in (hi, lo):
        assert torch.equal(t, t.to(torch.bfloat16).float())                     # both halves are bf16 numbers
    s64 = hi.double() + lo.double()
    assert torch.equal((hi + lo).double(), s64), "hi + lo is not exact in f32"
    assert torch.equal((x - hi).double(), x.double() - hi.double()), "x - hi is not exact in f32"
    # The remainder r = x - hi is at most half a unit of hi's 8th bit, 2^-8 p with p = 2^floor(log2 |x|).  At exactly 2^-8 p it is a power of two and lo = r; below it
    # the power of two under |r| is at most 2^-9 p and lo, r rounded to 8 bits, is off by at most 2^-8 of that:  |x - hi - lo| <= 2^-17 p  (<= 2^-17 |x|, and reached).
    # The 2^-18 |x| this rule was first written down with charges each rounding 2^-9 of the value, which holds just below a power of two only (582.06 = 0x1.2307b4p+9 is at 1.05 x 2^-18 |x|;
    # kernel_compare's docstring tells the same story about u and r).  Where r is a bf16 SUBNORMAL (spacing 2^-133; |x| < 2^-117) the floor is half that spacing:
    # 2^-126 (1 + 2^-8 + 2^-9) has r = -2^-135 and lo = 0.
    ax, err = x.double().abs(), (x.double() - s64).abs()
    p = torch.exp2(torch.floor(torch.log2(ax.clamp_min(2.0 ** -126))))
    bound = (2.0 ** -17 * p).clamp_min(2.0 ** -134)
    assert bool((err <= bound).all()), (err / bound).max().item()
    assert (err / bound).max().item() > 0.9, "the bound is not sharp on these inputs: is it the right one?"
    # powers of two and 8-bit numbers split to themselves and zero
    p = torch.exp2(torch.arange(-126, 128).float())
    hp, lp = X.split_bf16(p)
    assert torch.equal(hp, p) and not bool(lp.any())
    h1, l1 = X.split_bf16(_f32([1 + 2.0 ** -10 + 2.0 ** -20]))
    assert h1.item() == 1.0 and l1.item() == 2.0 ** -10
    hz, lz = X.split_bf16(torch.zeros(3))
    assert not bool(hz.any()) and not bool(lz.any())                             # the zero fill of a K tail splits to zeros


def test_split_of_non_finite_values():
    """an Inf keeps its hi half and its lo half is NaN (Inf - Inf): the rows and columns it touches come out non-finite, as include/fyc.h says"""
    hi, lo = X.split_bf16(torch.tensor([float("inf"), float("-inf"), float("nan")]))
    assert torch.isinf(hi[:2]).all() and torch.isnan(hi[2]) and torch.isnan(lo).all()


_refs = {}


def _reference(c):
    if c.name not in _refs:
        ops = G.operands(c)
        _refs[c.name] = (ops, G.run_emulator(c, ops, torch.float64), G.bound_terms(c, ops))
    return _refs[c.name]


@pytest.mark.parametrize("case", X.GEMM_CASES, ids=G.case_ids(X.GEMM_CASES))
def test_spec_emulator_inside_the_bound_gemm_cases(case):
    """the rule as specified, run in f32 on every GPU case, stays inside the bound the GPU is judged by - global rel-L2 <= 2e-5 included (compare's (b))"""
    c = case
    ops, ref_buf, S = _reference(c)
    buf = ops.buf.clone()
    a, w, out, kw = G.gemm_kwargs(c, ops, buf)
    X.SplitEmuOps().gemm(a, w, out, **kw)
    fig = compare(G.logical(c, buf), G.logical(c, ref_buf), dtype="f32", bound_terms=X.bound_for(S, c.K, G.tile_shape(c.want_cfg)), guard=Guard(ops.buf, buf, ops.mask), tag=c.name)
    assert fig["global_rel"] <= RTOL["f32"]
    assert fig["elem_ratio"] > 1e-4, "the split emulator reproduced the f64 reference: nothing was split"


@pytest.mark.parametrize("name", sorted(X.epilogue_cases()))
def test_spec_emulator_inside_the_bound_epilogue_cases(name):
    case = X.epilogue_cases()[name]
    ref = X.run_epilogue_case(G.emulator(torch.float64), case)
    got = X.run_epilogue_case(X.SplitEmuOps(), case)
    fig = compare(got, ref, dtype="f32", bound_terms=X.bound_for(X.epilogue_bound_terms(case), case["K"]), tag=name)
    assert fig["global_rel"] <= RTOL["f32"]


def test_split_emulator_with_identity_weight_returns_hi_plus_lo():
    """what the GPU test of the same name asserts bit for bit, on the specification: W = I makes the output hi(a) + lo(a), which is not a"""
    g = torch.Generator().manual_seed(5)
    a = torch.randn(40, 64, generator=g) * (1 + 2.0 ** -10 + 2.0 ** -20)
    out = torch.zeros(40, 64)
    X.SplitEmuOps().gemm(a, torch.eye(64), out, M=40, N=64, K=64, lda=64, ldw=64, ldo=64)
    hi, lo = X.split_bf16(a)
    assert torch.equal(out, hi + lo) and (out != a).float().mean().item() >= 0.5


# ---- environment ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,dtype,products", [({}, torch.bfloat16, "exact"), ({"FYC_COMPUTE_DTYPE": "f32"}, torch.float32, "exact"),
                                               ({"FYC_COMPUTE_DTYPE": "f32x3"}, torch.float32, "split"),
                                               ({"FYC_COMPUTE_DTYPE": "f32", "FYC_F32_PRODUCTS": "split"}, torch.float32, "split"),
                                               ({"FYC_COMPUTE_DTYPE": "f32x3", "FYC_F32_PRODUCTS": "exact"}, torch.float32, "exact"),
                                               ({"FYC_F32_PRODUCTS": "split"}, torch.bfloat16, "split")])
def test_environment_switches(monkeypatch, env, dtype, products):
    import followyourclick_amd as fyc
    for k in ("FYC_COMPUTE_DTYPE", "FYC_F32_PRODUCTS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert fyc.default_compute_dtype() == dtype and fyc.default_f32_products() == products


def test_environment_bad_values_raise(monkeypatch):
    import followyourclick_amd as fyc
    monkeypatch.setenv("FYC_F32_PRODUCTS", "f16")
    with pytest.raises(ValueError, match="FYC_F32_PRODUCTS"):
        fyc.default_f32_products()
    monkeypatch.delenv("FYC_F32_PRODUCTS")
    monkeypatch.setenv("FYC_COMPUTE_DTYPE", "f32x2")
    with pytest.raises(ValueError, match="f32x3"):
        fyc.default_compute_dtype()


def test_hipops_takes_the_mode_from_the_environment(monkeypatch):
    """HipOps.f32_products starts from default_f32_products(); set_f32_products changes it, forgets the cached plans and refuses other words"""
    from followyourclick_amd import ops
    monkeypatch.setenv("FYC_F32_PRODUCTS", "split")
    h = ops.HipOps()
    assert h.f32_products == "split"
    monkeypatch.delenv("FYC_F32_PRODUCTS")
    h = ops.HipOps()
    assert h.f32_products == "exact"
    h._ws_need["k"], h._q_cache["k"] = 1, 1
    h.set_f32_products("split")
    assert h.f32_products == "split" and not h._ws_need and not h._q_cache
    with pytest.raises(ValueError):
        h.set_f32_products("f16")


# ---- keyword, instance mode and dtype -> the field, for the three entry points of the tier ---------------------------------------------------------
# (f32 tensors?, `products` keyword, HipOps.f32_products) -> the f32_products field that reaches the library, or the exception.  attention() has no fused kernel
# with exact f32 products: where the table says 0 for f32 tensors it raises FycError instead.
_FIELD = {(True, None, "exact"): 0, (True, None, "split"): 1, (True, "exact", "exact"): 0, (True, "exact", "split"): 0, (True, "split", "exact"): 1, (True, "split", "split"): 1,
          (False, None, "exact"): 0, (False, None, "split"): 0, (False, "exact", "exact"): 0, (False, "exact", "split"): 0, (False, "split", "exact"): TypeError, (False, "split", "split"): TypeError,
          (True, "f16", "exact"): ValueError, (True, "f16", "split"): ValueError, (False, "f16", "exact"): ValueError, (False, "f16", "split"): ValueError}
# the smallest tensors each wrapper accepts: entry point -> (library function, dtype -> positional tensors, keywords)
_CALLS = {
    "gemm": ("fyc_gemm", lambda dt: (torch.zeros(8, 8, dtype=dt), torch.zeros(8, 8, dtype=dt), torch.zeros(8, 8, dtype=dt)), dict(M=8, N=8, K=8, lda=8, ldw=8, ldo=8)),
    "attention": ("fyc_attention", lambda dt: (torch.zeros(2, 8, dtype=dt), torch.zeros(8, 8, dtype=dt), torch.zeros(8, 8, dtype=dt), torch.zeros(2, 8, dtype=dt)),
                  dict(batch=1, heads=1, n_q=2, n_k=8, d=8, ldo=8, ldvt=8, scale=1.0)),
    "temporal_attention": ("fyc_temporal_attention", lambda dt: (torch.zeros(2, 24, dtype=dt), torch.zeros(2, 8, dtype=dt)), dict(clips=1, frames=2, pixels=1, heads=1, d=8, scale=1.0)),
}


@pytest.mark.parametrize("mode", ["exact", "split"])
@pytest.mark.parametrize("keyword", [None, "exact", "split", "f16"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("op", sorted(_CALLS))
def test_field_by_entry_point_dtype_keyword_and_mode(monkeypatch, op, dtype, keyword, mode):
    """one rule for gemm, attention and temporal_attention (ops.resolve_f32_products): what reaches the library, or what is raised before anything is called"""
    from followyourclick_amd import _lib
    monkeypatch.delenv("FYC_F32_PRODUCTS", raising=False)
    monkeypatch.delenv("FYC_COMPUTE_DTYPE", raising=False)
    h = X.hip_ops_recorder(monkeypatch)
    h.set_f32_products(mode)
    want = _FIELD[dtype == torch.float32, keyword, mode]
    if op == "attention" and dtype == torch.float32 and want == 0:
        want = _lib.FycError
    function, tensors, kw = _CALLS[op]
    if isinstance(want, int):
        getattr(h, op)(*tensors(dtype), products=keyword, **kw)
        (name, args), = h.calls
        assert name == function and args.f32_products == want and args.dtype == {torch.float32: _lib.FYC_F32, torch.bfloat16: _lib.FYC_BF16, torch.float16: _lib.FYC_F16}[dtype]
    else:
        with pytest.raises(want, match={ValueError: "products", TypeError: "split", _lib.FycError: "materialised"}[want]):
            getattr(h, op)(*tensors(dtype), products=keyword, **kw)
        assert not h.calls


# ---- the C entry point ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,products", [(1, 1), (2, 1), (0, 2), (1, 2), (0, -1)])
def test_bad_f32_products_are_refused_without_gpu(dtype, products):
    """f32_products = 1 with a 16-bit dtype, or a value other than 0 / 1: refused before anything is launched, the message names the field"""
    from followyourclick_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    lib = _lib.load()
    g = _lib.GemmArgs()
    g.M, g.N, g.K, g.lda, g.ldw, g.ldo, g.batch, g.out_scale = 128, 128, 64, 64, 64, 128, 1, 1.0
    g.a, g.w, g.out = 0x10000000, 0x20000000, 0x30000000
    g.dtype, g.f32_products = dtype, products
    assert lib.fyc_gemm(ctypes.byref(g), None) != 0
    assert b"f32_products" in lib.fyc_last_error()


def test_layout_queries_do_not_read_the_field():
    """both rules run the same tiles: the layout queries answer the same with the field set"""
    from followyourclick_amd import _lib
    lib = _lib.load()
    for M, N, K, cs_rows in ((300, 328, 136, 0), (1152, 128, 64, 192), (288, 328, 520, 96), (2048, 1280, 5120, 64)):
        ans = []
        for products in (0, 1):
            g = _lib.GemmArgs()
            g.M, g.N, g.K, g.batch, g.dtype, g.cs_rows, g.f32_products = M, N, K, 1, _lib.FYC_F32, cs_rows, products
            tr, sl = _lib.i32(0), _lib.i32(0)
            ans.append((lib.fyc_gemm_row_parts(ctypes.byref(g)), lib.fyc_gemm_workspace_bytes(ctypes.byref(g)),
                        lib.fyc_gemm_stat_layout(ctypes.byref(g), ctypes.byref(tr), ctypes.byref(sl)), tr.value, sl.value))
        assert ans[0] == ans[1], (M, N, K, ans)
        assert ans[0][1] == 0, "an f32 problem asked for split-K scratch"
