"""Torch specification of the split-bf16 product rule of the f32x3 tier (include/fyc.h: f32_products = FYC_PRODUCTS_SPLIT_BF16) - the one home of the rule in
torch: split_bf16, split_product and the three error constants below serve fyc_gemm's specification here and those of fyc_temporal_attention
(tests/tattn_split_spec.py) and fyc_attention (tests/attn_split_spec.py) - then fyc_gemm's GPU cases (tests/test_f32x3_gpu.py) as data and the per-element bound
they are judged by, and the HipOps recorder of the CPU tests of the three entry points.  A helper, not a test module; no GPU is touched here.

The rule: hi(x) = RNE_bf16(x), lo(x) = RNE_bf16(x - hi(x)) - the subtraction is exact in f32 - and
    acc += hi(a) hi(w) + hi(a) lo(w) + lo(a) hi(w)
in f32 (the three bf16 x bf16 products are exact in f32); lo(a) lo(w) is dropped.  The kernels' statements of it: csrc/split_bf16.h, csrc/gemm_kernel.h::Mma<f32x3_t>.
The constants the derivation below arrives at: REMAINDER = 2^-17 (|x - hi - lo| / |x|), PRODUCT = 2^-15 (one three-term product against a w), and
OPERAND = 2^-16 = PRODUCT / 2, the uncertainty charged to EACH of two operands so that their product is charged PRODUCT (the attention specs' dq, dk).

The bound, against the f64 reference of the UNSPLIT operands, is the one the feature was specified with:
    |got - ref| <= ulp_f32(ref) + (K + 8) 2^-24 S + 2^-16 S_aw,        S_aw = |out_scale| sum_k |a| |w|  <=  S
  * hi is x rounded to 8 significant bits, |x - hi| <= 2^-8 p with p the power of two at or below |x|, and lo is that remainder rounded to 8 bits again:
    |x - hi - lo| <= 2^-17 p <= 2^-17 |x|  (tests/test_f32x3.py; half a unit in the 8th place is 2^-9 of a value just below a power of two and 2^-8 of one just above);
  * a w - (hi_a hi_w + hi_a lo_w + lo_a hi_w) = (a - hi_a - lo_a) w + (hi_a + lo_a) (w - hi_w - lo_w) + lo_a lo_w <= (2^-17 + 2^-17 + 2^-16) |a| |w| = 2^-15 |a| |w|, the last term being
    the dropped product, <= 2^-8 |a| 2^-8 |w|.  A product reaches that only when both values lie just above a power of two and every rounding sits at half a unit; for
    a mantissa in the middle of its binade each term is half of it, and the remainders have either sign.  2^-16 S_aw is therefore half the worst case of a single
    product and is what a sum of K products of mixed mantissas stays far below: the specification emulator sits at 0.21 x the whole bound at K = 48, 0.11 x at
    K = 136 and below 0.04 x at K = 576 (tests/test_f32x3.py runs it on every GPU case), while a kernel that dropped one of the two cross products is off by 2^-9 |a w| per
    product, several times the bound at these K;
  * what is left is a sum of 3 K exact products accumulated in f32 by matrix instructions that add 32 at a time: fewer roundings on the path of a term than
    the sequential sum of K terms kernel_compare charges (K + 8) 2^-24 S for.
Since S_aw <= S the bound is handed to kernel_compare.compare as BoundTerms(S, K + 256, tile): 2^-16 = 256 2^-24.  The constant stays 1, like C_ACC.
Exact f32 products pass this bound too: what tells the two rules apart is the identity-weight test, not the bound."""
import math
from dataclasses import replace

import torch

import gemm_cases as G
from kernel_compare import BoundTerms
from tconv_spec import TconvEmuOps

LINEAR, GEGLU, HEADS = 0, 1, 2
REMAINDER, OPERAND, PRODUCT = 2.0 ** -17, 2.0 ** -16, 2.0 ** -15      # (module docstring)


def split_bf16(x):
    """(hi, lo) of an f32 tensor, both f32 tensors holding bf16 values"""
    assert x.dtype == torch.float32
    hi = x.to(torch.bfloat16).float()
    lo = (x - hi).to(torch.bfloat16).float()
    return hi, lo


def split_product(x, y_t, drop=None):
    """x @ y_t by the rule, f32: hi(x) lo(y) + lo(x) hi(y) + hi(x) hi(y), the two small terms first, as the kernels' matrix instructions add them
    (csrc/split_bf16.h::mma3 with y as the A operand).  drop = "hi_lo" / "lo_hi" leaves out hi(x) lo(y) / lo(x) hi(y): the defects the specs must catch."""
    assert drop in (None, "hi_lo", "lo_hi")
    (xh, xl), (yh, yl) = split_bf16(x), split_bf16(y_t)
    hi_lo, lo_hi = xh @ yl, xl @ yh
    small = lo_hi if drop == "hi_lo" else hi_lo if drop == "lo_hi" else hi_lo + lo_hi
    return small + xh @ yh


# the emulator defects of the two attention specs -> what their score product (x = q, y = k) and their P V product (x = p, y = v) leave out
ATTN_DEFECTS = ("drop_q_lok", "drop_lop_v")
ATTN_DROPS = {"drop_q_lok": ("hi_lo", None), "drop_lop_v": (None, "lo_hi")}


def hip_ops_recorder(monkeypatch):
    """a HipOps that launches nothing and takes CPU tensors: ensure_init is a no-op, _call keeps the argument struct in .calls"""
    from followyourclick_amd import ops
    monkeypatch.setattr(ops, "_p", lambda t: None if t is None else t.data_ptr())
    h = ops.HipOps()
    h.calls = []
    h.ensure_init = lambda device: None
    h._call = lambda name, args: h.calls.append((name, args))
    return h


class SplitEmuOps(TconvEmuOps):
    """the op emulator whose gemm forms its products by the split rule: the three partial products come from the emulator's own GEMM (so pitches, batch
    stripes, the dual-source A and the convolution gathers are the emulator's), are added in f32, and the sum goes through the emulator's epilogue once
    more as the operand of an identity-weight GEMM, which adds nothing but zeros to it"""

    def __init__(self):
        super().__init__(acc=torch.float32)

    def gemm(self, a, w, out, *, M, N, K, lda, ldw, batch=1, stride_a=0, stride_w=0, stride_o=0, mode=0, conv=None, a2=None, k_split=0, lda2=0, **epi):
        assert a.dtype == torch.float32 and w.dtype == torch.float32 and epi.get("ln_nparts", 0) == 0 and epi.get("row_parts") is None
        (ah, al), (wh, wl) = split_bf16(a), split_bf16(w)
        a2h, a2l = split_bf16(a2) if a2 is not None else (None, None)
        raw = dict(M=M, N=N, K=K, lda=lda, ldw=ldw, ldo=N, batch=batch, stride_a=stride_a, stride_w=stride_w, stride_o=M * N, mode=mode, conv=conv, k_split=k_split, lda2=lda2)
        acc = torch.zeros(batch, M, N)
        for x, x2, y in ((ah, a2h, wl), (al, a2l, wh), (ah, a2h, wh)):      # the order of Mma<f32x3_t>::mma
            part = torch.zeros(batch, M, N)
            super().gemm(x, y, part, a2=x2, **raw)
            acc = acc + part
        eye = torch.eye(N)
        for z in range(batch):
            o = out if out is None or batch == 1 else out.reshape(-1)[z * stride_o:]      # (EmuOps.gemm indexes its output from the start of what it is given)
            super().gemm(acc[z].contiguous(), eye, o, M=M, N=N, K=N, lda=N, ldw=N, **epi)


# ---- the GPU cases ------------------------------------------------------------------------------------------------------------------------
# The plan of an f32 problem reads neither `tile` nor fyc_set_tuning key 1 (csrc/gemm_plan.h: the narrow epilogue only exists for configs 1 and 2, and N picks
# between them: 128x128 where N is a multiple of 128, else 128x64).  Every case still runs with key 1 = 0 and = 1, as a caller who forces the tile would run
# it, and both must give the same bits; what really puts a case on config 1 is its N, so the plain and the convolution problem also come with N = 384.
def _gemm_cases():
    out = [c for c in G.CASES if c.dt == "f32" and (c.group in ("pixel", "stripes") or (c.group == "plain" and ("norb" in c.name or "rb96" in c.name))
                                                   or (c.group == "conv" and "-c64-" in c.name and any(g in c.name for g in ("s1p1", "s2p0", "up5x7"))))]
    wide = dict(N=384, ldo=392, ldr=400, want_cfg=1)
    out.append(replace(G.BY_NAME["plain-f32-t0r0-rb96"], name="plain-f32-n384-rb96", ldrb=388, **wide))
    out.append(replace(G.BY_NAME["conv-s1p1-c64-f32-t0r0"], name="conv-s1p1-c64-f32-n384", ldrb=388, **wide))
    # the frame-axis convolution: the problem of the split-K T3 case, in f32 (an f32 problem never splits K: see below)
    out.append(G.Case(name="t3-f32", group="t3", dt="f32", mode=G.T3, M=288, N=328, K=576, lda=192, ldw=584, ldo=336, ldr=344, residual=1, rowbias=True, rpb=96, ldrb=332,
                      rb_off=8, conv=(("Cin", 192), ("frames", 3), ("rows", 96)), want_cfg=2, want_ring=-1))
    return out


# Split-K: csrc/gemm_plan.h splits 16-bit problems only (`h16 && linear && ...`), so M 288, N 328, K 520 with fyc_set_tuning key 10 = 2 runs unsplit in f32,
# in either product rule, and fyc_gemm_workspace_bytes() is 0 for it (tests/test_f32x3_gpu.py asserts that): there is no f32 split-K case.
GEMM_CASES = _gemm_cases()
assert len({c.name for c in GEMM_CASES}) == len(GEMM_CASES)


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def epilogue_cases():
    """name -> (a, w, out buffers maker, kwargs): one case each of GEGLU, HEADS, LINEAR + GELU, the LayerNorm fold, chan_parts and the dual-source A, at the
    smallest f32 shapes tests/test_kernels_gpu.py uses for them.  Every value is a CPU f32 tensor; `outs()` makes fresh zeroed outputs."""
    cases = {}
    M, C = 200, 64                                                                              # test_gemm_geglu
    cases["geglu"] = dict(a=rnd((M, C), 1), w=rnd((8 * C, C), 2, 1 / 8), kw=dict(M=M, N=8 * C, K=C, lda=C, ldw=C, ldo=4 * C, epilogue=GEGLU, bias=rnd((8 * C,), 3)),
                          out=(M, 4 * C), K=C)
    tokens, heads, d = 64, 8, 8                                                                 # test_gemm_heads
    Ch, Mh = heads * d, 3 * tokens
    cases["heads"] = dict(a=rnd((Mh, 64), 1), w=rnd((3 * Ch, 64), 2, 1 / 8), kw=dict(M=Mh, N=3 * Ch, K=64, lda=64, ldw=64, epilogue=HEADS, bias=rnd((3 * Ch,), 3)),
                          heads=dict(seg_cols=Ch, heads=heads, tokens=tokens, transposed=[0, 0, 1], ld=[0, 0, tokens], Bn=3, d=d), K=64)
    M, N, K = 32, 64, 64                                                                        # test_gemm_activation
    cases["gelu"] = dict(a=rnd((M, K), 1), w=rnd((N, K), 2, 2 / math.sqrt(K)), kw=dict(M=M, N=N, K=K, lda=K, ldw=K, ldo=N, ldr=N, act=1, bias=rnd((N,), 3), residual=rnd((M, N), 4)),
                         out=(M, N), K=K)
    M, C = 77, 64                                                                               # test_gemm_layernorm_fold, "linear"
    x = rnd((M, C), 1) * 1.5 + 0.3
    gamma, beta = 1 + 0.2 * rnd((C,), 2), 0.1 * rnd((C,), 3)
    w, b = rnd((3 * C, C), 4, 1 / math.sqrt(C)), rnd((3 * C,), 5)
    wf = w * gamma[None, :]
    mean = x.mean(dim=1)
    st = torch.stack([mean, (x.var(dim=1, unbiased=False) + 1e-5).rsqrt()], dim=1).contiguous()
    cases["lnfold"] = dict(a=x, w=wf, kw=dict(M=M, N=3 * C, K=C, lda=C, ldw=C, ldo=3 * C, bias=w @ beta + b, ln_stats=st, ln_colsum=wf.sum(dim=1)), out=(M, 3 * C), K=C)
    M, N, K = 1152, 128, 64                                                                     # test_gemm_output_statistics: 192-row samples straddle the 128-row tiles
    cases["chan"] = dict(a=rnd((M, K), 1), w=rnd((N, K), 2, 1 / math.sqrt(K)), kw=dict(M=M, N=N, K=K, lda=K, ldw=K, ldo=N, out_scale=1.25, bias=rnd((N,), 3)),
                         out=(M, N), K=K, cs_rows=192)
    M, C = 300, 64                                                                              # test_gemm_dual_source_k
    cases["dual"] = dict(a=rnd((M, C), 1), a2=rnd((M, 4 * C), 2), w=rnd((C, 5 * C), 3, 1 / math.sqrt(5 * C)),
                         kw=dict(M=M, N=C, K=5 * C, lda=C, ldw=5 * C, ldo=C, ldr=C, k_split=C, lda2=4 * C, bias=rnd((C,), 4), residual=rnd((M, C), 5)), out=(M, C), K=5 * C)
    return cases


def run_epilogue_case(ops, case, *, to=lambda t: t, dtype=torch.float32, **extra):
    """one case of epilogue_cases() on `ops` (an emulator, or HipOps with to = .cuda()); returns the output as one [rows][columns] CPU tensor of `dtype`"""
    kw = {k: (to(v.to(dtype) if k == "residual" else v) if isinstance(v, torch.Tensor) else v) for k, v in case["kw"].items()}
    a, w = to(case["a"].to(dtype)), to(case["w"].to(dtype))
    if "a2" in case:
        kw["a2"] = to(case["a2"].to(dtype))
    if "heads" in case:
        h = case["heads"]
        outs = [to(torch.zeros(h["Bn"], h["heads"], h["tokens"], h["d"], dtype=dtype)), to(torch.zeros(h["Bn"], h["heads"], h["tokens"], h["d"], dtype=dtype)),
                to(torch.zeros(h["Bn"], h["heads"], h["d"], h["tokens"], dtype=dtype))]
        ops.gemm(a, w, None, heads=dict(seg_cols=h["seg_cols"], heads=h["heads"], tokens=h["tokens"], outs=outs, transposed=h["transposed"], ld=h["ld"]), **kw, **extra)
        rows = h["Bn"] * h["heads"] * h["tokens"]
        return torch.cat([outs[0].cpu().reshape(rows, h["d"]), outs[1].cpu().reshape(rows, h["d"]), outs[2].cpu().permute(0, 1, 3, 2).reshape(rows, h["d"])], dim=1)
    out = to(torch.zeros(case["out"], dtype=dtype))
    ops.gemm(a, w, out, **kw, **extra)
    return out.cpu()


def epilogue_bound_terms(case):
    """S of the bound for an epilogue case, [rows][columns] f64 in the layout run_epilogue_case returns: the magnitude of what the epilogue's last rounding
    acts on.  LINEAR (+ activation, + LayerNorm fold): sum |a||w| scaled by |rstd|, + |rstd mean colsum| + |bias| + |residual|, times |out_scale| - the
    activations are 1-Lipschitz up to 1.13 (GELU) and are charged 2 x their argument's terms.  GEGLU: value x GELU(gate), each factor carrying its own terms:
    |v| S_g 1.13 + S_v |gelu(g)| + S_v S_g, all f64."""
    kw = case["kw"]
    a = case["a"].double() if "a2" not in case else torch.cat([case["a"], case["a2"]], dim=1).double()
    w = case["w"].double()
    S = a.abs() @ w.abs().t()
    if "ln_stats" in kw:
        st, cs = kw["ln_stats"].double(), kw["ln_colsum"].double()
        S = st[:, 1:2].abs() * (S + st[:, 0:1].abs() * cs.abs()[None])
    if kw.get("bias") is not None:
        S = S + kw["bias"].double().abs()[None]
    ep = kw.get("epilogue", LINEAR)
    if ep == GEGLU:
        pre = a @ w.t() + kw["bias"].double()[None]
        M, N = pre.shape
        v, g = pre.reshape(M, N // 32, 2, 16)[:, :, 0], pre.reshape(M, N // 32, 2, 16)[:, :, 1]
        Sv, Sg = S.reshape(M, N // 32, 2, 16)[:, :, 0], S.reshape(M, N // 32, 2, 16)[:, :, 1]
        return (v.abs() * Sg * 1.13 + Sv * torch.nn.functional.gelu(g).abs() + Sv * Sg).reshape(M, N // 2)
    if kw.get("act", 0):
        S = 2 * S
    if kw.get("residual") is not None:
        S = S + kw["residual"].double().abs()
    S = S * abs(kw.get("out_scale", 1.0))
    if ep == HEADS:
        h = case["heads"]
        C, rows = h["seg_cols"], h["Bn"] * h["heads"] * h["tokens"]
        segs = [S[:, s * C:(s + 1) * C].reshape(h["Bn"], h["tokens"], h["heads"], h["d"]).permute(0, 2, 1, 3).reshape(rows, h["d"]) for s in range(3)]
        return torch.cat(segs, dim=1)
    return S


def bound_for(S, K, tile=(128, 64)):
    """the split rule's bound in the form kernel_compare.compare takes (module docstring)"""
    return BoundTerms(S, K + 256, tile)
