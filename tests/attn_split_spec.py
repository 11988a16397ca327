"""Torch specification of fyc_attention's split-bf16 product rule for f32 tensors (include/fyc.h: fyc_attn_args.f32_products = FYC_PRODUCTS_SPLIT_BF16;
HipOps.attention(products="split")), the cases of tests/test_attn_split_gpu.py as data, and the per-element bound they are judged by.  A helper, not a test
module; no GPU is touched here.

The rule, with hi(x) = RNE_bf16(x), lo(x) = RNE_bf16(x - hi(x)) (tests/f32x3_spec.py: split_bf16, and split_product for the three-term products below):
  * q' = q * f32(scale * log2e), one f32 rounding; q' and k are split, nothing is rounded to 16 bits before the split;
  * t[i][j] = sum_c hi(q') hi(k) + hi(q') lo(k) + lo(q') hi(k) in f32: the score in log2 units;
  * p = exp2(t - m) in f32; m is the row maximum, or (lag > 0) a value up to RESCALE_THR = 6 log2 units below it: where the kernel's running maximum ends up depends
    on the order of the keys; keys >= n_k have p = 0;
  * p is split UNNORMALISED: O[i][c] = sum_j hi(p) hi(v) + hi(p) lo(v) + lo(p) hi(v), l[i] = sum_j hi(p) + lo(p), both f32;
  * o = O * (1 / l) stored as f32; with accumulate: prev + o_scale * o in f32.

The bound, against the f64 attention of the UNSPLIT operands (kernel_compare.softmax_bound_terms: plain f64, no rounding of the weights), constant 1, with
f32x3_spec's PRODUCT = 2^-15, OPERAND = 2^-16 and REMAINDER = 2^-17 (derived in its docstring):
    |got - ref| <= ulp_f32(ref) + rest + (PRODUCT + REMAINDER) (w @ |v|) + 6 ln2 2^-24 (w @ |v| + |o|)
  * rest = softmax_bound_terms(dtype="f32", kind="flash", dq = OPERAND |q|, dk = OPERAND |k|): the bound of an f32 flash evaluation (weights unnormalised before l, so
    their error moves the output only along v_j - o; (d + 8) 2^-24 on the score sum, 4 u + 2 u |s - max| on the exponential, (n_k + 8) 2^-24 on the P V sum and the
    epilogue) whose q and k are uncertain by dq and dk.  The split score product is an f32 sum of 3 d exact products that is off from q'.k by at most
    PRODUCT sum |q'||k|, and dq.|k| + |q|.dk + dq.dk >= PRODUCT sum |q||k| charges exactly that.  The f32 roundings of q' = q sl2e and of sl2e itself are two of the "+ 8".
  * PRODUCT (w @ |v|): the three-term P V products, as for the score.
  * REMAINDER (w @ |v|): l is the sum of hi(p) + lo(p), each off from the p that the exponential produced by at most REMAINDER p: the normalisation is off by that much.
  * 6 ln2 2^-24 (w @ |v| + |o|), added here, not fitted: softmax_bound_terms charges the rounding of the subtraction in exp2(t - m) as 2 u |s - max| for m = the TRUE
    maximum.  The kernel's m may lag it by up to RESCALE_THR = 6 log2 units, so |t - m| is up to 6 larger and the rounded difference is off by up to 6 u more
    log2 units: a relative 6 ln2 u on a weight, different from key to key, so it does not cancel in the normalisation; sum_j w_j e_j (v_j - o) <= max |e| (w @ |v| + |o|).
    The products by alpha = exp2(m_old - m_new) when the maximum moves are one f32 rounding each of O and of l, at most (150 + 120) / 6 times in any case here: they are
    part of the (n_k + 8) roundings of the P V term, of which the matrix instructions (32 products per addition) use n_k / 32 * 3.
  * accumulate: attention_cases.reference's terms - rest and the terms above times |o_scale|, 2 2^-24 (|prev| + |o_scale o|) for the multiply-add, ulp of the result.
Exact f32 products pass this bound too: what tells the rules apart is n_k = 1, where p = l = 1 and the output is hi(v) + lo(v) bit for bit, not v.

Global rel-L2: attention_cases.RTOL_TEMPORAL["f32"] = 2e-5 for groups A, B, C, E.  Group D (scores offset by +-90 / +-120 log2 units, spikes of 40 / 150) is not held to
it: a 2^-18 relative error of the split on a score of 120 is several 1e-4 log2 units, and correct arithmetic is at 1e-4.  Its tolerance is TWICE the rel-L2 of this
file's emulator (lag 0) on the same case, computed on the CPU and recorded in D_SPEC_REL below (tests/test_attn_split.py recomputes them); the factor 2 is for the
kernel's other summation order and its lagging maximum.

Cases: the bf16 Flash cases of tests/attention_cases.py, groups A - E, taken in f32 (`replace`).  The split kernel (csrc/attention_f32x3.hip) has QT = 2 and, up to
d = 80, QT = 4 (tuning key 3 forces them; 3 is not built, those cases are left out); its key tiles are 32 keys for every head dim, and group B's key counts 1, 31,
32, 33, 63, 64, 65, 96, ... 257 sit on both sides of those edges and run one, two, three and more ring stages; 150 queries are a ragged block and 270 a full and a
ragged block of 64 QT queries at QT = 4 (group A); group X adds the one thing that list cannot reach, the dispatch choosing QT = 4 itself (n_q >= 2048).  Pad keys are overwritten with +- the largest bf16 number (attention_cases pads with +- the f32 maximum, whose hi is Inf).
split_traits() names the instantiation a case runs, as attention_cases.traits does for the 16-bit kernel.

Defects of the emulator: "drop_q_lok" drops hi(q') lo(k), "drop_lop_v" drops lo(p) hi(v) - each must leave the bound, except where they cannot change the output by
construction (n_k = 1: p = 1 has no lo half and the score does not matter; group E: p = 1 on the selected key, 2^-80 elsewhere, and q', k are exact in bf16);
"freeze_max" keeps the first 32-key block's maximum (attention_cases): visible where 2^height overflows f32, the spikes of 150."""
from dataclasses import replace

import numpy as np
import torch

import attention_cases as A
import f32x3_spec as X
import kernel_compare as KC
from emu_ops import EmuOps, _flat, _strided
from followyourclick_amd.ops import resolve_f32_products

RTOL = A.RTOL_TEMPORAL["f32"]
RESCALE_THR = 6.0
BF16_MAX = float(torch.finfo(torch.bfloat16).max)
DEFECTS = X.ATTN_DEFECTS
P_IS_ONE = "p = 1 on the only / the selected key (no lo half), and the score product decides nothing"

# rel-L2 of emulate(c) (lag 0) against the f64 reference on the group-D cases, computed on the CPU (tests/test_attn_split.py::test_group_d_tolerances_are_the_recorded_ones)
D_SPEC_REL = {
    "D-f32split-d40-offset-120": 1.048e-04,
    "D-f32split-d40-offset-90": 3.766e-05,
    "D-f32split-d40-offset+90": 4.149e-05,
    "D-f32split-d40-offset+120": 1.044e-04,
    "D-f32split-d40-spikes40": 6.901e-06,
    "D-f32split-d40-spikes150": 1.208e-05,
    "D-f32split-d64-offset-120": 8.365e-05,
    "D-f32split-d64-offset-90": 2.674e-05,
    "D-f32split-d64-offset+90": 2.486e-05,
    "D-f32split-d64-offset+120": 8.846e-05,
    "D-f32split-d64-spikes40": 6.147e-06,
    "D-f32split-d64-spikes150": 1.093e-05,
}


def _in_f32(c):
    name = c.name.replace("-bf16-", "-f32split-")
    rtol = 2 * D_SPEC_REL[name] if c.group == "D" else RTOL
    defects, unchanged = DEFECTS, ()
    if c.n_k == 1 or c.group == "E":
        defects, unchanged = (), tuple((d, P_IS_ONE) for d in DEFECTS)
    if c.recipe == "spikes" and c.param > 128:
        defects += ("freeze_max",)
    return replace(c, dt="f32", name=name, rtol=rtol, defects=defects, unchanged=unchanged)


BF16_CASES = [c for c in A.by_group("flash", "A", "B", "C", "D", "E") if c.dt == "bf16" and c.qt != 3]
# group X: what the 16-bit list does not reach - the dispatch's OWN choice of QT = 4 (from 2048 queries on; every QT = 4 case above forces it with tuning key 3):
# eight full blocks of 256 queries and a ragged ninth, two key tiles, the second ragged
AUTO_QT4 = [A.Flash("X-f32split-d40-nq2049-nk33-auto", "X", "f32", 1, 2, 2049, 33, 40, RTOL, ldvt=40, defects=DEFECTS)]
CASES = [_in_f32(c) for c in BF16_CASES] + AUTO_QT4
assert len({c.name for c in CASES}) == len(CASES)


def by_group(*groups):
    return [c for c in CASES if c.group in groups]


def effective_qt(c):
    """attention_f32x3.hip: `int qt = (p.d <= 80 && p.n_q >= 2048) ? 4 : 2;` then tuning key 3 if it is 2, or 4 with d <= 80"""
    qt = 4 if (c.d <= 80 and c.n_q >= 2048) else 2
    if c.qt == 2 or (c.qt == 4 and c.d <= 80):
        qt = c.qt
    return qt


def split_traits(c):
    dvt = (c.d + 15) // 16                              # switch ((p.d + 15) / 16): 16-row blocks of O^T
    dp32 = (dvt + 1) // 2                               # case 1, 2 -> 1; 3, 4 -> 2; 5, 6 -> 3; 7, 8 -> 4; 9, 10 -> 5 k-steps of 32 channels
    qt = effective_qt(c)
    loads = (32 * (dp32 * 8 + 1) + dvt * 128 + 255) // 256      # Geo::LOADS
    return dict(instance=(dp32, dvt, qt), padded=c.d != dp32 * 32, lds_bytes=3 * loads * 4096,      # Geo::LDS_BYTES; > 64 KB: rp::LdsAttr
                full_tiles=c.n_k // 32, ragged_tile=c.n_k % 32 != 0, tiles=(c.n_k + 31) // 32,   # nfull, ntiles
                query_blocks=(c.n_q + 64 * qt - 1) // (64 * qt), ragged_queries=c.n_q % (64 * qt) != 0, xcd=(c.B * c.H) % 8 == 0)


def built():
    """every (DP32, DVT, QT) of csrc/attention_f32x3.hip"""
    return {((dvt + 1) // 2, dvt, qt) for dvt in range(1, 11) for qt in ((2, 4) if dvt <= 5 else (2,))}


def labels(c):
    qt = effective_qt(c)
    return KC.Labels(lambda i: f"batch {i // c.n_q}, query {i % c.n_q}: query block {i % c.n_q // (64 * qt)}, wave {i % c.n_q % (64 * qt) // (16 * qt)}, "
                               f"tile {i % c.n_q % (16 * qt) // 16}, lane column {i % 16}",
                     lambda j: f"head {j // c.d}, channel {j % c.d}: 16-row block {j % c.d // 16}, quad {j % 16 // 4}")


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------------
def split_flash(q, k, v, *, scale, lag=0.0, defect=None):
    """the rule on q [..][n_q][d], k, v [..][n_k][d] f32 -> o f32 [..][n_q][d] (before accumulate)"""
    assert q.dtype == k.dtype == v.dtype == torch.float32
    sl2e = float(np.float32(scale) * np.float32(1.44269504088896340736))
    drop_qk, drop_pv = X.ATTN_DROPS.get(defect, (None, None))
    t = X.split_product(q * sl2e, k.transpose(-1, -2), drop=drop_qk)
    m = t[..., :32].max(dim=-1, keepdim=True).values if defect == "freeze_max" else t.max(dim=-1, keepdim=True).values - lag
    p = torch.exp2(t - m)
    ph, pl = X.split_bf16(p)
    return X.split_product(p, v, drop=drop_pv) * (1.0 / (ph + pl).sum(dim=-1, keepdim=True))


class SplitAttnEmuOps(EmuOps):
    """the op emulator whose attention takes `products` like HipOps': None = this instance's f32_products; f32 tensors run the split rule only"""

    def __init__(self, acc=torch.float64, f32_products="exact"):
        super().__init__(acc=acc)
        self.f32_products = f32_products

    def attention(self, q, k, vt, o, *, batch, heads, n_q, n_k, d, ldo, ldvt, scale, kv_batch_div=1, accumulate=False, o_scale=1.0, q_batch_mod=0, products=None,
                  defect=None, lag=0.0):
        resolve_f32_products("attention", q.dtype, products, self.f32_products, fused_exact=False)      # the refusals; what is left: 16-bit tensors, or f32 and "split"
        qB = q_batch_mod or batch
        Q = _flat(q)[: qB * heads * n_q * d].reshape(qB, heads, n_q, d)[torch.arange(batch) % qB]
        if q.dtype != torch.float32:
            return super().attention(Q.contiguous(), k, vt, o, batch=batch, heads=heads, n_q=n_q, n_k=n_k, d=d, ldo=ldo, ldvt=ldvt, scale=scale, kv_batch_div=kv_batch_div,
                                     accumulate=accumulate, o_scale=o_scale)
        kvB = (batch + kv_batch_div - 1) // kv_batch_div
        idx = torch.arange(batch) // kv_batch_div
        K = _flat(k)[: kvB * heads * n_k * d].reshape(kvB, heads, n_k, d)[idx]
        V = _strided(_flat(vt), (kvB, heads, d, n_k), (heads * d * ldvt, d * ldvt, ldvt, 1), 0)[idx].transpose(-1, -2).contiguous()
        O = split_flash(Q, K, V, scale=scale, lag=lag, defect=defect).permute(0, 2, 1, 3).reshape(batch * n_q, heads * d)
        dst = _strided(_flat(o), (batch * n_q, heads * d), (ldo, 1), 0)
        if accumulate:
            O = dst + torch.tensor(o_scale, dtype=torch.float32) * O
        dst.copy_(O)


# ---- operands, reference, bound ---------------------------------------------------------------------------------------------------------------------
_refs = {}


def operands(c):
    """attention_cases.operands in f32, the pad keys of vt overwritten with +- the largest bf16 number (finite after the split, as far from zero as that allows)"""
    ops = A.operands(replace(c, rtol=RTOL))      # (attention_cases seeds its generator from the whole case: the operands must not move with a tolerance that is derived from them)
    pad = c.ldvt - c.n_k
    if pad:
        ops.vt[..., c.n_k:] = torch.tensor([BF16_MAX, -BF16_MAX] * c.ldvt)[:pad]
        ops.pad_value = ops.vt[..., c.n_k]
    return ops


def reference(c):
    """-> (ops, ref: the guarded buffer holding the f64 reference of the unsplit operands stored as f32, bound [rows][cols] f64); computed once per problem, never modified"""
    if c.problem in _refs:
        return _refs[c.problem]
    ops = operands(c)
    o = torch.empty(c.B, c.n_q, c.H, c.d, dtype=torch.float64)
    rest = torch.empty_like(o)
    for b in range(c.B):
        for h in range(c.H):
            kv = A.kv_of(c, b)
            q, k, v = ops.q_full[A.q_of(c, b), h].double(), ops.k[kv, h].double(), ops.vt[kv, h, :, : c.n_k].double().T.contiguous()
            ob, rb, w = KC.softmax_bound_terms(q, k, v, scale=c.scale, dtype="f32", kind="flash", dq=X.OPERAND * q.abs(), dk=X.OPERAND * k.abs())
            wv = w @ v.abs()
            o[b, :, h], rest[b, :, h] = ob, rb + (X.PRODUCT + X.REMAINDER) * wv + RESCALE_THR * KC.LN2 * 2.0 ** -24 * (wv + ob.abs())
    o, rest = o.reshape(c.rows, c.cols), rest.reshape(c.rows, c.cols)
    ref = ops.buf.clone()
    if c.accumulate:
        prev = A.window(c, ops.buf).double()
        A.window(c, ref).copy_((prev + c.o_scale * o).float())
        bound = KC.ulp(A.window(c, ref).double(), "f32") + abs(c.o_scale) * rest + 2 * 2.0 ** -24 * (prev.abs() + abs(c.o_scale) * o.abs())
    else:
        A.window(c, ref).copy_(o.float())
        bound = KC.ulp(A.window(c, ref).double(), "f32") + rest
    _refs[c.problem] = (ops, ref, bound)
    return _refs[c.problem]


def materialised_bound(c):
    """the bound of the MATERIALISED sequence with split products (score GEMM, fyc_softmax_rows, P V GEMM: engine/unet3d.py::_attend) against the same reference:
    tattn_split_spec's form - the weights are normalised in f32 BEFORE they are split, so their error acts on |v_j|, not on |v_j - o| (kind="temporal"), and there is
    neither a lagging maximum nor an l made of split halves:  ulp_f32(ref) + rest_temporal(dq, dk) + 2^-15 (w @ |v|), with accumulate's terms as above"""
    ops, ref, _ = reference(c)
    rest = torch.empty(c.B, c.n_q, c.H, c.d, dtype=torch.float64)
    o = torch.empty_like(rest)
    for b in range(c.B):
        for h in range(c.H):
            kv = A.kv_of(c, b)
            q, k, v = ops.q_full[A.q_of(c, b), h].double(), ops.k[kv, h].double(), ops.vt[kv, h, :, : c.n_k].double().T.contiguous()
            o[b, :, h], rb, w = KC.softmax_bound_terms(q, k, v, scale=c.scale, dtype="f32", kind="temporal", dq=X.OPERAND * q.abs(), dk=X.OPERAND * k.abs())
            rest[b, :, h] = rb + X.PRODUCT * (w @ v.abs())
    o, rest = o.reshape(c.rows, c.cols), rest.reshape(c.rows, c.cols)
    if c.accumulate:
        prev = A.window(c, ops.buf).double()
        return KC.ulp(A.window(c, ref).double(), "f32") + abs(c.o_scale) * rest + 2 * 2.0 ** -24 * (prev.abs() + abs(c.o_scale) * o.abs())
    return KC.ulp(A.window(c, ref).double(), "f32") + rest


def emulate(c, ops, defect=None, lag=0.0):
    """the specification on a case -> its guarded buffer (CPU)"""
    buf = ops.buf.clone()
    SplitAttnEmuOps().attention(ops.q, ops.k, ops.vt, A.out_view(c, buf), batch=c.B, heads=c.H, n_q=c.n_q, n_k=c.n_k, d=c.d, ldo=c.ldo, ldvt=c.ldvt, scale=c.scale,
                                kv_batch_div=c.div, q_batch_mod=c.mod, accumulate=c.accumulate, o_scale=c.o_scale, products="split", defect=defect, lag=lag)
    return buf


def hi_plus_lo_of_v(c, ops):
    """what a one-key problem returns in the split rule, [rows][cols]: hi(v) + lo(v) of the only key, for every query; and v itself"""
    assert c.n_k == 1 and not c.accumulate
    v = torch.stack([ops.vt[A.kv_of(c, b), :, :, 0] for b in range(c.B)])[:, None].expand(c.B, c.n_q, c.H, c.d).reshape(c.rows, c.cols).contiguous()
    hi, lo = X.split_bf16(v)
    return hi + lo, v


def rel_l2(c, got, ref):
    g, r = A.window(c, got).double(), A.window(c, ref).double()
    return ((g - r).norm() / r.norm()).item()
