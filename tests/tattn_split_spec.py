"""Torch specification of fyc_temporal_attention's split-bf16 product rule for f32 tensors (include/fyc.h: fyc_tattn_args.f32_products =
FYC_PRODUCTS_SPLIT_BF16; HipOps.temporal_attention(products="split")), the cases of tests/test_tattn_split_gpu.py as data, and the per-element bound they
are judged by.  A helper, not a test module; no GPU is touched here.

The rule, with hi(x) = RNE_bf16(x), lo(x) = RNE_bf16(x - hi(x)) (tests/f32x3_spec.py: split_bf16, and split_product for the three-term products below):
  * q and k are taken as f32 and, with RoPE, rotated in f32 (two rounded products, one rounded sum); nothing is rounded to 16 bits before the split;
  * s[fq][fk] = sum_c hi(q) hi(k) + hi(q) lo(k) + lo(q) hi(k) in f32;
  * softmax in f32: max, exp2((s - max) * (scale * log2e)), f32 row sum; p is normalised by the row sum, then split;
  * o[fq][c] = sum_fk hi(p) hi(v) + hi(p) lo(v) + lo(p) hi(v) in f32, stored as f32.

The bound, against the f64 attention of the UNSPLIT operands, needs no measurement.  kernel_compare.softmax_bound_terms(dtype="f32", kind="temporal") is the
bound of an f32 evaluation whose q and k are uncertain by dq and dk; the split rule's score product is an f32 sum of 3 d exact products that is off from q.k by at
most PRODUCT sum |q||k| (the constants and their derivation: f32x3_spec's docstring; PRODUCT = 2^-15, OPERAND = 2^-16), which is what
    dq = OPERAND |q|,  dk = OPERAND |k|       (+ 3 u (|x cos| + |x' sin|) under RoPE, as attention_cases._temporal_reference charges the exact f32 kernel)
charge it: dq.|k| + |q|.dk + dq.dk >= PRODUCT sum |q||k|.  The P V product is off by at most PRODUCT sum_fk w |v| in the same way, and the reference is stored as f32:
    |got - ref| <= ulp_f32(ref) + rest(dq, dk) + PRODUCT (w @ |v|).
The global tolerance is the exact f32 kernel's, attention_cases.RTOL_TEMPORAL["f32"] = RTOL_TEMPORAL_ROPE["f32"] = 2e-5.
Exact f32 products pass this bound too: what tells the rules apart is a single-frame problem, where p = 1 and the split rule returns hi(v) + lo(v), not v.

Cases: every group-F temporal problem of tests/attention_cases.py (13 head dims x NFT 1..4 x RoPE off / on, P in {1, 5}, H in {1, 3, 8}, clips in {1, 2}: task
counts that fill and do not fill the last block), two more for the family that runs two tasks per block, and its group-E selection problems (F in {16, 17, 33, 64} x d in {16, 64, 104, 160}), taken from the bf16 list in f32.

Defects of the emulator (each must leave the bound wherever F > 1): "drop_q_lok" drops hi(q) lo(k), "drop_lop_v" drops lo(p) hi(v)."""
from dataclasses import replace

import numpy as np
import torch

import attention_cases as A
import f32x3_spec as X
import kernel_compare as KC
from followyourclick_amd.ops import resolve_f32_products
from rope_spec import RopeEmuOps, rotate_half

RTOL = {False: A.RTOL_TEMPORAL["f32"], True: A.RTOL_TEMPORAL_ROPE["f32"]}      # by RoPE
DEFECTS = X.ATTN_DEFECTS


def _in_f32(c):
    return replace(c, dt="f32", name=c.name.replace("-bf16-", "-f32split-"), rtol=RTOL[c.rope], defects=(), unchanged=())


FAMILY_CASES = [_in_f32(c) for c in A.by_group("temporal", "F") if c.dt == "bf16"]
SELECT_CASES = [_in_f32(c) for c in A.by_group("temporal", "E") if c.dt == "bf16"]
# (DP 160, NFT 4) is the one family whose blocks hold two tasks instead of four (csrc/temporal_attn_f32x3.hip: the V^T tiles of four do not fit a CU's LDS); the
# list above gives it even task counts only: one problem of three tasks, its last block half empty, with and without RoPE
TWO_TASK_CASES = [A.Temporal(f"X-f32split-d{d}-F{F}-P1-H3-c1{'-rope' if rope else ''}", "X", "f32", 1, F, 1, 3, d, rope, RTOL[rope]) for d, F, rope in ((160, 49, False), (136, 64, True))]
CASES = FAMILY_CASES + TWO_TASK_CASES + SELECT_CASES
assert len(FAMILY_CASES) == 104 and len(SELECT_CASES) == 16 and len({c.name for c in CASES}) == len(CASES)


def split_attention(q, k, v, *, scale, rope=None, defect=None):
    """the rule on q, k, v f32 [..][F][d] (rope: the (cos, sin) tables [F][d/2]) -> o f32 [..][F][d]"""
    assert q.dtype == k.dtype == v.dtype == torch.float32
    if rope is not None:
        cos, sin = (torch.cat((t, t), dim=-1).float() for t in rope)
        q, k = (t * cos + rotate_half(t) * sin for t in (q, k))
    drop_qk, drop_pv = X.ATTN_DROPS.get(defect, (None, None))
    s = X.split_product(q, k.transpose(-1, -2), drop=drop_qk)
    sl2e = float(np.float32(scale) * np.float32(1.44269504088896340736))
    p = torch.exp2((s - s.max(dim=-1, keepdim=True).values) * sl2e)
    p = p * (1.0 / p.sum(dim=-1, keepdim=True))
    return X.split_product(p, v, drop=drop_pv)


class SplitTAttnEmuOps(RopeEmuOps):
    """the op emulator whose temporal_attention takes `products` like HipOps': None = this instance's f32_products"""

    def __init__(self, acc=torch.float64, f32_products="exact"):
        super().__init__(acc=acc)
        self.f32_products = f32_products

    def temporal_attention(self, qkv, o, *, clips, frames, pixels, heads, d, scale, rope=None, products=None, defect=None):
        if resolve_f32_products("temporal_attention", qkv.dtype, products, self.f32_products) == 0:
            return super().temporal_attention(qkv, o, clips=clips, frames=frames, pixels=pixels, heads=heads, d=d, scale=scale, rope=rope)
        Cc = heads * d
        x = qkv.reshape(-1)[: clips * frames * pixels * 3 * Cc].reshape(clips, frames, pixels, 3, heads, d)
        q, k, v = (x[:, :, :, i].permute(0, 2, 3, 1, 4) for i in range(3))          # b p h f d
        O = split_attention(q, k, v, scale=scale, rope=rope, defect=defect).permute(0, 3, 1, 2, 4).reshape(clips * frames * pixels, Cc)
        o.reshape(-1)[: O.numel()].reshape(O.shape).copy_(O)


def emulate(c, ops, defect=None):
    """the specification on a case -> its guarded buffer (CPU)"""
    buf = ops.buf.clone()
    SplitTAttnEmuOps().temporal_attention(ops.qkv, A.out_view(c, buf), clips=c.clips, frames=c.F, pixels=c.P, heads=c.H, d=c.d, scale=c.scale, rope=ops.tables,
                                          products="split", defect=defect)
    return buf


def hi_plus_lo_of_v(c, ops):
    """what a single-frame problem returns in the split rule, [rows][cols]: hi(v) + lo(v)"""
    assert c.F == 1
    v = ops.qkv.reshape(c.rows, 3, c.cols)[:, 2]
    hi, lo = X.split_bf16(v.contiguous())
    return hi + lo, v


_refs = {}


def reference(c):
    """-> (ops, ref: the guarded buffer holding the f64 reference of the unsplit operands stored as f32, bound [rows][cols] f64); computed once per problem, never modified"""
    if c.problem in _refs:
        return _refs[c.problem]
    ops = A.operands(c)
    q, k, v = A._split(c, ops)
    dq, dk = X.OPERAND * q.double().abs(), X.OPERAND * k.double().abs()
    if c.rope:
        (q, mq), (k, mk) = (A._rotate(t.float(), *ops.tables) for t in (q, k))
        dq, dk = X.OPERAND * q.double().abs() + 3 * KC.U["f32"] * mq.double(), X.OPERAND * k.double().abs() + 3 * KC.U["f32"] * mk.double()
    o = torch.empty(c.clips, c.P, c.H, c.F, c.d, dtype=torch.float64)
    rest = torch.empty_like(o)
    for b in range(c.clips):
        for p in range(c.P):
            o[b, p], rest[b, p], w = KC.softmax_bound_terms(q[b, p].double(), k[b, p].double(), v[b, p].double(), scale=c.scale, dtype="f32", kind="temporal",
                                                            dq=dq[b, p], dk=dk[b, p])
            rest[b, p] += X.PRODUCT * (w @ v[b, p].double().abs())
    o, rest = (t.permute(0, 3, 1, 2, 4).reshape(c.rows, c.cols) for t in (o, rest))
    ref = ops.buf.clone()
    A.window(c, ref).copy_(o.float())
    _refs[c.problem] = (ops, ref, KC.ulp(A.window(c, ref).double(), "f32") + rest)
    return _refs[c.problem]
