"""Torch specification of what fyc_attention gained with ABI 308 - the causal mask and head dims above 160 (csrc/attention_wide.h) - the cases of
tests/test_attn_wide_gpu.py as data, and the per-element bounds they are judged by.  A helper, not a test module; no GPU is touched here.

The two rules are the ones include/fyc.h states per dtype family; the mask only removes keys:
  * 16-bit (T = bf16 / f16): q' = T(q * f32(scale * log2e)); t = q' . k in f32; keys j > i (causal) and j >= n_k are removed BEFORE the maximum; p = exp2(t - m) in f32
    with m the row maximum over the remaining keys or (lag > 0) up to 6 log2 units below it; p is rounded to T; O = sum_j T(p) v in f32, l = sum_j T(p) in f32;
    o = T(O * (1 / l)); accumulate: T(prev + o_scale * o).
  * tier (f32 tensors, split-bf16 products): tests/attn_split_spec.py's rule word for word (q' and k split, three-term products, p split unnormalised,
    l = sum hi(p) + lo(p)), with the same removal of keys.

Bounds, against plain f64 attention of the unrounded operands over the VISIBLE keys: kernel_compare.softmax_bound_terms (16-bit, kind "flash") and attn_split_spec's
form (tier: dq = OPERAND |q|, dk = OPERAND |k|, + (PRODUCT + REMAINDER) (w @ |v|) + 6 ln2 2^-24 (w @ |v| + |o|)), constants unchanged.  Causal rows are judged row by
row: row i is a problem of its own with the keys 0 .. i, which is exactly what the rule computes (a removed key has p = 0 exactly and adding 0 is exact), so the
bound of row i is the unmasked bound of that smaller problem, with n_k = i + 1 in the (n_k + 8) 2^-24 term.
Where the new kernel departs from the derivations of those two files, and why no term is added:
  * the head dim is walked in chunks of 128 channels, but a score is still ONE f32 accumulation chain over all d products (the chunks continue the same MFMA
    accumulator): d roundings, as charged;
  * l is added up on the VALU from the rounded p (per lane, then over the four lanes of a query column) instead of by a row of ones in the PV product: an f32 sum
    of the very same values with at most n_k / 4 + 2 additions on the path of a term - no more than the (n_k + 8) charged, and the weights still add up to 1;
  * there is no -m in a padding slot of the head dim (MSUB), so m is never rounded to T: one error source fewer;
  * O^T is produced 128 rows at a time from the same P fragments: every output element is still one chain over the keys.

The discriminating causal operands (recipe "discriminating"): q in [0.75, 1.25]^d, k_j = c_j * (1, .., 1) with c_j = j * step, step a power of two (every c_j is exact in T) chosen so that for every row every
removed score exceeds every kept one by at least 40 log2 units (asserted on the rounded operands by check_discriminating).  The unmasked f64 attention then puts
all weight of every row on the LAST key; a kernel that lets one removed key into the maximum or into l returns that key's value row instead of v_i."""
import math
from dataclasses import dataclass, replace

import numpy as np
import torch

import attention_cases as A
import attn_split_spec as S
import f32x3_spec as X
import kernel_compare as KC

CW, KB, NS = 128, 32, 4          # attention_wide.h: channels per chunk, keys per tile, ring stages
GAP = 40.0                       # log2 units between a removed and a kept score of the discriminating set


@dataclass(frozen=True)
class Wide:
    f: A.Flash                   # shapes, dtype, pitches, batch indexing, accumulate: attention_cases.Flash with its operands and guarded buffer
    causal: bool = False
    recipe: str = "random"       # "random": attention_cases' operands; "discriminating": see the module docstring

    @property
    def name(self):
        return self.f.name


def _rtol(dt, accumulate):
    if dt == "f32":
        return S.RTOL
    return (A.RTOL_FLASH_ACC if accumulate else A.RTOL_FLASH)[dt]


def _case(group, dt, B, H, n_q, n_k, d, *, causal=False, recipe="random", ldvt=0, **kw):
    ldvt = ldvt or (n_k + 7) // 8 * 8
    name = f"{group}-{dt}-d{d}-b{B}h{H}-nq{n_q}-nk{n_k}" + ("-causal" if causal else "") + ("-disc" if recipe == "discriminating" else "") + \
        ("-acc" if kw.get("accumulate") else "") + (f"-div{kw['div']}" if kw.get("div", 1) > 1 else "") + (f"-ldvt{ldvt}" if ldvt != (n_k + 7) // 8 * 8 else "")
    return Wide(A.Flash(name, group, dt, B, H, n_q, n_k, d, _rtol(dt, kw.get("accumulate", False)), ldvt=ldvt, **kw), causal, recipe)


DTS = ("bf16", "f16", "f32")
WIDE_D = (192, 256, 320, 512)
WIDE_SHAPES = ((1, 1), (17, 31), (64, 32), (65, 33), (150, 65), (81, 81))
WIDE_BH = ((1, 1), (2, 1), (1, 3))
CAUSAL_D = (8, 40, 64, 80, 160, 512)
CAUSAL_N = (1, 2, 16, 17, 32, 33, 77, 130)


def _cases():
    out = []
    # W: head dims above 160.  Every d x dtype at least twice, every (n_q, n_k) and every (batch, heads) with every dtype: a rotation, not the product
    for dt in DTS:
        for rep in range(2):
            for i, (n_q, n_k) in enumerate(WIDE_SHAPES):      # every shape twice per dtype, the head dims and the (batch, heads) pairs rotating under them
                B, H = WIDE_BH[(i + rep) % len(WIDE_BH)]
                out.append(_case("W", dt, B, H, n_q, n_k, WIDE_D[(i + 2 * rep) % len(WIDE_D)]))
    for dt in DTS:
        # the batch machinery at d = 512 and 320: accumulate with o_scale, kv_batch_div = 2, ldvt > n_k with finite pad keys (two pad chunks of 4 / one of 8), 8 (batch, head)
        # pairs (the XCD block order), two ragged query blocks of 64 queries at QT = 1 and three of 128 at QT = 2 (d = 256: 270 queries)
        out.append(_case("X", dt, 2, 1, 65, 33, 512, accumulate=True, o_scale=0.7))
        out.append(_case("X", dt, 3, 1, 17, 31, 320, div=2))
        out.append(_case("X", dt, 1, 1, 81, 81, 512, ldvt=96))
        out.append(_case("X", dt, 2, 4, 17, 65, 192))
        out.append(_case("X", dt, 1, 1, 270, 150, 256))
    # C: causal, d <= 160 and 512, every n of the list with every dtype, random and discriminating operands
    i = 0
    for d in CAUSAL_D:
        for dt in DTS:
            for rep in range(2):
                n = CAUSAL_N[i % len(CAUSAL_N)]
                B, H = WIDE_BH[i % len(WIDE_BH)]
                out.append(_case("C", dt, B, H, n, n, d, causal=True, recipe="random" if rep == 0 else "discriminating"))
                i += 3      # coprime to 8
    for dt in DTS:
        out.append(_case("C", dt, 2, 12, 77, 77, 64, causal=True))                            # the CLIP text tower's launch
        out.append(_case("C", dt, 1, 2, 130, 130, 64, causal=True, recipe="discriminating"))    # two query blocks: the second one's tiles, the first one's skipped
        out.append(_case("C", dt, 1, 1, 130, 130, 512, causal=True, recipe="discriminating"))  # three query blocks of 64 (QT = 1)
        out.append(_case("C", dt, 2, 1, 33, 33, 40, causal=True, accumulate=True, o_scale=-1.5))
        out.append(_case("C", dt, 1, 2, 65, 65, 320, causal=True))                             # 2.5 chunks with the mask: the causal instantiation of three chunks
    assert len({c.name for c in out}) == len(out)
    return out


CASES = _cases()


def by_group(*groups):
    return [c for c in CASES if c.f.group in groups]


def case_ids(cases):
    return [c.name for c in cases]


def traits(c):
    """what a case launches (attention_wide.h): instantiation (family, NC, CAUSAL, QT), key tiles visited by the LAST query block, ring units, query blocks"""
    f = c.f
    nc = (f.d + CW - 1) // CW
    qt = 1 if nc >= 3 else 2
    tiles = (f.n_k + KB - 1) // KB
    nqb = (f.n_q + 64 * qt - 1) // (64 * qt)
    first_block_tiles = min(tiles, (min(64 * qt, f.n_q) - 1) // KB + 1) if c.causal else tiles
    return dict(instance=(f.dt, nc, c.causal, qt), chunks=f.d / CW, tiles=tiles, ragged_tile=f.n_k % KB != 0, units=tiles * 2 * nc, skipped_tiles=tiles - first_block_tiles,
                query_blocks=nqb, ragged_queries=f.n_q % (64 * qt) != 0, xcd=(f.B * f.H) % 8 == 0, padded_step=f.d % 32 != 0)


def built():
    """every (family, NC, CAUSAL, QT) the three instantiation files build (run_wide_impl)"""
    return {(dt, nc, causal, 1 if nc >= 3 else 2) for dt in DTS for nc in (1, 2, 3, 4) for causal in (False, True) if causal or nc >= 2}      # d <= 128 without the mask: the kernels of ABI 307


def labels(c):
    f, qt = c.f, traits(c)["instance"][3]
    return KC.Labels(lambda i: f"batch {i // f.n_q}, query {i % f.n_q}: query block {i % f.n_q // (64 * qt)}, wave {i % f.n_q % (64 * qt) // (16 * qt)}, lane column {i % 16}",
                     lambda j: f"head {j // f.d}, channel {j % f.d}: chunk {j % f.d // CW}, 16-row block {j % CW // 16}, quad {j % 16 // 4}")


# ---- operands ------------------------------------------------------------------------------------------------------------------------------------
def operands(c):
    f = c.f
    ops = S.operands(f) if f.dt == "f32" else A.operands(f)
    if c.recipe == "discriminating":
        T = A.DT[f.dt]
        g = torch.Generator().manual_seed(A._seed(f) ^ 0x5EED)
        q = (0.75 + 0.5 * torch.rand(f.B, f.H, f.n_q, f.d, generator=g)).to(T)
        a_min = (q.double().sum(-1) * f.scale * KC.LOG2E).min().item()      # q_i . u in log2 units per unit of c, u = (1, .., 1)
        step = 2.0 ** math.ceil(math.log2(GAP / a_min))                      # a power of two: c_j = j * step is exact in bf16 / f16 / f32 for j < 256
        assert f.n_k <= 256
        k = (torch.arange(f.n_k, dtype=torch.float64) * step)[None, None, :, None].expand(f.kvB, f.H, f.n_k, f.d).to(T).contiguous()
        ops.q_full, ops.q, ops.k = q, q, k
    return ops


def check_discriminating(c, ops):
    """on the rounded operands, in f64: every removed score exceeds every kept score of its row by >= GAP log2 units; returns the smallest such excess"""
    f = c.f
    worst = math.inf
    for b in range(f.B):
        for h in range(f.H):
            t = (ops.q_full[b, h].double() @ ops.k[A.kv_of(f, b), h].double().T) * f.scale * KC.LOG2E
            for i in range(f.n_q - 1):
                worst = min(worst, (t[i, i + 1:].min() - t[i, : i + 1].max()).item())
    return worst


# ---- reference and bound ---------------------------------------------------------------------------------------------------------------------------
def _terms(c, q, k, v):
    """(o, rest) of one (batch, head) in f64: KC.softmax_bound_terms, for the tier with attn_split_spec's extra terms; causal: row by row on the keys 0 .. i"""
    f = c.f

    def one(q_, k_, v_):
        if f.dt != "f32":
            o, rest, _ = KC.softmax_bound_terms(q_, k_, v_, scale=f.scale, dtype=f.dt, kind="flash")
            return o, rest
        o, rest, w = KC.softmax_bound_terms(q_, k_, v_, scale=f.scale, dtype="f32", kind="flash", dq=X.OPERAND * q_.abs(), dk=X.OPERAND * k_.abs())
        wv = w @ v_.abs()
        return o, rest + (X.PRODUCT + X.REMAINDER) * wv + S.RESCALE_THR * KC.LN2 * 2.0 ** -24 * (wv + o.abs())
    if not c.causal:
        return one(q, k, v)
    rows = [one(q[i:i + 1], k[: i + 1], v[: i + 1]) for i in range(q.shape[0])]
    return torch.cat([r[0] for r in rows]), torch.cat([r[1] for r in rows])


_refs = {}


def reference(c):
    """-> (ops, ref: the guarded buffer holding the f64 reference rounded to the storage type, bound [rows][cols] f64); computed once per case, never modified"""
    if c in _refs:
        return _refs[c]
    f, T = c.f, A.DT[c.f.dt]
    ops = operands(c)
    o = torch.empty(f.B, f.n_q, f.H, f.d, dtype=torch.float64)
    rest = torch.empty_like(o)
    for b in range(f.B):
        for h in range(f.H):
            kv = A.kv_of(f, b)
            o[b, :, h], rest[b, :, h] = _terms(c, ops.q_full[A.q_of(f, b), h].double(), ops.k[kv, h].double(), ops.vt[kv, h, :, : f.n_k].double().T.contiguous())
    o, rest = o.reshape(f.rows, f.cols), rest.reshape(f.rows, f.cols)
    ref = ops.buf.clone()
    if f.accumulate:
        prev = A.window(f, ops.buf).double()
        A.window(f, ref).copy_((prev + f.o_scale * o).to(T))
        bound = KC.ulp(A.window(f, ref).double(), f.dt) + abs(f.o_scale) * rest + 2 * 2.0 ** -24 * (prev.abs() + abs(f.o_scale) * o.abs())
    else:
        A.window(f, ref).copy_(o.to(T))
        bound = KC.ulp(A.window(f, ref).double(), f.dt) + rest
    _refs[c] = (ops, ref, bound)
    return _refs[c]


def unmasked_reference(c, ops):
    """the f64 attention WITHOUT the mask, [rows][cols]: what a kernel that ignores `causal` computes"""
    f = c.f
    o = torch.empty(f.B, f.n_q, f.H, f.d, dtype=torch.float64)
    for b in range(f.B):
        for h in range(f.H):
            kv = A.kv_of(f, b)
            w = torch.softmax(ops.q_full[b, h].double() @ ops.k[kv, h].double().T * f.scale, dim=-1)
            o[b, :, h] = w @ ops.vt[kv, h, :, : f.n_k].double().T
    return o.reshape(f.rows, f.cols)


# ---- the two rules ----------------------------------------------------------------------------------------------------------------------------------
def _sl2e(scale):
    return float(np.float32(scale) * np.float32(1.44269504088896340736))


def _removed(n_q, n_k, causal):
    return (torch.arange(n_k)[None, :] > torch.arange(n_q)[:, None]) if causal else torch.zeros(n_q, n_k, dtype=torch.bool)


def rule_16bit(q, k, v, *, scale, causal=False, lag=0.0, defect=None):
    """q [..][n_q][d], k, v [..][n_k][d] of T -> o f32 [..][n_q][d] (before the store / accumulate).  defect "mask_after_max": the maximum is taken over all keys"""
    T = q.dtype
    qp = (q.float() * _sl2e(scale)).to(T)
    t = (qp.double() @ k.double().transpose(-1, -2)).float()
    gone = _removed(q.shape[-2], k.shape[-2], causal)
    m = (t if defect == "mask_after_max" else t.masked_fill(gone, -math.inf)).max(dim=-1, keepdim=True).values - lag
    p = torch.exp2(t.masked_fill(gone, -math.inf) - m).to(T)
    return (p.double() @ v.double()).float() * (1.0 / p.float().sum(dim=-1, keepdim=True))


def rule_tier(q, k, v, *, scale, causal=False, lag=0.0, defect=None):
    """attn_split_spec.split_flash with the removal of keys"""
    t = X.split_product(q * _sl2e(scale), k.transpose(-1, -2))
    gone = _removed(q.shape[-2], k.shape[-2], causal)
    m = (t if defect == "mask_after_max" else t.masked_fill(gone, -math.inf)).max(dim=-1, keepdim=True).values - lag
    p = torch.exp2(t.masked_fill(gone, -math.inf) - m)
    ph, pl = X.split_bf16(p)
    return X.split_product(p, v) * (1.0 / (ph + pl).sum(dim=-1, keepdim=True))


def attention_rule(q, k, vt, o, *, batch, heads, n_q, n_k, d, ldo, ldvt, scale, kv_batch_div=1, accumulate=False, o_scale=1.0, q_batch_mod=0, causal=False,
                   lag=0.0, defect=None):
    """one fyc_attention launch by the rules above, on CPU tensors laid out as the kernel's (tests/emu_ops_wide.py and emulate() share it)"""
    from emu_ops import _flat, _strided
    qB = q_batch_mod or batch
    Q = _flat(q)[: qB * heads * n_q * d].reshape(qB, heads, n_q, d)[torch.arange(batch) % qB]
    kvB = (batch + kv_batch_div - 1) // kv_batch_div
    idx = torch.arange(batch) // kv_batch_div
    K = _flat(k)[: kvB * heads * n_k * d].reshape(kvB, heads, n_k, d)[idx]
    V = _strided(_flat(vt), (kvB, heads, d, n_k), (heads * d * ldvt, d * ldvt, ldvt, 1), 0)[idx].transpose(-1, -2).contiguous()
    rule = rule_tier if q.dtype == torch.float32 else rule_16bit
    O = rule(Q, K, V, scale=scale, causal=causal, lag=lag, defect=defect).permute(0, 2, 1, 3).reshape(batch * n_q, heads * d)
    dst = _strided(_flat(o), (batch * n_q, heads * d), (ldo, 1), 0)
    if accumulate:
        O = dst.float() + torch.tensor(o_scale, dtype=torch.float32) * O      # in f32, one rounding to T at the store
    dst.copy_(O.to(q.dtype))


def emulate(c, ops, lag=0.0, defect=None):
    """the specification on a case -> its guarded buffer (CPU)"""
    f = c.f
    buf = ops.buf.clone()
    attention_rule(ops.q, ops.k, ops.vt, A.out_view(f, buf), batch=f.B, heads=f.H, n_q=f.n_q, n_k=f.n_k, d=f.d, ldo=f.ldo, ldvt=f.ldvt, scale=f.scale,
                   kv_batch_div=f.div, q_batch_mod=f.mod, accumulate=f.accumulate, o_scale=f.o_scale, causal=c.causal, lag=lag, defect=defect)
    return buf
