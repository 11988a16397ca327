"""The fyc_attention and fyc_temporal_attention cases of tests/test_attention_bounds_gpu.py as data: what each of them launches, its operands from a
seeded generator, its plain f64 reference with the per-element bound of tests/kernel_compare.py, and a torch model of each kernel's rounding points
with the defects that the bound is there to catch.  A helper, not a test module; no GPU is touched here.

Three users share the list:
  * tests/test_attention_cases.py (CPU) asserts through traits() / ttraits() that the list reaches every instantiation the library builds and every
    compile-time path of the kernel template, that the models stay inside the bound and that every declared defect leaves it;
  * tests/test_attention_bounds_gpu.py launches the cases into guarded buffers;
  * the figures of profiles/attention_bound_coverage.txt are keyed by the case names.

traits() restates the compile-time choices of csrc/attention_kernel.h from (d, n_q, n_k, QT) as a reader understands them; each line names the line it
mirrors.  Nothing here is computed by a copy of the kernel.

Defects (apply to the model's output; a case lists the ones that must leave its bound in `defects`, and the ones that cannot change its output BY
CONSTRUCTION in `unchanged`, with the reason - tests/test_attention_cases.py checks both claims):
  drop_heaviest   the heaviest key of one query is dropped            swap_rows    two adjacent query rows are swapped
  drop_last_key   key n_k - 1 is dropped (a tail mask one key short)  shift_head   one head's stripe holds the next head's output
  pad_key         one pad key is counted: zero K row, vt's pad value  ignore_div   kv_batch_div is ignored for batch element 1
  freeze_max      the running max stays what the first block made it  ignore_mod   q_batch_mod is ignored
  scale_prev      o_scale multiplies the previous value instead
  temporal: mask_last (the last frame is masked), rope_sign (the sign of the sine term flipped in the upper half), rope_next_q (the query rotated
  with the tables of frame f + 1; rotating q AND k with the next frame's tables leaves every score unchanged - RoPE scores depend on f - g only -
  so that form of the defect cannot be seen by any test of the attention core).
"""
import math
from dataclasses import dataclass, replace
from types import SimpleNamespace
from typing import Tuple

import numpy as np
import torch

import kernel_compare as KC
import rope_spec

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
FRONT = 64                   # guard elements in front of `o`
BACK_ROWS = 2                # flash: guard rows behind it (temporal: one row block of P rows)
FILL = {2: 0x7B7B, 4: 0x7B7B7B7B}      # prefill bit pattern: finite (3.3e36 in bf16, 61280 in f16, 1.3e36 in f32), no NaN, unlikely as an output
TUNE_ATTN_VARIANT = 3        # fyc_set_tuning key: 16-query tiles per wave (QT)
# the global tolerances of the existing tests of the same op (test_kernels_gpu.py, test_kernels_f16_gpu.py, test_rope_gpu.py)
RTOL_FLASH = {"bf16": 6e-3, "f16": 1.5e-3}                    # test_attention, test_attention_every_head_dim (_f16)
RTOL_FLASH_ACC = {"bf16": 8e-3, "f16": 2e-3}                  # their accumulate halves; the offset / spike tests
RTOL_TEMPORAL = {"bf16": 6e-3, "f16": 1.5e-3, "f32": 2e-5}    # test_temporal_attention (_f16)
RTOL_TEMPORAL_ROPE = {"bf16": 6e-3, "f16": 6e-3, "f32": 2e-5}  # test_rope_gpu.py::RTOL


@dataclass(frozen=True)
class Flash:
    name: str
    group: str                      # "A" head dims, "B" key tails, "C" batch indexing, "D" scores, "E" selection
    dt: str
    B: int
    H: int
    n_q: int
    n_k: int
    d: int
    rtol: float
    qt: int = 0                     # tuning key 3 (0: the dispatch's own choice, QT = 2 at every shape here)
    ldvt: int = 0
    ldo_pad: int = 8                # ldo = H * d + ldo_pad
    div: int = 1                    # kv_batch_div
    mod: int = 0                    # q_batch_mod
    accumulate: bool = False
    o_scale: float = 1.0
    recipe: str = "random"          # "random", "tails", "offset", "spikes", "select"
    param: float = 0.0              # the offset / the spike height, log2 units
    defects: Tuple[str, ...] = ()
    unchanged: Tuple[Tuple[str, str], ...] = ()
    kind = "flash"

    @property
    def ldo(self):
        return self.H * self.d + self.ldo_pad

    @property
    def kvB(self):
        return (self.B + self.div - 1) // self.div

    @property
    def rows(self):
        return self.B * self.n_q

    @property
    def cols(self):
        return self.H * self.d

    @property
    def scale(self):
        return self.d ** -0.5

    @property
    def problem(self):
        """what operands and reference depend on: the cases of one problem share them"""
        return replace(self, name="", qt=0, defects=(), unchanged=())


@dataclass(frozen=True)
class Temporal:
    name: str
    group: str                      # "F" families, "E" selection
    dt: str
    clips: int
    F: int
    P: int
    H: int
    d: int
    rope: bool
    rtol: float
    recipe: str = "random"          # "random", "select"
    defects: Tuple[str, ...] = ()
    unchanged: Tuple[Tuple[str, str], ...] = ()
    kind = "temporal"

    @property
    def rows(self):
        return self.clips * self.F * self.P

    @property
    def cols(self):
        return self.H * self.d

    @property
    def scale(self):
        return self.d ** -0.5 * (math.log(16) / math.log(self.F) if self.F > 16 else 1.0)      # the reference's query factor beyond the training length

    @property
    def problem(self):
        return replace(self, name="", defects=(), unchanged=())


# ---- what a case executes ---------------------------------------------------------------------------------------------------------
def effective_qt(c):
    """attention.hip: `int qt = (a->n_q >= 1024 && wg3 >= 512 && a->d <= 48) ? 3 : 2;` then tuning key 3 if 2..4 and (d <= 80 or it is 2)"""
    wg3 = c.B * c.H * ((c.n_q + 191) // 192)
    qt = 3 if (c.n_q >= 1024 and wg3 >= 512 and c.d <= 48) else 2
    if 2 <= c.qt <= 4 and (c.d <= 80 or c.qt == 2):
        qt = c.qt
    return qt


def traits(c):
    d, qt = c.d, effective_qt(c)
    dp16, dvt = (d + 15) // 16, d // 16 + 1             # FYC_ATTN_CASE: launch_attn<T, (D + 15) / 16, D / 16 + 1, QT>
    dc = dp16 * 2                                       # constexpr int DC = DP16 * 2;
    kxor = dc == 8                                      # constexpr bool KXOR = (DC == 8);
    pc = 8 if kxor else dc + 1                          # constexpr int PC = KXOR ? 8 : DC + 1;
    k_it, v_it = (64 * pc + 255) // 256, (dvt * 16 * 8 + 255) // 256      # K_IT = (KB * PC + 255) / 256, V_IT = (V_ROWS * 8 + 255) / 256
    nfull, ntiles = c.n_k // 64, (c.n_k + 63) // 64     # const int nfull = p.n_k / KB;  const int ntiles = (p.n_k + KB - 1) / KB;
    return dict(
        group="small" if d <= 48 else "medium" if d <= 96 else "large",      # attention.hip: if (a->d <= 48) run_small ... if (a->d <= 96) run_medium
        qt=qt,
        ks=dp16 // 2,                                   # constexpr int KS = DP16 / 2;
        tail=bool(dp16 & 1),                            # constexpr bool TAIL = (DP16 & 1) != 0;
        msub=dvt == dp16,                               # constexpr bool MSUB = (DVT == DP16);
        pipe=dp16 <= 3,                                 # constexpr bool PIPE = DP16 <= 3;
        kxor=kxor,
        offs_in_lds=k_it + v_it <= 4,                   # constexpr bool OFFS_IN_LDS = (K_IT + V_IT) <= 4;
        full_tiles=nfull,
        steady_tiles=max(nfull - 2, 0),                 # const int n_steady = nfull > 2 ? nfull - 2 : 0;
        ragged_tile=ntiles > nfull,                     # issue(): tile < nfull ? issue_full : issue_general
        last_tile_blocks=2 if (ntiles - 1) * 64 + 32 < c.n_k else 1,      # const int nb = ... (tile * KB + 32 < p.n_k) ? 2 : 1
        query_blocks=(c.n_q + 64 * qt - 1) // (64 * qt),                  # p.nqb = (p.n_q + 64 * QT - 1) / (64 * QT);
        xcd=(c.B * c.H) % 8 == 0,                       # if ((BH & 7) == 0) { const int xcd = blockIdx.x & 7 ...
    )


FAMILIES = [(32, 32, 2), (48, 64, 3), (64, 64, 4), (80, 96, 5), (96, 96, 6), (128, 128, 8), (160, 160, 10)]      # launch_d: if (p.d <= X) launch_t<T, DP, DVT, ROPE>


def ttraits(c):
    family = next((dp, dvt) for lim, dp, dvt in FAMILIES if c.d <= lim)
    nft = 1 if c.F <= 16 else 2 if c.F <= 32 else 3 if c.F <= 48 else 4      # launch_t: if (p.frames <= 16) ... <= 32 ... <= 48 ... else 4
    tasks = c.clips * c.P * c.H
    return dict(family=None if c.dt == "f32" else family,                    # the f32 kernel is one scalar kernel, instantiated on ROPE only
                nft=None if c.dt == "f32" else nft,
                lazy=None if c.dt == "f32" else (nft > 2 or (c.rope and nft > 1)),      # constexpr bool LAZY = NFT > 2 || (ROPE && NFT > 1);
                rope=c.rope, padded=c.d != family[0], ragged_grid=tasks % 4 != 0)      # const long long task = blockIdx.x * 4 + (threadIdx.x >> 6);


def built_flash():
    """every (type, d, QT) of csrc/attention_groups.h"""
    out = set()
    for dt in ("bf16", "f16"):
        for d in range(8, 161, 8):
            for qt in ((2, 3, 4) if d <= 80 else (2,)):
                out.add((dt, d, qt))
    return out


def built_temporal():
    """every (type, family, NFT, RoPE) of csrc/temporal_attn.hip, and the two f32 kernels"""
    out = {(dt, (dp, dvt), nft, rope) for dt in ("bf16", "f16") for _, dp, dvt in FAMILIES for nft in (1, 2, 3, 4) for rope in (False, True)}
    return out | {("f32", None, None, False), ("f32", None, None, True)}


# ---- the case list ------------------------------------------------------------------------------------------------------------------
TAIL_NK = [1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 191, 192, 193, 257]
SPIKE_KEYS = [163, 172, 180, 189, 35, 44, 52, 61]       # late (third tile) and early (second block of the first tile), one per lane quad (key % 32 // 8) each
SPIKE_QUERIES = [2, 9, 17, 21, 26, 33, 40, 47]
SPIKE_HEIGHTS = {"f16": (18.0, 40.0), "bf16": (40.0, 150.0)}
NOT_OVER = "2^height is a finite bf16 number: probabilities against the first block's maximum do not overflow, and the normalised result is the same"


def _pad8(n):
    return (n + 7) // 8 * 8


def _flash_cases():
    out = []
    for dt in ("bf16", "f16"):
        # A: head dims
        for d in range(8, 161, 8):
            for qt in ((2, 3, 4) if d <= 80 else (2,)):
                out.append(Flash(f"A-{dt}-d{d}-qt{qt}", "A", dt, 2, 3, 150, 97, d, RTOL_FLASH[dt], qt=qt, ldvt=104,
                                 defects=("drop_heaviest", "pad_key", "swap_rows", "shift_head")))
                if qt > 2:      # 150 queries are one block of 64 QT queries from QT = 3 on: 270 are two, the second ragged
                    out.append(Flash(f"A-{dt}-d{d}-qt{qt}-nq270", "A", dt, 2, 3, 270, 97, d, RTOL_FLASH[dt], qt=qt, ldvt=104,
                                     defects=("drop_heaviest", "swap_rows")))
        # B: key tails
        for d in (40, 64, 160):
            for nk in TAIL_NK:
                out.append(Flash(f"B-{dt}-d{d}-nk{nk}", "B", dt, 1, 8, 40, nk, d, RTOL_FLASH[dt], ldvt=_pad8(nk) + 8, recipe="tails",
                                 defects=("drop_last_key", "pad_key", "drop_heaviest")))
        # C: batch indexing
        for d in (40, 80, 160):
            for div in (1, 2, 3):
                out.append(Flash(f"C-{dt}-d{d}-B5-div{div}", "C", dt, 5, 3, 70, 77, d, RTOL_FLASH[dt], ldvt=80, div=div,
                                 defects=("swap_rows",) + (("ignore_div",) if div > 1 else ()),
                                 unchanged=(("ignore_div", "kv_batch_div = 1: b / 1 = b"),) if div == 1 else ()))
            for mod in (0, 2):
                out.append(Flash(f"C-{dt}-d{d}-B4-mod{mod}-div2", "C", dt, 4, 8, 150, 77, d, RTOL_FLASH[dt], ldvt=80, div=2, mod=mod,
                                 defects=("ignore_div", "shift_head") + (("ignore_mod",) if mod else ()),
                                 unchanged=(("ignore_mod", "q_batch_mod = 0: every batch element has its own q"),) if not mod else ()))
            for o_scale in (0.7, -1.5):
                out.append(Flash(f"C-{dt}-d{d}-acc{o_scale:+g}", "C", dt, 2, 3, 70, 77, d, RTOL_FLASH_ACC[dt], ldvt=80, accumulate=True, o_scale=o_scale,
                                 defects=("scale_prev", "drop_heaviest")))
        # D: scores
        for d in (40, 64):
            for off in (-120.0, -90.0, 90.0, 120.0):
                over = dt == "f16"      # the late spike of this recipe is about 2^45 above the first block
                out.append(Flash(f"D-{dt}-d{d}-offset{off:+g}", "D", dt, 1, 4, 48, 200, d, RTOL_FLASH_ACC[dt], ldvt=208, recipe="offset", param=off,
                                 defects=("drop_heaviest",) + (("freeze_max",) if over else ()), unchanged=() if over else (("freeze_max", NOT_OVER),)))
            for h in SPIKE_HEIGHTS[dt]:
                over = not (dt == "bf16" and h < 128)
                out.append(Flash(f"D-{dt}-d{d}-spikes{h:g}", "D", dt, 1, 4, 48, 200, d, RTOL_FLASH_ACC[dt], ldvt=208, recipe="spikes", param=h,
                                 defects=("drop_heaviest",) + (("freeze_max",) if over else ()), unchanged=() if over else (("freeze_max", NOT_OVER),)))
        # E: selection
        for d in (16, 40, 64, 160):
            out.append(Flash(f"E-{dt}-d{d}-97", "E", dt, 2, 3, 97, 97, d, RTOL_FLASH[dt], ldvt=104, recipe="select"))
            out.append(Flash(f"E-{dt}-d{d}-97-div2-mod2", "E", dt, 4, 2, 97, 97, d, RTOL_FLASH[dt], ldvt=104, div=2, mod=2, recipe="select"))
    return out


TEMPORAL_D = [8, 24, 40, 48, 56, 64, 72, 88, 96, 104, 128, 136, 160]
TEMPORAL_F = {1: [1, 2, 15, 16], 2: [17, 32], 3: [33, 48], 4: [49, 64]}      # by NFT
ONE_FRAME = "one frame: the only table row is cos = 1, sin = 0, and a single key has weight 1 whatever its score"


def _temporal_cases():
    out = []
    n = 0
    for i, d in enumerate(TEMPORAL_D):
        for nft, fl in TEMPORAL_F.items():
            F = fl[(i + nft) % len(fl)]
            for rope in (False, True):
                P, H, clips = (1, 5)[n % 2], (1, 3, 8)[n % 3], (1, 2)[(n // 2) % 2]
                n += 1
                for dt in ("bf16", "f16") + (("f32",) if nft == (i % 4) + 1 else ()):
                    rt = (RTOL_TEMPORAL_ROPE if rope else RTOL_TEMPORAL)[dt]
                    defects, unchanged = ("mask_last",), ()
                    if rope and F > 1:
                        defects += ("rope_sign", "rope_next_q")
                    elif rope:
                        unchanged = (("rope_sign", ONE_FRAME), ("rope_next_q", ONE_FRAME))
                    out.append(Temporal(f"F-{dt}-d{d}-F{F}-P{P}-H{H}-c{clips}{'-rope' if rope else ''}", "F", dt, clips, F, P, H, d, rope, rt,
                                        defects=defects, unchanged=unchanged))
    # E: selection
    for dt in ("bf16", "f16"):
        for F in (16, 17, 33, 64):
            for d in (16, 64, 104, 160):
                out.append(Temporal(f"E-{dt}-d{d}-F{F}", "E", dt, 2, F, 3, 3, d, False, RTOL_TEMPORAL[dt], recipe="select"))
    out.append(Temporal("E-f32-d64-F33", "E", "f32", 2, 33, 3, 3, 64, False, RTOL_TEMPORAL["f32"], recipe="select"))
    return out


FLASH_CASES = _flash_cases()
TEMPORAL_CASES = _temporal_cases()
CASES = FLASH_CASES + TEMPORAL_CASES
assert len({c.name for c in CASES}) == len(CASES)


def by_group(kind, *groups):
    return [c for c in CASES if c.kind == kind and c.group in groups]


def case_ids(cases):
    return [c.name for c in cases]


# ---- operands -----------------------------------------------------------------------------------------------------------------------
def _seed(c):
    return int.from_bytes(repr(c.problem).encode(), "little") % (2 ** 31 - 1)


def _filled(n, T):
    es = torch.empty(0, dtype=T).element_size()
    return torch.full((n,), FILL[es], dtype={2: torch.int16, 4: torch.int32}[es]).view(T)


def _codes(n, d):
    """n distinct +-1 rows of length d: the bits of the index and their complements (two rows differ in at least two places: dot products differ by
    at least 4), the remaining places +1"""
    bits = max(1, (n - 1).bit_length())
    assert 2 * bits <= d
    b = ((torch.arange(n)[:, None] >> torch.arange(bits)[None, :]) & 1).double() * 2 - 1
    return torch.cat([b, -b, torch.ones(n, d - 2 * bits, dtype=torch.float64)], dim=1)


def select_gain(scale):
    """the power of two c with c * 4 * scale * log2e >= 80: the selected key's score leads every other by at least 80 log2 units"""
    return 2.0 ** math.ceil(math.log2(80.0 / (4 * scale * KC.LOG2E)))


def kv_of(c, b):
    return b // c.div


def q_of(c, b):
    return b % c.mod if c.mod else b


def operands(c):
    if c.kind == "temporal":
        return _temporal_operands(c)
    T, g = DT[c.dt], torch.Generator().manual_seed(_seed(c))
    B, H, nq, nk, d = c.B, c.H, c.n_q, c.n_k, c.d
    ops = SimpleNamespace(designated=[], spikes=[], pi=None)
    q = torch.randn(B, H, nq, d, generator=g)            # for every batch element; the kernel is given the first q_batch_mod of them
    k = torch.randn(c.kvB, H, nk, d, generator=g)
    v = torch.randn(c.kvB, H, nk, d, generator=g)
    if c.recipe == "offset":      # test_attention_score_offsets_and_late_spikes at n_q = 48, n_k = 200
        q[..., 0], q[..., 1] = 1.0, 2.0
        k[..., 0] = c.param * math.sqrt(d) / KC.LOG2E                        # every score moves by `param` log2 units
        k[..., 1] = torch.arange(nk).float() * 0.004                         # and creeps up a little with every key
        k[:, :, 190] += q[:, :, 17] * 5                                      # late spike for query 17
        k[:, :, 2] += q[:, :, 40] * 7                                        # early spike for query 40
    elif c.recipe == "spikes":    # test_attention_late_spike_in_every_lane_quad, one query per key
        for qs, key in zip(SPIKE_QUERIES, SPIKE_KEYS):
            unit = (q[:, :, qs] * q[:, :, qs]).sum(-1, keepdim=True) * c.scale * KC.LOG2E
            k[:, :, key] += q[:, :, qs] * (c.param / unit)
            ops.spikes.append((qs, key))
    elif c.recipe == "select":
        assert nq == nk and not c.accumulate
        code, gain = _codes(nk, d), select_gain(c.scale)
        sigma = torch.stack([torch.stack([torch.randperm(nk, generator=g) for _ in range(H)]) for _ in range(c.kvB)])      # k[kvb, h][j] = code[sigma[j]]
        tau = torch.stack([torch.stack([torch.randperm(nk, generator=g) for _ in range(H)]) for _ in range(B)])            # q[b, h][i] = gain * code[tau[i]]
        if c.mod:
            tau = tau[torch.arange(B) % c.mod]
        k, q = code[sigma].float(), gain * code[tau].float()
        inv = torch.argsort(sigma, dim=-1)
        ops.pi = torch.stack([torch.gather(inv[kv_of(c, b)], -1, tau[b]) for b in range(B)])                               # [B][H][n_q]: the key each query selects
        v = (0.5 + 1.49 * torch.rand(c.kvB, H, nk, d, generator=g)) * (torch.randint(0, 2, (c.kvB, H, nk, d), generator=g) * 2 - 1)
    q, k, v = q.to(T), k.to(T), v.to(T)
    if c.recipe == "tails" and nk >= 3:
        # designated queries with a moderate weight on the keys a tail mask can lose: the last, the one before, the first of the last 32-key block,
        # the first of the last tile.  k_j = alpha q_r with alpha solved for a weight of 0.35 in f64, two sweeps (the keys see each other)
        keys = []
        for j in (nk - 1, nk - 2, (nk - 1) // 32 * 32, (nk - 1) // 64 * 64):
            if j not in keys:
                keys.append(j)
        ops.designated = list(zip((3, 12, 21, 30), keys))
        for _ in range(3):
            for r, j in ops.designated:
                qr = q[0, :, r].double()                                                        # [H][d]
                s = torch.einsum("hd,hjd->hj", qr, k[0].double()) * c.scale
                s[:, j] = -math.inf
                target = torch.log(0.35 / 0.65 * torch.exp(s).sum(-1))                          # [H]
                k[0, :, j] = (qr * (target / (c.scale * (qr * qr).sum(-1)))[:, None]).to(T)
    vt = torch.empty(c.kvB, H, d, c.ldvt, dtype=T)
    vt[..., :nk] = v.transpose(-1, -2)
    big = torch.finfo(T).max
    vt[..., nk:] = torch.tensor([big, -big] * c.ldvt, dtype=T)[: c.ldvt - nk]      # pad keys: finite, as far from zero as the type goes, alternating sign
    ops.q_full, ops.q, ops.k, ops.vt = q, q[: c.mod] if c.mod else q, k, vt
    ops.pad_value = vt[..., nk] if c.ldvt > nk else None                            # [kvB][H][d]
    # the guarded output buffer
    buf = _filled(FRONT + (c.rows + BACK_ROWS) * c.ldo, T)
    mask = torch.zeros(buf.numel(), dtype=torch.bool)
    win = mask[FRONT:].view(c.rows + BACK_ROWS, c.ldo)
    win[: c.rows, : c.cols] = True
    if c.accumulate:
        window(c, buf).copy_(torch.randn(c.rows, c.cols, generator=g).to(T))
    ops.buf, ops.mask = buf, mask
    return ops


def _temporal_operands(c):
    T, g = DT[c.dt], torch.Generator().manual_seed(_seed(c))
    C = c.cols
    ops = SimpleNamespace(pi=None)
    x = torch.randn(c.clips, c.F, c.P, 3, c.H, c.d, generator=g)
    if c.recipe == "select":
        code, gain = _codes(c.F, c.d), select_gain(c.scale)
        shape = (c.clips, c.P, c.H)
        sigma = torch.stack([torch.randperm(c.F, generator=g) for _ in range(c.clips * c.P * c.H)]).view(*shape, c.F)
        tau = torch.stack([torch.randperm(c.F, generator=g) for _ in range(c.clips * c.P * c.H)]).view(*shape, c.F)
        x[:, :, :, 0] = (gain * code[tau]).float().permute(0, 3, 1, 2, 4)            # [clips][P][H][F][d] -> [clips][F][P][H][d]
        x[:, :, :, 1] = code[sigma].float().permute(0, 3, 1, 2, 4)
        x[:, :, :, 2] = (0.5 + 1.49 * torch.rand(c.clips, c.F, c.P, c.H, c.d, generator=g)) * (torch.randint(0, 2, (c.clips, c.F, c.P, c.H, c.d), generator=g) * 2 - 1)
        ops.pi = torch.gather(torch.argsort(sigma, dim=-1), -1, tau)                 # [clips][P][H][F]: the frame each query frame selects
    ops.qkv = x.to(T).reshape(c.rows, 3 * C)
    ops.tables = rope_spec.rope_tables(c.d, c.F) if c.rope else None
    ops.tables_next = tuple(t[1:].contiguous() for t in rope_spec.rope_tables(c.d, c.F + 1)) if c.rope else None
    buf = _filled(FRONT + (c.rows + c.P) * C, T)
    mask = torch.zeros(buf.numel(), dtype=torch.bool)
    mask[FRONT: FRONT + c.rows * C] = True
    ops.buf, ops.mask = buf, mask
    return ops


def window(c, buf):
    """the [rows][cols] output inside a guarded buffer (a view)"""
    ld = c.ldo if c.kind == "flash" else c.cols
    return buf[FRONT:].view(-1, ld)[: c.rows, : c.cols]


def out_view(c, buf):
    """what is passed as `o`: the buffer from its first output element on"""
    return buf[FRONT:]


def labels(c):
    if c.kind == "flash":
        qt = effective_qt(c)
        return KC.Labels(lambda i: f"batch {i // c.n_q}, query {i % c.n_q}: query block {i % c.n_q // (64 * qt)}, wave {i % c.n_q % (64 * qt) // (16 * qt)}, "
                                   f"tile {i % c.n_q % (16 * qt) // 16}, lane column {i % 16}",
                         lambda j: f"head {j // c.d}, channel {j % c.d}: 16-row block {j % c.d // 16}, quad {j % 16 // 4}")
    return KC.Labels(lambda i: f"clip {i // (c.F * c.P)}, frame {i // c.P % c.F}, pixel {i % c.P}", lambda j: f"head {j // c.d}, channel {j % c.d}")


# ---- reference and bound ------------------------------------------------------------------------------------------------------------
def reference(c, ops):
    """-> (ref: the guarded buffer holding the f64 reference rounded to the storage type, bound [rows][cols] f64, w: the reference weights
    [B][H][n_q][n_k] / [clips][P][H][F][F])"""
    if c.kind == "temporal":
        return _temporal_reference(c, ops)
    T = DT[c.dt]
    o = torch.empty(c.B, c.n_q, c.H, c.d, dtype=torch.float64)
    rest = torch.empty_like(o)
    w = torch.empty(c.B, c.H, c.n_q, c.n_k, dtype=torch.float64)
    for b in range(c.B):
        for h in range(c.H):
            kv = kv_of(c, b)
            o[b, :, h], rest[b, :, h], w[b, h] = KC.softmax_bound_terms(ops.q_full[q_of(c, b), h].double(), ops.k[kv, h].double(), ops.vt[kv, h, :, : c.n_k].double().T.contiguous(),
                                                                       scale=c.scale, dtype=c.dt, kind="flash")
    o, rest = o.reshape(c.rows, c.cols), rest.reshape(c.rows, c.cols)
    ref = ops.buf.clone()
    if c.accumulate:
        prev = window(c, ops.buf).double()
        acc = prev + c.o_scale * o
        window(c, ref).copy_(acc.to(T))
        bound = KC.ulp(window(c, ref).double(), c.dt) + abs(c.o_scale) * rest + 2 * 2.0 ** -24 * (prev.abs() + abs(c.o_scale) * o.abs())
    else:
        window(c, ref).copy_(o.to(T))
        bound = KC.ulp(window(c, ref).double(), c.dt) + rest
    return ref, bound, w


def _rotate(x, cos, sin, flip_upper=False):
    """x [..][F][d] f32, tables [F][d/2]: x cos + rotate_half(x) sin in f32 as include/fyc.h specifies; -> (rotated, |x cos| + |x' sin|)"""
    cs, sn = torch.cat((cos, cos), -1), torch.cat((sin, sin), -1)
    if flip_upper:
        sn = torch.cat((sin, -sin), -1)
    return x * cs + rope_spec.rotate_half(x) * sn, (x * cs).abs() + (rope_spec.rotate_half(x) * sn).abs()


def _split(c, ops):
    x = ops.qkv.reshape(c.clips, c.F, c.P, 3, c.H, c.d)
    return tuple(x[:, :, :, i].permute(0, 2, 3, 1, 4) for i in range(3))        # [clips][P][H][F][d]


def _temporal_reference(c, ops):
    T = DT[c.dt]
    q, k, v = _split(c, ops)
    dq = dk = None
    if c.rope:
        (q, mq), (k, mk) = (_rotate(t.float(), *ops.tables) for t in (q, k))
        if c.dt != "f32":
            q, k = q.to(T), k.to(T)
            dq, dk = KC.ulp(q.double(), c.dt), KC.ulp(k.double(), c.dt)
        else:
            dq, dk = 3 * KC.U["f32"] * mq.double(), 3 * KC.U["f32"] * mk.double()
    o = torch.empty(c.clips, c.P, c.H, c.F, c.d, dtype=torch.float64)
    rest = torch.empty_like(o)
    w = torch.empty(c.clips, c.P, c.H, c.F, c.F, dtype=torch.float64)
    for b in range(c.clips):
        for p in range(c.P):
            kw = dict(dq=dq[b, p], dk=dk[b, p]) if dq is not None else {}
            o[b, p], rest[b, p], w[b, p] = KC.softmax_bound_terms(q[b, p].double(), k[b, p].double(), v[b, p].double(), scale=c.scale, dtype=c.dt, kind="temporal", **kw)
    o, rest = (t.permute(0, 3, 1, 2, 4).reshape(c.rows, c.cols) for t in (o, rest))
    ref = ops.buf.clone()
    window(c, ref).copy_(o.to(T))
    return ref, KC.ulp(window(c, ref).double(), c.dt) + rest, w


# ---- models of the kernels' rounding points -----------------------------------------------------------------------------------------
def flash_model(c, ops, placement=0.0, defect=None):
    """The flash kernel's roundings in torch (kernel_compare's docstring, points 1 - 6), for a running max that sits `placement` log2 units below the
    row's true maximum (0 .. RESCALE_THR = 6: where it ends up depends on the order of the keys) -> the window [rows][cols] in the storage type"""
    T, t = DT[c.dt], traits(c)
    sl2e = float(np.float32(c.scale) * np.float32(1.44269504088896340736))
    out = torch.empty(c.B, c.n_q, c.H, c.d, dtype=torch.float32)
    for b in range(c.B):
        kv = kv_of(c, b) if not (defect == "ignore_div" and b == 1) else b
        qb = q_of(c, b) if defect != "ignore_mod" else b
        q1 = (ops.q_full[qb].float() * sl2e).to(T).float()                          # 1
        k, v = ops.k[kv].float(), ops.vt[kv, :, :, : c.n_k].float().transpose(-1, -2)
        s = q1 @ k.transpose(-1, -2)                                                # 2  [H][n_q][n_k]
        if defect == "pad_key":
            s = torch.cat((s, torch.zeros(c.H, c.n_q, 1)), -1)
            v = torch.cat((v, ops.pad_value[kv].float()[:, None, :]), 1)
        if defect == "drop_last_key":
            s[..., c.n_k - 1] = -math.inf
        if defect == "drop_heaviest":
            dq = defect_query(c)
            s[c.H - 1, dq, s[c.H - 1, dq, : c.n_k].argmax()] = -math.inf
        m = (s[..., :32].max(-1, keepdim=True).values if defect == "freeze_max" else s.max(-1, keepdim=True).values - placement)
        if t["msub"]:
            m = m.to(T).float()                                                     # const float m_new = mv ? round_through<T>(m_run + mx) : m_run
        p = torch.exp2(s - m).to(T).float()                                         # 3, 4
        out[b] = ((p @ v) * (1.0 / p.sum(-1, keepdim=True))).transpose(0, 1)        # 5, 6
    out = out.reshape(c.rows, c.cols)
    if c.accumulate:
        prev = window(c, ops.buf).float()
        out = c.o_scale * prev + out if defect == "scale_prev" else prev + c.o_scale * out
    out = out.to(T)
    if defect == "swap_rows":
        r = c.rows - c.n_q + DEFECT_QUERY          # in the last batch element
        out[[r, r + 1]] = out[[r + 1, r]]
    if defect == "shift_head":
        out = out.clone()
        src = out.view(c.rows, c.H, c.d)
        out.view(c.rows, c.H, c.d)[:, c.H - 2] = src[:, c.H - 1].clone()
    return out


DEFECT_QUERY = 21


def defect_query(c):
    """whose heaviest key drop_heaviest drops: in group D a query with a spike (the common score offset makes the bound of an ordinary row wide:
    the kernel's Q' rounding acts on 120 log2 units there, and that it moves all keys alike is not known to a per-key bound)"""
    return 17 if c.group == "D" else DEFECT_QUERY


def temporal_model(c, ops, defect=None):
    T = DT[c.dt]
    q, k, v = (t.float() for t in _split(c, ops))
    if c.rope:
        tq = ops.tables_next if defect == "rope_next_q" else ops.tables
        q, k = _rotate(q, *tq, flip_upper=defect == "rope_sign")[0], _rotate(k, *ops.tables, flip_upper=defect == "rope_sign")[0]
        if c.dt != "f32":
            q, k = q.to(T).float(), k.to(T).float()
    s = q @ k.transpose(-1, -2)
    if defect == "mask_last":
        s[..., c.F - 1] = -math.inf
    if c.dt != "f32":
        sl2e = float(np.float32(c.scale) * np.float32(1.44269504088896340736))
        p = torch.exp2((s - s.max(-1, keepdim=True).values) * sl2e)
        p = (p * (1.0 / p.sum(-1, keepdim=True))).to(T).float()
    else:
        s = s * c.scale
        p = torch.exp(s - s.max(-1, keepdim=True).values)
        p = p * (1.0 / p.sum(-1, keepdim=True))
    return (p @ v).permute(0, 3, 1, 2, 4).reshape(c.rows, c.cols).to(T)


def model(c, ops, placement=0.0, defect=None):
    return flash_model(c, ops, placement, defect) if c.kind == "flash" else temporal_model(c, ops, defect)


def selected(c, ops):
    """selection cases: the output that must come out bit for bit, v[pi(query)]"""
    if c.kind == "flash":
        out = torch.empty(c.B, c.n_q, c.H, c.d, dtype=DT[c.dt])
        for b in range(c.B):
            for h in range(c.H):
                out[b, :, h] = ops.vt[kv_of(c, b), h, :, : c.n_k].T[ops.pi[b, h]]
        return out.reshape(c.rows, c.cols)
    v = _split(c, ops)[2]                                                       # [clips][P][H][F][d]
    return torch.gather(v, 3, ops.pi[..., None].expand(-1, -1, -1, -1, c.d)).permute(0, 3, 1, 2, 4).reshape(c.rows, c.cols)
