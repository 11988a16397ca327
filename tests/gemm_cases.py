"""The fyc_gemm cases of tests/test_gemm_epilogues_gpu.py as data, with what each of them is MEANT to execute.  A helper, not a test module;
no GPU is touched here.

Three users share the list, so that the GPU tests cannot drift away from the kernels they name:
  * tests/test_gemm_cases.py (CPU) writes the cases in the line format of tests/gemm_plan_harness.hip's second mode and compares the
    recorded launch - executed tile config, ring depth, wide, split or not - with the declared intent;
  * tests/test_kernel_compare.py (CPU) runs every case on the emulator in f32 and in f64 accumulation;
  * tests/test_gemm_epilogues_gpu.py launches them.

The intent is written down from the rules of csrc/gemm_plan.h as a reader understands them, not computed by a copy of the planner:
  * 16-bit, every pitch a multiple of 8 elements, 16-byte aligned operands: the wide (16-byte, LDS-staged) epilogue, on the tile that was asked
    for; tile 0 is the automatic choice, which is 128x64 (config 2) at every N used here (N = 328, 320 with M < 4096, 40);
  * ring depths other than 2 exist for (1, 3) and, in PLAIN mode, (2, 3) and (2, 4);
  * the 64-byte K-tile configs 8 / 10 cannot stage several row-bias groups per row tile: with rows_per_batch = 96 their 128-byte twins 6 / 1 run.
    The cases keep those combinations (the replacement is a decision worth pinning) and each convolution geometry also runs 8 and 10 WITHOUT a
    row bias, so that 8 and 10 are executed wide in every mode;
  * f32, an output that is not 16-byte aligned or an odd pitch: the narrow per-lane epilogue, which only exists for configs 1 and 2.
"""
import math
from dataclasses import dataclass, field, replace
from typing import Optional, Tuple

import torch

from test_kernels_gpu import CONV_TILES, F16_TILES, PLAIN_TILES

PLAIN, CONV, UP2, T3 = 0, 1, 2, 3
DT = {"bf16": torch.bfloat16, "f32": torch.float32, "f16": torch.float16}
DT_CODE = {"f32": 0, "bf16": 1, "f16": 2}                 # fyc_dtype
TUNE_TILE, TUNE_RING, TUNE_SPLITK_MIN_KT = 1, 2, 10       # fyc_set_tuning keys
FRONT = 64                                                # guard elements in front of `out` (a multiple of 8: the alignment of `out` is out_off's)
BACK_ROWS = 2                                             # guard rows behind it
EXTRA_PLAIN_RINGS = [(2, 3), (2, 4)]                      # the deeper rings of the 128x64 linears, next to PLAIN_TILES
AUTO_TILE = 2                                             # what tile 0 resolves to at the shapes of this file (see the head)


@dataclass(frozen=True)
class Case:
    name: str
    group: str                       # "plain", "narrow", "conv", "pixel", "alias", "stripes", "splitk"
    dt: str
    mode: int
    M: int
    N: int
    K: int
    lda: int
    ldw: int
    ldo: int
    ldr: int = 0
    ldrb: int = 0
    rpb: int = 1
    bias: bool = True
    rowbias: bool = False
    rb_off: int = 0                  # floats between the start of the row-bias table and the pointer passed
    residual: int = 0                # 0 none, 1 a buffer of its own, 2 the output itself (in-place add)
    out_off: int = 0                 # elements added to the (16-byte aligned) output pointer
    tile: int = 0
    ring: int = 0
    tuning: Tuple[Tuple[int, int], ...] = ()      # further fyc_set_tuning keys
    batch: int = 1
    stride_a: int = 0
    stride_w: int = 0
    stride_o: int = 0
    out_scale: float = 1.0
    conv: Optional[Tuple[Tuple[str, int], ...]] = None      # the items of ops.gemm's `conv` dict
    identity_w: bool = False
    chan: bool = False
    cs_rows: int = 0
    # ---- what the case is meant to execute ----
    want_cfg: int = 0                # tile config after the narrow-epilogue rewrite
    want_ring: int = 2               # -1: the f32 entries take none
    want_wide: int = 0
    want_split: bool = False

    @property
    def conv_dict(self):
        return dict(self.conv) if self.conv is not None else None

    @property
    def cols(self):
        """columns of the output buffer the launch writes: the batch elements of the stripes case lie side by side"""
        return self.N * self.batch

    @property
    def all_tuning(self):
        return ((TUNE_TILE, self.tile), (TUNE_RING, self.ring)) + tuple(self.tuning)


def _intent(dt, tile, ring, mode, *, staged_rb, narrow=False):
    if dt == "f32":
        return dict(want_cfg=2, want_ring=-1, want_wide=0)
    if narrow:
        return dict(want_cfg=2, want_ring=2, want_wide=0)
    cfg = tile if tile else AUTO_TILE
    if staged_rb and cfg in (8, 10):
        cfg = 6 if cfg == 8 else 1
    deep = (cfg, ring) == (1, 3) or (mode == PLAIN and (cfg, ring) in EXTRA_PLAIN_RINGS)
    return dict(want_cfg=cfg, want_ring=ring if deep else 2, want_wide=1)


def _dt_tiles(tiles16, f16_tiles):
    return [("bf16", t) for t in tiles16] + [("f16", t) for t in f16_tiles] + [("f32", (0, 0))]


RB_LAYOUTS = {"norb": dict(rowbias=False), "rb96": dict(rowbias=True, rpb=96, ldrb=332, rb_off=8), "rb256": dict(rowbias=True, rpb=256, ldrb=332, rb_off=8)}


def _plain_cases():
    out = []
    base = dict(mode=PLAIN, M=300, N=328, K=136, lda=144, ldw=152, ldo=336, ldr=344, residual=1, out_scale=0.75)
    for dt, (tile, ring) in _dt_tiles(PLAIN_TILES + EXTRA_PLAIN_RINGS, F16_TILES + [(8, 2), (10, 2)]):
        for rb, rbkw in RB_LAYOUTS.items():
            out.append(Case(name=f"plain-{dt}-t{tile}r{ring}-{rb}", group="plain", dt=dt, tile=tile, ring=ring, **base, **rbkw,
                            **_intent(dt, tile, ring, PLAIN, staged_rb=rb == "rb96")))
    # 4.2: the same problem where nothing allows a 16-byte access
    for dt in ("bf16", "f16"):
        for tile in (0, 5):
            kw = dict(base, ldo=329)
            out.append(Case(name=f"narrow-{dt}-t{tile}", group="narrow", dt=dt, tile=tile, ring=0, out_off=1, rowbias=True, rpb=96, ldrb=331, rb_off=8, **kw,
                            **_intent(dt, tile, 0, PLAIN, staged_rb=True, narrow=True)))
    return out


# (name, mode, stride, pad, Hin, Win): 8 x 12 outputs each
CONV_GEOMS = [("s1p1", CONV, 1, 1, 8, 12), ("s2p1", CONV, 2, 1, 16, 24), ("s2p0", CONV, 2, 0, 16, 24), ("s1p0", CONV, 1, 0, 9, 13),
              ("up2x", UP2, 1, 1, 4, 6), ("up5x7", UP2, 1, 1, 5, 7)]


def _conv_cases():
    out = []
    frames, Ho, Wo, Cout = 3, 8, 12, 328
    for gname, mode, stride, pad, Hin, Win in CONV_GEOMS:
        conv = (("Hout", Ho), ("Wout", Wo), ("Hin", Hin), ("Win", Win), ("stride", stride), ("pad", pad))
        for Cin in (64, 128):
            base = dict(group="conv", mode=mode, M=frames * Ho * Wo, N=Cout, K=9 * Cin, lda=Cin, ldw=9 * Cin + 8, ldo=336, ldr=344, residual=1,
                        conv=conv + (("Cin", Cin),))
            for dt, (tile, ring) in _dt_tiles(CONV_TILES, F16_TILES):
                out.append(Case(name=f"conv-{gname}-c{Cin}-{dt}-t{tile}r{ring}", dt=dt, tile=tile, ring=ring, rowbias=True, rpb=96, ldrb=332, rb_off=8, **base,
                                **_intent(dt, tile, ring, mode, staged_rb=True)))
            if Cin == 64:      # 8 / 10 themselves: without row-bias groups to stage (see the head)
                for tile in (8, 10):
                    out.append(Case(name=f"conv-{gname}-c{Cin}-bf16-t{tile}r2-norb", dt="bf16", tile=tile, ring=2, **base, **_intent("bf16", tile, 2, mode, staged_rb=False)))
    # one pixel per frame: every tap but the centre is padding
    conv = (("Hout", 1), ("Wout", 1), ("Hin", 1), ("Win", 1), ("stride", 1), ("pad", 1), ("Cin", 64))
    for dt, (tile, ring) in _dt_tiles(CONV_TILES, F16_TILES):
        out.append(Case(name=f"pixel-{dt}-t{tile}r{ring}", group="pixel", dt=dt, mode=CONV, M=5, N=328, K=576, lda=64, ldw=584, ldo=336, ldr=344, residual=1, conv=conv,
                        tile=tile, ring=ring, **_intent(dt, tile, ring, CONV, staged_rb=False)))
    return out


def _alias_cases():
    """the engine's in-place add y = x I + y: the residual is the output"""
    return [Case(name=f"alias-{dt}-t{tile}", group="alias", dt=dt, mode=PLAIN, M=300, N=320, K=320, lda=320, ldw=320, ldo=328, ldr=328, bias=False, residual=2,
                 identity_w=True, tile=tile, ring=0, **_intent(dt, tile, 0, PLAIN, staged_rb=False))
            for dt in ("bf16", "f16") for tile in (0, 1, 5, 6, 8, 11)]


def _stripe_cases():
    """P V of the materialised attention: head z writes the columns [40 z, 40 z + 40) of every row"""
    return [Case(name=f"stripes-{dt}", group="stripes", dt=dt, mode=PLAIN, M=40, N=40, K=48, lda=48, ldw=56, ldo=160, bias=False, batch=4,
                 stride_a=40 * 48, stride_w=40 * 56, stride_o=40, **_intent(dt, 0, 0, PLAIN, staged_rb=False)) for dt in ("f32", "bf16", "f16")]


def _splitk_cases():
    out = []
    for dt in ("bf16", "f16"):
        for chan in (False, True):
            common = dict(group="splitk", dt=dt, M=288, N=328, ldo=336, ldr=344, residual=1, rowbias=True, rpb=96, ldrb=332, rb_off=8, tuning=((TUNE_SPLITK_MIN_KT, 2),),
                          chan=chan, cs_rows=96 if chan else 0, want_cfg=1, want_ring=2, want_wide=1, want_split=True)
            tag = "-stats" if chan else ""
            out.append(Case(name=f"splitk-plain-{dt}{tag}", mode=PLAIN, K=520, lda=528, ldw=536, **common))
            out.append(Case(name=f"splitk-t3-{dt}{tag}", mode=T3, K=576, lda=192, ldw=584, conv=(("Cin", 192), ("frames", 3), ("rows", 96)), **common))
    return out


CASES = _plain_cases() + _conv_cases() + _alias_cases() + _stripe_cases() + _splitk_cases()
assert len({c.name for c in CASES}) == len(CASES)
BY_NAME = {c.name: c for c in CASES}

# today's tests/test_kernels_gpu.py::test_gemm_plain, as it calls fyc_gemm (rows_per_batch = 50, pitches = widths, tile 5 forced): NOT a GPU case
# of this file, only pinned by tests/test_gemm_cases.py - the 16-bit sweep takes the narrow epilogue on config 1 / 2
OLD_PLAIN_SWEEP = [Case(name=f"old-plain-{dt}-{M}x{N}x{K}", group="old", dt=dt, mode=PLAIN, M=M, N=N, K=K, lda=K, ldw=K, ldo=N, ldr=N, rowbias=True, rpb=50, residual=1,
                        out_scale=0.75, tile=5, ring=2, want_cfg=1 if (N % 128 == 0 or N > 512) else 2, want_ring=2, want_wide=0)
                   for dt in ("bf16",) for M, N, K in [(256, 128, 128), (300, 320, 320), (154, 64, 768), (8, 256, 64), (1000, 960, 40), (513, 4, 576)]]


def by_group(*groups):
    return [c for c in CASES if c.group in groups]


def case_ids(cases):
    return [c.name for c in cases]


# ---- the line format of tests/gemm_plan_harness.hip's second mode ----------------------------------------------------------------------
def harness_line(c):
    es = 4 if c.dt == "f32" else 2
    f = dict(dtype=DT_CODE[c.dt], mode=c.mode, M=c.M, N=c.N, K=c.K, lda=c.lda, ldw=c.ldw, ldo=c.ldo, ldr=c.ldr, ldrb=c.ldrb, rpb=c.rpb, bias=int(c.bias),
             rowbias=int(c.rowbias), residual=c.residual, out_off=(FRONT + c.out_off) * es, rb_off=4 * c.rb_off, batch=c.batch, stride_a=c.stride_a,
             stride_w=c.stride_w, stride_o=c.stride_o, chan=int(c.chan), cs_rows=c.cs_rows)
    if c.conv is not None:
        conv = c.conv_dict
        if c.mode == T3:
            f.update(Cin=conv["Cin"], t3_frames=conv["frames"], t3_rows=conv["rows"])
        else:
            f.update(conv)
    toks = [c.name] + [f"{k}={v}" for k, v in f.items()] + [f"tune={k}:{v}" for k, v in c.all_tuning if v]
    return " ".join(toks)


# ---- operands -------------------------------------------------------------------------------------------------------------------------
def _rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def prefill(n, dtype):
    """a finite, non-zero pattern that every storage type holds exactly and that does not repeat with the period of a row or a tile"""
    i = torch.arange(n, dtype=torch.float64)
    return ((0.5 + (i % 13) / 16) * (1 - 2 * (i % 2))).to(dtype)


@dataclass
class Operands:
    a: torch.Tensor
    w: torch.Tensor
    bias: Optional[torch.Tensor]
    rb_table: Optional[torch.Tensor]      # the whole row-bias table; the op gets rb_table.reshape(-1)[rb_off:]
    residual: Optional[torch.Tensor]      # None for residual == 0 and for the in-place case
    buf: torch.Tensor                     # the output buffer with its guard bands, prefilled (in-place case: holding y)
    mask: torch.Tensor = field(repr=False, default=None)      # bool over buf: what the op may write


def out_offset(c):
    return FRONT + c.out_off


def buf_len(c):
    return out_offset(c) + (c.M + BACK_ROWS) * c.ldo


def logical(c, buf):
    """the [M][columns] window of an output buffer that the launch writes"""
    return torch.as_strided(buf, (c.M, c.cols), (c.ldo, 1), buf.storage_offset() + out_offset(c))


def operands(c):
    """the CPU operands of a case, the same values for every tile of a problem (seeded by the operand, not by the case)"""
    T = DT[c.dt]
    conv = c.conv_dict
    if c.mode == PLAIN:
        a = _rnd((c.batch * c.M, c.lda) if c.batch > 1 else (c.M, c.lda), T, 1)
        assert c.batch == 1 or (c.stride_a == c.M * c.lda and c.stride_w == c.N * c.ldw and c.stride_o == c.N)
    elif c.mode == T3:
        a = _rnd((c.M, conv["Cin"]), T, 1)
    else:
        a = _rnd((c.M // (conv["Hout"] * conv["Wout"]) * conv["Hin"] * conv["Win"], conv["Cin"]), T, 1)
    if c.identity_w:
        w = torch.zeros(c.N, c.ldw, dtype=T)
        w[:, :c.K] = torch.eye(c.N, c.K, dtype=T)
    else:
        w = _rnd((c.batch * c.N, c.ldw), T, 2, 1 / math.sqrt(c.K))
    bias = _rnd((c.N,), torch.float32, 3) if c.bias else None
    rb_table = None
    if c.rowbias:
        groups = (c.M + c.rpb - 1) // c.rpb
        rb_table = _rnd((c.rb_off + groups * (c.ldrb or c.N),), torch.float32, 5)
    residual = _rnd((c.M, c.ldr), T, 4) if c.residual == 1 else None
    buf = prefill(buf_len(c), T)
    mask = torch.zeros(buf_len(c), dtype=torch.bool)
    logical(c, mask).fill_(True)
    if c.residual == 2:
        logical(c, buf).copy_(_rnd((c.M, c.cols), T, 4))
    return Operands(a=a, w=w, bias=bias, rb_table=rb_table, residual=residual, buf=buf, mask=mask)


def gemm_kwargs(c, ops_, out_buf, *, to=lambda t: t, residual_buf=None):
    """(a, w, out) and the keyword arguments of ops.gemm / EmuOps.gemm for a case; `to` moves an operand (e.g. to the GPU), `out_buf` is the
    whole guarded buffer on that side.  residual_buf: run the in-place case out of place, with its y read from this guarded buffer"""
    out = out_buf[out_offset(c):]
    kw = dict(M=c.M, N=c.N, K=c.K, lda=c.lda, ldw=c.ldw, ldo=c.ldo, ldr=c.ldr, ldrb=c.ldrb, rows_per_batch=c.rpb, out_scale=c.out_scale, mode=c.mode)
    if c.bias:
        kw["bias"] = to(ops_.bias)
    if c.rowbias:
        kw["rowbias"] = to(ops_.rb_table)[c.rb_off:]
    if c.residual == 1:
        kw["residual"] = to(ops_.residual)
    elif c.residual == 2:
        kw["residual"] = out if residual_buf is None else residual_buf[out_offset(c):]
    if c.conv is not None:
        kw["conv"] = c.conv_dict
    if c.batch > 1:
        kw.update(batch=c.batch, stride_a=c.stride_a, stride_w=c.stride_w, stride_o=c.stride_o)
    return to(ops_.a), to(ops_.w), out, kw


def emulator(acc):
    """the op emulator with the frame-axis convolution (tests/tconv_spec.py); imported late: that module pulls in the engine"""
    from tconv_spec import TconvEmuOps
    return TconvEmuOps(acc=acc)


def run_emulator(c, ops_, acc, *, storage=None):
    """the whole guarded output buffer after the emulator ran the case, accumulating in `acc` and storing as `storage` (default: the case's type)"""
    T = DT[c.dt] if storage is None else storage
    buf = ops_.buf.to(T).clone()
    a, w, out, kw = gemm_kwargs(c, ops_, buf)
    emulator(acc).gemm(a, w, out, **kw)
    return buf


def bound_terms(c, ops_):
    """S of kernel_compare.compare: the f64 sum of the absolute values of every term the epilogue adds, times |out_scale| - the emulator itself run
    on the operands' absolute values, so the indexing (pitches, row-bias groups, convolution taps, batch stripes) is the emulator's own"""
    ab = Operands(a=ops_.a.abs(), w=ops_.w.abs(), bias=None if ops_.bias is None else ops_.bias.abs(), rb_table=None if ops_.rb_table is None else ops_.rb_table.abs(),
                  residual=None if ops_.residual is None else ops_.residual.abs(), buf=ops_.buf.abs(), mask=ops_.mask)
    cc = replace(c, out_scale=abs(c.out_scale))
    buf = ab.buf.double().clone()
    a, w, out, kw = gemm_kwargs(cc, ab, buf)
    emulator(torch.float64).gemm(a, w, out, **kw)
    return logical(c, buf).clone()


def tile_shape(cfg):
    """(rows, columns) of a tile config (csrc/gemm_kernel.h::dispatch_cfg), for compare's report"""
    bm = 256 if cfg in (3, 4, 5, 7, 12, 13, 14) else 128
    bn = {2: 64, 4: 64, 5: 320, 6: 320, 8: 320, 12: 320, 7: 256, 13: 256, 11: 160}.get(cfg, 128)
    return bm, bn

