"""The fyc_gemm cases of tests/test_gemm_epilogues_gpu.py as data, with what each of them is MEANT to execute.  A helper, not a test module;
no GPU is touched here.

Three users share the list, so that the GPU tests cannot drift away from the kernels they name:
  * tests/test_gemm_cases.py (CPU) writes the cases in the line format of tests/gemm_plan_harness.hip's second mode and compares the
    recorded launch - executed tile config, ring depth, wide, split or not - with the declared intent;
  * tests/test_kernel_compare.py (CPU) runs every case of the LINEAR groups on the emulator in f32 and in f64 accumulation; tests/test_gemm_epilogue_cases.py (CPU) runs a
    torch model of every form of the other groups, and their declared defects, against the bounds of analysis() below;
  * tests/test_gemm_epilogues_gpu.py launches them.

The intent is written down from the rules of csrc/gemm_plan.h as a reader understands them, not computed by a copy of the planner:
  * 16-bit, every pitch a multiple of 8 elements, 16-byte aligned operands: the wide (16-byte, LDS-staged) epilogue, on the tile that was asked
    for; tile 0 is the automatic choice, which is 128x64 (config 2) at every N used here (N = 328, 320 with M < 4096, 40);
  * ring depths other than 2 exist for (1, 3) and, in PLAIN mode, (2, 3) and (2, 4);
  * the 64-byte K-tile configs 8 / 10 cannot stage several row-bias groups per row tile: with rows_per_batch = 96 their 128-byte twins 6 / 1 run.
    The cases keep those combinations (the replacement is a decision worth pinning) and each convolution geometry also runs 8 and 10 WITHOUT a
    row bias, so that 8 and 10 are executed wide in every mode;
  * f32, an output that is not 16-byte aligned or an odd pitch: the narrow per-lane epilogue, which only exists for configs 1 and 2.

The groups geglu, heads, act, lnfold, dualk and t3 (EPILOGUE_GROUPS) carry the rest of fyc_gemm: the GEGLU and head-split epilogues, LINEAR with an activation, the folded
LayerNorm, dual-source K and the unsplit frame-axis convolution.  Their rules, as read from the sources:
  * tile 0 at M < 4096: 128x128 (1) for N a multiple of 128 or above 512 (672, 600, 384), else 128x64 (2) (auto_tile);
  * GEGLU pairs value and gate blocks inside a wave: configs 6 and 11 give a wave an odd number of blocks and the planner runs 5 instead (gemm_plan.h::GEMM_TILES, column `geglu`);
  * the activation family builds the tiles 1, 2 and 6 only, and every planned tile is folded onto one of them (gemm_plan.h::gemm_executed_cfg); it takes no ring depth;
  * HEADS is wide when head_dim % 8 == 0, tokens % 16 == 0, the V^T pitch % 8 == 0 and the segments are 16-byte aligned, unless key 6 or key 7 is set;
  * a residual next to a fold makes the LINEAR epilogue narrow (gemm_plan.h::plan_gemm, `packed && ...`);
  * keys 6 (no wide epilogue) and 7 (no wide head split) act in the planner and are seen by the harness.  Keys 12, 13 and 15 act in gemm_plan.h::gemm_launch_plan
    (the decisions of one launch: the harness calls it for the launch it recorded) - restated here, and tests/test_gemm_cases.py compares the restatement with the library for every case:
        pre      epilogue inputs by DMA under the K loop: a wide launch with a 2-deep ring, at least two K tiles (64 elements each for 16-bit types, 32 on configs 8 / 10), no
                 split-K, no ln_nparts, statistics (if any) as 16-byte aligned stored pairs of an EVEN number of rows, a row bias only where the packed LINEAR epilogue
                 stages it, and key 12 != 1 (pre_staged)
        fast1    the specialised pass 1 of the packed epilogues, unless key 13 = 1: GEGLU then takes the LDS-staged wide form, HEADS the LDS-staged one
        heads_pk the pack-first head split: key 15 = 1 on, 2 off, else M <= 8192 - every wide heads case sets the key, so that the staged form production runs at
                 M > 8192 is reached at M = 336
  * each wide geglu / heads / act / lnfold problem runs once more on its automatic tile with key 12 = 1 (`-k12`): the same expressions on self-loaded inputs, bit for bit.
Every problem is ragged in M, N and K against every tile and every pitch is wider than its row.  A HEADS segment has a guarded buffer of its own (FRONT elements in front,
SEG_BACK behind, the pad columns [tokens, ld) of V^T outside the mask) and is compared as a 2-D window: rows (batch, head, token), or (batch, head, channel) for V^T.
"""
import math
from dataclasses import dataclass, field, replace
from typing import Optional, Tuple

import torch

from test_kernels_gpu import CONV_TILES, F16_TILES, PLAIN_TILES

PLAIN, CONV, UP2, T3 = 0, 1, 2, 3
LINEAR, GEGLU, HEADS = 0, 1, 2
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
    group: str                       # LINEAR_GROUPS: "plain", "narrow", "conv", "pixel", "alias", "stripes", "splitk"; EPILOGUE_GROUPS: "geglu", "heads", "act", "lnfold", "dualk", "t3"
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
    epilogue: int = 0                # LINEAR, GEGLU, HEADS
    act: int = 0                     # 0 none, 1 erf-GELU, 2 quick-GELU
    ln: int = 0                      # folded LayerNorm: 0 none, 1 stored {mean, rstd} pairs, n > 1 = ln_nparts partial {sum, sum sq} pairs per row
    a2: bool = False                 # dual-source K: columns [k_split, K) of the operand come from a second buffer of pitch lda2
    k_split: int = 0
    lda2: int = 0
    heads: Optional[Tuple] = None    # (seg_cols, heads, tokens, transposed per segment, seg_ld per segment (0: tokens), element offset per segment)
    a_guard: int = 0                 # T3: NaN rows in front of and behind the operand
    # ---- what the case is meant to execute ----
    want_cfg: int = 0                # tile config after the narrow-epilogue rewrite
    want_ring: int = 2               # -1: the f32 and the activation entries take none
    want_wide: int = 0
    want_split: bool = False
    want_form: str = ""              # the epilogue form the launch decisions select (head of the file), for the new groups: "packed", "staged", "narrow"
    want_pre: bool = False           # meant to take its epilogue inputs pre-staged under the K loop

    @property
    def conv_dict(self):
        return dict(self.conv) if self.conv is not None else None

    @property
    def cols(self):
        """columns of the output buffer the launch writes: the batch elements of the stripes case lie side by side"""
        return (self.N // 2 if self.epilogue == GEGLU else self.N) * self.batch

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


# ---- the other epilogues of fyc_gemm: GEGLU, head split, activation, folded LayerNorm, dual-source K, unsplit T3 (see the head) -----------------
LINEAR_GROUPS = ("plain", "narrow", "conv", "pixel", "alias", "stripes", "splitk")      # judged by kernel_compare.element_bound through bound_terms()
EPILOGUE_GROUPS = ("geglu", "heads", "act", "lnfold", "dualk", "t3")                    # judged by epilogue_bound() below
TUNE_NO_WIDE, TUNE_NO_WIDE_HEADS, TUNE_NO_PRESTAGE, TUNE_GENERIC_PASS1, TUNE_HEADS_PACKED = 6, 7, 12, 13, 15
ACT_WIDE_TILES = {1: 1, 3: 1, 7: 1, 5: 6, 6: 6}      # gemm_plan.h::gemm_executed_cfg, activation family: what a planned tile runs as, wide; everything else 128x64 (2)
GEGLU_REPLACED = {6: 5, 11: 5}                        # gemm_plan.h::GEMM_TILES, column `geglu`: a wave of these owns an odd number of column blocks


def auto_tile(M, N):
    """gemm_plan.h::plan_gemm, "tile config and ring depth", for M < 4096, 16-bit"""
    assert M < 4096
    if N % 320 == 0:
        return 5 if N >= 5120 else 1 if N >= 2560 else 2
    return 1 if (N % 128 == 0 or N > 512) else 2


def narrow_tile(cfg, N):
    """gemm_plan.h::gemm_executed_cfg, !wide: only configs 1 and 2 are built narrow"""
    return cfg if cfg in (1, 2) else 1 if (N % 128 == 0 or N > 512) else 2


def k_tiles(c, cfg):
    """K tiles per output tile: 128-byte LDS rows, 64-byte ones for configs 8 / 10"""
    bk = (64 if cfg in (8, 10) else 128) // (4 if c.dt == "f32" else 2)
    return -(-c.K // bk)


def pre_staged(c):
    """gemm_plan.h::gemm_launch_plan, q.pre - restated: a wide 2-deep-ring launch with at least two K tiles, unsplit, whose statistics (if any) are stored pairs of an even number
    of rows (16-byte aligned: the harness and the tests pass aligned tables), no row bias outside the packed LINEAR epilogue, and key 12 not set"""
    return bool(c.want_wide == 1 and c.want_ring in (2, -1) and not c.want_split and k_tiles(c, c.want_cfg) >= 2 and c.ln <= 1 and (c.ln == 0 or c.M % 2 == 0) and
                (not c.rowbias or c.epilogue == LINEAR) and dict(c.tuning).get(TUNE_NO_PRESTAGE, 0) != 1)


def _want(dt, M, N, tile, *, narrow=False, act=False, geglu=False, staged=False, packed_heads=None, tuning=()):
    """the intent of a case of the new groups, from the rules of the head of this file"""
    if dt == "f32":
        return dict(want_cfg=1 if N % 128 == 0 else 2, want_ring=-1, want_wide=0, want_form="narrow")
    cfg = tile if tile else auto_tile(M, N)
    if geglu:
        cfg = GEGLU_REPLACED.get(cfg, cfg)
    if narrow:
        return dict(want_cfg=narrow_tile(cfg, N), want_ring=-1 if act else 2, want_wide=0, want_form="narrow")
    if act:
        return dict(want_cfg=ACT_WIDE_TILES.get(cfg, 2), want_ring=-1, want_wide=1, want_form="staged")
    form = "staged" if staged else "packed"
    if packed_heads is not None:
        form = "packed" if (packed_heads and not staged) else "staged"
    return dict(want_cfg=cfg, want_ring=2, want_wide=1, want_form=form)


def _finish(cases):
    """want_pre from the restated conditions; the key-12 twin of every wide problem on its automatic tile"""
    out = []
    for c in cases:
        c = replace(c, want_pre=pre_staged(c))
        out.append(c)
        if c.want_wide and c.tile == 0 and c.group in ("geglu", "heads", "act", "lnfold") and dict(c.tuning).get(TUNE_GENERIC_PASS1, 0) == 0 and c.want_pre:
            out.append(replace(c, name=c.name + "-k12", tuning=c.tuning + ((TUNE_NO_PRESTAGE, 1),), want_pre=False))
    return out


GEGLU_TILES = [0, 1, 2, 3, 4, 5, 7, 8, 10, 6, 11]


def _geglu_cases():
    out = []
    base = dict(group="geglu", mode=PLAIN, epilogue=GEGLU, M=300, N=672, K=136, lda=144, ldw=152, ldo=344)
    for ln in (0, 1):
        for dt in ("bf16", "f16"):
            tag = f"geglu-{dt}-ln{ln}"
            for tile in GEGLU_TILES:
                out.append(Case(name=f"{tag}-t{tile}", dt=dt, ln=ln, tile=tile, **base, **_want(dt, 300, 672, tile, geglu=True)))
            for tile in (0, 1, 5):
                out.append(Case(name=f"{tag}-t{tile}-k13", dt=dt, ln=ln, tile=tile, tuning=((TUNE_GENERIC_PASS1, 1),), **base, **_want(dt, 300, 672, tile, geglu=True, staged=True)))
            out.append(Case(name=f"{tag}-k6", dt=dt, ln=ln, tuning=((TUNE_NO_WIDE, 1),), **base, **_want(dt, 300, 672, 0, geglu=True, narrow=True)))
            out.append(Case(name=f"{tag}-odd", dt=dt, ln=ln, out_off=1, **dict(base, ldo=345), **_want(dt, 300, 672, 0, geglu=True, narrow=True)))
        out.append(Case(name=f"geglu-f32-ln{ln}", dt="f32", ln=ln, **base, **_want("f32", 300, 672, 0)))
    return out


# head geometries (d, H, tokens, batch elements): C = 200, a 16-column block straddles two heads, M = 336 has batch elements across the 128- and 256-row tile borders; C = 128
HEAD_GEOMS = {"d40": (40, 5, 48, 7), "d64": (64, 2, 16, 19), "d12": (12, 5, 77, 4)}
# segment layouts of the engine's call sites: unet3d.py:420 / encoders.py:180 / vae.py:66 (q | k | V^T), unet3d.py:149 / encoders.py:302 (k | V^T), unet3d.py:433 / encoders.py:300 (q)
HEAD_LAYOUTS = {"qkv": (0, 0, 1), "kv": (0, 1), "q": (0,)}


def _heads_case(dt, geom, layout, ln, tile, *, tuning=(), seg_off=0, tag="", **want):
    d, H, tokens, Bn = HEAD_GEOMS[geom]
    tr = HEAD_LAYOUTS[layout]
    ld_t = (tokens + 7) // 8 * 8 + (8 if tokens % 8 == 0 else 0)      # the V^T pitch: 56 for 48 tokens, 24 for 16, 80 for 77
    M, N = Bn * tokens, len(tr) * H * d
    hd = (H * d, H, tokens, tr, tuple(ld_t if t else 0 for t in tr), tuple(seg_off for _ in tr))
    return Case(name=f"heads-{geom}-{layout}-{dt}-ln{ln}-t{tile}{tag}", group="heads", dt=dt, mode=PLAIN, epilogue=HEADS, M=M, N=N, K=136, lda=144, ldw=152, ldo=0, out_scale=0.75,
                ln=ln, tile=tile, tuning=tuning, heads=hd, **_want(dt, M, N, tile, **want))


def _heads_cases():
    out = []
    pk = lambda v: ((TUNE_HEADS_PACKED, v),)
    for dt in ("bf16", "f16"):
        for key, tag in ((1, "-pk"), (2, "-st")):
            for ln in (0, 1):
                for tile in (0, 1, 5, 6, 11):
                    out.append(_heads_case(dt, "d40", "qkv", ln, tile, tuning=pk(key), tag=tag, packed_heads=key == 1))
            for layout in ("kv", "q"):
                for tile in (0, 5):
                    out.append(_heads_case(dt, "d40", layout, 1, tile, tuning=pk(key), tag=tag, packed_heads=key == 1))
            for tile in (0, 6):
                out.append(_heads_case(dt, "d64", "qkv", 0, tile, tuning=pk(key), tag=tag, packed_heads=key == 1))
        for layout in ("kv", "q"):
            out.append(_heads_case(dt, "d64", layout, 1, 0, tuning=pk(2), tag="-st", packed_heads=False))
        out.append(_heads_case(dt, "d40", "qkv", 1, 1, tuning=pk(1) + ((TUNE_GENERIC_PASS1, 1),), tag="-pk-k13", packed_heads=True, staged=True))
        out.append(_heads_case(dt, "d40", "qkv", 0, 0, tuning=((TUNE_NO_WIDE_HEADS, 1),), tag="-k7", narrow=True))
        out.append(_heads_case(dt, "d12", "qkv", 1, 0, seg_off=4, narrow=True))
    out.append(_heads_case("f32", "d12", "qkv", 1, 0, seg_off=4))
    for ln in (0, 1):
        out.append(_heads_case("f32", "d40", "qkv", ln, 0))
    out.append(_heads_case("f32", "d64", "qkv", 0, 0))
    return out


ACT_TILES = [0, 1, 2, 6, 5]      # 5 is planned and runs the family's 128x320 instantiation (6)


def _act_cases():
    out = []
    base = dict(group="act", mode=PLAIN, M=300, N=328, K=136, lda=144, ldw=152, ldo=336, ldr=344, residual=1, out_scale=0.75)
    for act in (1, 2):
        for dt in ("bf16", "f16"):
            for tile in ACT_TILES:
                out.append(Case(name=f"act{act}-{dt}-t{tile}", dt=dt, act=act, tile=tile, **base, **_want(dt, 300, 328, tile, act=True)))
            out.append(Case(name=f"act{act}-{dt}-odd", dt=dt, act=act, **dict(base, ldo=329), **_want(dt, 300, 328, 0, act=True, narrow=True)))
        out.append(Case(name=f"act{act}-f32", dt="f32", act=act, **base, **_want("f32", 300, 328, 0)))
    return out


def _lnfold_cases():
    out = []
    base = dict(group="lnfold", mode=PLAIN, N=328, K=136, lda=144, ldw=152, ldo=336, ldr=344)
    for dt in ("bf16", "f16"):
        for tile in (0, 1, 5, 6):
            out.append(Case(name=f"lnfold-{dt}-m300-t{tile}", dt=dt, M=300, ln=1, tile=tile, **base, **_want(dt, 300, 328, tile)))
        for tile in (0, 5):      # an odd M: the statistics cannot come as 16-byte pairs, the epilogue loads them itself
            out.append(Case(name=f"lnfold-{dt}-m301-t{tile}", dt=dt, M=301, ln=1, tile=tile, **base, **_want(dt, 301, 328, tile)))
            out.append(Case(name=f"lnfold-{dt}-parts3-t{tile}", dt=dt, M=300, ln=3, tile=tile, **base, **_want(dt, 300, 328, tile)))
        # a residual next to the fold: planned narrow (gemm_plan.h::plan_gemm)
        out.append(Case(name=f"lnfold-{dt}-res", dt=dt, M=300, ln=1, residual=1, out_scale=0.75, **base, **_want(dt, 300, 328, 0, narrow=True)))
    for M, ln in ((300, 1), (301, 1), (300, 3)):
        out.append(Case(name=f"lnfold-f32-m{M}-ln{ln}", dt="f32", M=M, ln=ln, residual=1, out_scale=0.75, **base, **_want("f32", M, 328, 0)))
    return out


def _dualk_cases():
    out = []
    for ks, K2, lda, lda2 in ((64, 136, 72, 144), (128, 64, 136, 72)):
        base = dict(group="dualk", mode=PLAIN, M=300, N=328, K=ks + K2, lda=lda, ldw=ks + K2 + 8, ldo=336, ldr=344, residual=1, out_scale=0.75, a2=True, k_split=ks, lda2=lda2)
        for dt in ("bf16", "f16"):
            for tile in (0, 1, 5, 6):
                out.append(Case(name=f"dualk{ks}-{dt}-t{tile}", dt=dt, tile=tile, **base, **_want(dt, 300, 328, tile)))
        out.append(Case(name=f"dualk{ks}-f32", dt="f32", **base, **_want("f32", 300, 328, 0)))
    return out


def _t3_cases():
    """unsplit: 5 clips x 3 frames x 20 rows - the 128- and 256-row tiles straddle frames and clips"""
    out = []
    for Cin in (64, 128):
        base = dict(group="t3", mode=T3, M=300, N=328, K=3 * Cin, lda=Cin, ldw=3 * Cin + 8, ldo=336, ldr=344, residual=1, out_scale=1.25, a_guard=21,
                    conv=(("Cin", Cin), ("frames", 3), ("rows", 20)))
        for dt, (tile, ring) in _dt_tiles(CONV_TILES, F16_TILES):
            out.append(Case(name=f"t3-c{Cin}-{dt}-t{tile}r{ring}", dt=dt, tile=tile, ring=ring, **base, **_intent(dt, tile, ring, T3, staged_rb=False),
                            want_form="narrow" if dt == "f32" else "packed"))
    return out


CASES = _finish(_plain_cases() + _conv_cases() + _alias_cases() + _stripe_cases() + _splitk_cases() +
                _geglu_cases() + _heads_cases() + _act_cases() + _lnfold_cases() + _dualk_cases() + _t3_cases())
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
    if c.epilogue or c.act:
        f.update(epilogue=c.epilogue, act=c.act)
    if c.ln:
        f.update(ln=1, ln_nparts=c.ln if c.ln > 1 else 0)
    if c.a2:
        f.update(a2=1, k_split=c.k_split, lda2=c.lda2)
    if c.heads is not None:
        sc, H, tokens, tr, ld, off = c.heads
        f.update(seg_cols=sc, heads=H, tokens=tokens, seg_tr=",".join(map(str, tr)), seg_ld=",".join(map(str, ld)), seg_off=",".join(str((FRONT + o) * es) for o in off))
        del f["out_off"]
    toks =[c.name] + [f"{k}={v}" for k, v in f.items()] + [f"tune={k}:{v}" for k, v in c.all_tuning if v]
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
    # the new groups (epilogue_operands): one guarded buffer per HEADS segment in bufs / masks (buf / mask are the first), the second K source, the fold's inputs
    bufs: Optional[list] = field(repr=False, default=None)
    masks: Optional[list] = field(repr=False, default=None)
    a2: Optional[torch.Tensor] = None
    ln_stats: Optional[torch.Tensor] = None
    ln_colsum: Optional[torch.Tensor] = None
    a_buf: Optional[torch.Tensor] = field(repr=False, default=None)      # T3: the operand between its NaN guard rows


def out_offset(c):
    return FRONT + c.out_off


def buf_len(c):
    return out_offset(c) + (c.M + BACK_ROWS) * c.ldo


def logical(c, buf):
    """the [M][columns] window of an output buffer that the launch writes"""
    return torch.as_strided(buf, (c.M, c.cols), (c.ldo, 1), buf.storage_offset() + out_offset(c))


def operands(c):
    """the CPU operands of a case, the same values for every tile of a problem (seeded by the operand, not by the case)"""
    if c.epilogue or c.act or c.ln or c.a2 or c.a_guard:      # a feature of the EPILOGUE_GROUPS (tests/f32x3_spec.py has LINEAR cases of its own, one of them named t3)
        return epilogue_operands(c)
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
    if c.heads is not None:      # out_buf: the list of guarded segment buffers
        sc, H, tokens, tr, ld, off = c.heads
        out = None
        hd = dict(seg_cols=sc, heads=H, tokens=tokens, outs=[b[FRONT + o:] for b, o in zip(out_buf, off)], transposed=list(tr), ld=list(ld))
    else:
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
    if c.heads is not None:
        kw["heads"] = hd
        del kw["ldo"]
    if c.batch > 1:
        kw.update(batch=c.batch, stride_a=c.stride_a, stride_w=c.stride_w, stride_o=c.stride_o)
    if c.epilogue:
        kw["epilogue"] = c.epilogue
    if c.act:
        kw["act"] = c.act
    if c.ln:
        kw.update(ln_stats=to(ops_.ln_stats), ln_colsum=to(ops_.ln_colsum), ln_nparts=c.ln if c.ln > 1 else 0, ln_eps=LN_EPS)
    if c.a2:
        kw.update(a2=to(ops_.a2), k_split=c.k_split, lda2=c.lda2)
    if c.a_guard:
        return to(ops_.a_buf)[c.a_guard:c.a_guard + c.M], to(ops_.w), out, kw
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
    """(rows, columns) of a tile config (csrc/gemm_plan.h::GEMM_TILES), for compare's report"""
    bm = 256 if cfg in (3, 4, 5, 7, 12, 13, 14) else 128
    bn = {2: 64, 4: 64, 5: 320, 6: 320, 8: 320, 12: 320, 7: 256, 13: 256, 11: 160}.get(cfg, 128)
    return bm, bn


# =========================================================================================================================================
# The new groups: operands, the f64 analysis behind their per-element bounds (derivation: the head of tests/kernel_compare.py), the windows a
# case is compared in, a torch model of the kernel's forms and the declared defects
# =========================================================================================================================================
LN_EPS = 1e-5
SEG_BACK = 64                    # guard elements behind a HEADS segment
u = 2.0 ** -24
AS_P = 0.3275911                 # gelu_erf_f (csrc/fyc_common.h:190-199)
AS_A = (1.061405429, -1.453152027, 1.421413741, -0.284496736, 0.254829592)      # Horner order
QUICK_C = 1.702
DQ = 1.10                        # |d/dx (x sigmoid(1.702 x))| <= 1.0998; asserted on a grid by tests/test_gemm_epilogue_cases.py
GEGLU_GATE_BIAS = 1.5            # added to the bias of every gate column (epilogue_operands says why)
EXP_U = RSQRT_U = 2.0           # the exp2 instruction behind __expf, rsqrtf: 1 ulp documented = up to 2 u relative (as tests/norm_cases.py has them)


def _f32c(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _seeded(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def seg_geometry(c, s):
    """(rows, cols, pitch, elements) of segment s as a 2-D window: [(batch, head, token)][channel], or for a transposed one [(batch, head, channel)][token] with pitch ld"""
    sc, H, tokens, tr, ld, off = c.heads
    d, Bn = sc // H, c.M // tokens
    if tr[s]:
        pitch = ld[s] if ld[s] > 0 else tokens
        return Bn * H * d, tokens, pitch, Bn * H * d * pitch
    return Bn * H * tokens, d, d, Bn * H * tokens * d


def epilogue_operands(c):
    """the CPU operands of a case of the new groups: seeded by the operand and the problem, the same for every tile and tuning key"""
    T = DT[c.dt]
    ops_ = Operands(a=None, w=None, bias=None, rb_table=None, residual=None, buf=None)
    Ka = c.k_split if c.a2 else (c.conv_dict["Cin"] if c.mode == T3 else c.K)
    a = _seeded((c.M, c.lda), 1)
    if c.ln:      # rows with |mean| / std up to 4, either sign
        a = a + 4.0 * (2.0 * torch.rand((c.M, 1), generator=torch.Generator().manual_seed(11)) - 1.0)
    ops_.a = a.to(T)
    if c.a2:
        ops_.a2 = _seeded((c.M, c.lda2), 7).to(T)
    if c.a_guard:
        ops_.a_buf = torch.full((c.M + 2 * c.a_guard, c.lda), float("nan"), dtype=T)
        ops_.a_buf[c.a_guard:c.a_guard + c.M] = ops_.a
    ops_.w = _seeded((c.N, c.ldw), 2, 1 / math.sqrt(c.K)).to(T)
    # GEGLU: the polynomial gate is off by up to PHI_ERR = 1.4e-4 on Phi, i.e. by delta = PHI_ERR / Phi(g) of the output: 1.4e-4 for a large gate, 9e-4 at g = -1.  A relative
    # shift delta carries an f16 element across a rounding boundary with probability delta / s (s the relative spacing, 4.9e-4 .. 9.8e-4) and then costs s, so a row or column
    # has an expected relative L2 of sqrt(delta s): 3e-4 .. 9e-4 beside f16's line tolerance of 5e-4.  A line of mostly negative gates fails that tolerance with nothing wrong
    # (the model of this file: column 269 at 5.1e-4 with gates centred on 0).  The gates are therefore centred on GEGLU_GATE_BIAS (deviation 1.03, 7 % negative: every column's
    # mean gate above 0.5, asserted by tests/test_gemm_epilogue_cases.py); each element, whatever the sign of its gate, is bounded on its own
    ops_.bias = _seeded((c.N,), 3, 0.25 if c.epilogue == GEGLU else 1.0) if c.bias else None
    if c.epilogue == GEGLU:
        ops_.bias.reshape(c.N // 32, 2, 16)[:, 1] += GEGLU_GATE_BIAS
    ops_.residual = _seeded((c.M, c.ldr), 4).to(T) if c.residual == 1 else None
    if c.ln:
        x = ops_.a[:, :Ka].double()
        ops_.ln_colsum = ops_.w[:, :c.K].double().sum(dim=1).float()
        if c.ln == 1:
            ops_.ln_stats = torch.stack([x.mean(dim=1), (x.var(dim=1, unbiased=False) + LN_EPS).rsqrt()], dim=1).float().contiguous()
        else:     # the producer's partial {sum, sum sq} over c.ln column ranges
            edges = [round(i * Ka / c.ln) for i in range(c.ln + 1)]
            ops_.ln_stats = torch.stack([torch.stack([x[:, lo:hi].sum(dim=1), (x[:, lo:hi] ** 2).sum(dim=1)], dim=1) for lo, hi in zip(edges, edges[1:])], dim=1).float().contiguous()
    if c.heads is None:
        ops_.buf = prefill(buf_len(c), T)
        ops_.mask = torch.zeros(buf_len(c), dtype=torch.bool)
        logical(c, ops_.mask).fill_(True)
        ops_.bufs, ops_.masks = [ops_.buf], [ops_.mask]
    else:
        ops_.bufs, ops_.masks = [], []
        for s, o in enumerate(c.heads[5]):
            rows, cols, pitch, n = seg_geometry(c, s)
            ops_.bufs.append(prefill(FRONT + o + n + SEG_BACK, T))
            m = torch.zeros(FRONT + o + n + SEG_BACK, dtype=torch.bool)
            torch.as_strided(m, (rows, cols), (pitch, 1), FRONT + o).fill_(True)      # the pad columns [tokens, ld) of V^T stay False
            ops_.masks.append(m)
        ops_.buf, ops_.mask = ops_.bufs[0], ops_.masks[0]
    return ops_


def windows(c):
    """[(name, buffer index, view(buffer) -> the 2-D window, Labels)] of a case"""
    from kernel_compare import Labels
    if c.heads is None:
        bm, bn = tile_shape(c.want_cfg)
        bo = bn // 2 if c.epilogue == GEGLU else bn
        lab = Labels(lambda i: f"row tile {i // bm} of {bm} rows, row {i % bm} in it, 16-row pass {i % bm // 16}",
                     lambda j: f"column tile {j // bo} of {bo} output columns, column {j % bo} in it, lane column {j % 16}")
        return [("out", 0, lambda buf: logical(c, buf), lab)]
    sc, H, tokens, tr, ld, off = c.heads
    d = sc // H
    out = []
    for s in range(len(tr)):
        rows, cols, pitch, _ = seg_geometry(c, s)
        view = (lambda buf, rows=rows, cols=cols, pitch=pitch, o=off[s]: torch.as_strided(buf, (rows, cols), (pitch, 1), buf.storage_offset() + FRONT + o))
        if tr[s]:
            lab = Labels(lambda i: f"batch {i // (H * d)}, head {i // d % H}, channel {i % d}", lambda j: f"token {j}, 8-token run {j // 8}")
        else:
            lab = Labels(lambda i: f"batch {i // (H * tokens)}, head {i // tokens % H}, token {i % tokens}", lambda j: f"channel {j}")
        out.append((f"seg{s}" + ("T" if tr[s] else ""), s, view, lab))
    return out


def to_windows(c, t):
    """a [M][output columns] tensor in the coordinates of the windows of the case"""
    if c.heads is None:
        return [t]
    sc, H, tokens, tr, ld, off = c.heads
    d, Bn = sc // H, c.M // tokens
    out = []
    for s in range(len(tr)):
        seg = t[:, s * sc:(s + 1) * sc].reshape(Bn, tokens, H, d)
        out.append(seg.permute(0, 2, 3, 1).reshape(Bn * H * d, tokens) if tr[s] else seg.permute(0, 2, 1, 3).reshape(Bn * H * tokens, d))
    return out


def operand_matrix(c, ops_, defect=None):
    """[M][K] in the K order of the weights, as stored (no conversion): the two sources of a dual-source problem side by side, the three taps of T3 gathered"""
    if c.mode == T3:
        from tconv_spec import gather_t3
        conv = c.conv_dict
        frames = c.M // conv["rows"] if defect == "t3_across_clips" else conv["frames"]      # defect: one clip of all the frames - a tap is read across every clip border
        return gather_t3(ops_.a, M=c.M, Cin=conv["Cin"], frames=frames, rows=conv["rows"])
    if not c.a2:
        return ops_.a[:, :c.K]
    ks = c.k_split
    if defect == "a2_lda":                # the second source indexed with the first one's pitch
        flat = ops_.a2.reshape(-1)
        idx = (torch.arange(c.M)[:, None] * c.lda + torch.arange(c.K - ks)[None, :]).clamp_max(flat.numel() - 1)
        return torch.cat([ops_.a[:, :ks], flat[idx]], dim=1)
    if defect == "k_switch_late":         # the K tile [ks, ks + 64) still read from the first source (which has run into its next row by then)
        flat = ops_.a.reshape(-1)
        idx = (torch.arange(c.M)[:, None] * c.lda + torch.arange(ks, ks + 64)[None, :]).clamp_max(flat.numel() - 1)
        return torch.cat([ops_.a[:, :ks], flat[idx], ops_.a2[:, 64:c.K - ks]], dim=1)
    return torch.cat([ops_.a[:, :ks], ops_.a2[:, :c.K - ks]], dim=1)


def gelu_exact(x):
    return 0.5 * x * (1.0 + torch.special.erf(x / math.sqrt(2.0)))


def gelu_as(x):
    """gelu_erf_f in f64 with the f32 constants of the source -> (value, first-order bound of its f32 evaluation error, operation by operation: csrc/fyc_common.h:191-198).
    z = |g| c (u z); d = fma(p, z, 1) (u d); t = rcp(d) (1 ulp: 2 u); four fma of the Horner form (u each); poly * t (u); z * z (u); __expf = exp2(x log2e): the product
    (u |x| in natural units), log2e as an f32 constant (0.25 u |x|), the instruction (EXP_U u); * (u); 2 - e (u); 0.5 g exact; the last product (u)"""
    x = x.double()
    z = x.abs() * _f32c(0.70710678118654752440)
    ez = u * z
    d = _f32c(AS_P) * z + 1.0
    ed = _f32c(AS_P) * ez + u * d
    t = 1.0 / d
    et = t * ed / d + 2 * u * t
    p, ep = torch.full_like(t, _f32c(AS_A[0])), torch.zeros_like(t)
    for cf in AS_A[1:]:
        pn = p * t + _f32c(cf)
        ep = t * ep + p.abs() * et + u * pn.abs()
        p = pn
    pt = p * t
    ept = t * ep + p.abs() * et + u * pt.abs()
    zz = z * z
    ezz = 2 * z * ez + u * zz
    E = torch.exp(-zz)
    eE = E * (ezz + 1.25 * u * zz + EXP_U * u)
    e = pt * E
    ee = E * ept + pt.abs() * eE + u * e.abs()
    val = 0.5 * x * torch.where(x >= 0, 2.0 - e, e)
    err = 0.5 * x.abs() * (ee + torch.where(x >= 0, u * (2.0 - e), torch.zeros_like(e))) + u * val.abs()
    return val, err


def gelu_as_error(lo=-12.0, hi=12.0, n=(1 << 21) + 1):
    """max |gelu_erf_f - x Phi(x)| of the Abramowitz-Stegun form itself, in f64 on a dense grid (beyond |x| = 12 e^(-x^2 / 2) is below 1e-31 and both sides are x or 0)"""
    g = torch.linspace(lo, hi, n, dtype=torch.float64)
    return float((gelu_as(g)[0] - gelu_exact(g)).abs().max())


GELU_AS_ERR = gelu_as_error()      # what the bounds use; never a number copied from a comment


def quick_gelu(x):
    """x sigmoid(1.702 x) in f64 -> (value, first-order bound of activate()'s f32 evaluation, csrc/gemm_kernel.h::activate: the product -1.702f x (u |a|), __expf (u |a| + 0.25 u |a| +
    EXP_U u, as in gelu_as), 1 + E (u), the division (u; HIP divides f32 correctly rounded), and 1.702f against the reference's 1.702 (|a| |1.702f / 1.702 - 1|))"""
    x = x.double()
    a = QUICK_C * x
    E = torch.exp(-a)
    val = x / (1.0 + E)
    rE = a.abs() * (2.25 * u + abs(_f32c(QUICK_C) / QUICK_C - 1.0)) + EXP_U * u
    return val, x.abs() * E / (1.0 + E) ** 2 * rE + 2 * u * val.abs()


def fold_terms(c, ops_):
    """(mu, rs, dmu, drs) per row, f64 [M][1]: the statistics the REFERENCE folds with and how far the kernel's may lie from them.  Stored pairs: both sides read the same f32
    numbers.  ln_nparts (csrc/gemm_kernel.h::ln_row): a chain of n - 1 f32 additions per sum, inv = 1.0f / K and a product each, mu * mu, the subtraction, + eps, rsqrtf - against
    the exact values of the same f32 partials; the reference's own f32 evaluation (EmuOps.gemm) is measured against them as well and added"""
    if c.ln == 1:
        st = ops_.ln_stats.double()
        z = torch.zeros(c.M, 1, dtype=torch.float64)
        return st[:, 0:1], st[:, 1:2], z, z
    import norm_cases as NC
    K, n = c.K, c.ln
    parts = ops_.ln_stats.reshape(c.M, n, 2)
    pr = parts.float().sum(dim=1)                                       # as EmuOps.gemm has it
    mean_ref = pr[:, 0] / K
    rs_ref = torch.rsqrt((pr[:, 1] / K - mean_ref * mean_ref).clamp_min(0) + LN_EPS)
    s, q = parts[:, :, 0].double().sum(dim=1), parts[:, :, 1].double().sum(dim=1)
    mu, eps = s / K, _f32c(LN_EPS)
    var = (q / K - mu * mu).clamp_min(0)
    rs = (var + eps).rsqrt()
    dmu = (n - 1) * u * parts[:, :, 0].double().abs().sum(dim=1) / K + 2 * u * mu.abs()
    dvar = (n - 1) * u * q / K + 2 * u * q / K + 2 * mu.abs() * dmu + u * mu * mu
    rho, _ = NC.norm_rho(var, dvar, eps)
    dmu = dmu + (mean_ref.double() - mu).abs()
    drs = rs * rho + (rs_ref.double() - rs).abs()
    e = lambda t: t.reshape(c.M, 1)
    return e(mean_ref.double()), e(rs_ref.double()), e(dmu), e(drs)


def analysis(c, ops_):
    """(val, rest): the exact value of every output element in f64, [M][output columns], and its bound WITHOUT the ulp_T(ref) of the store (head of tests/kernel_compare.py)"""
    from row_panel_cases import DG, PHI_ERR, Phi, phi_rounding
    A, W = operand_matrix(c, ops_).double(), ops_.w[:, :c.K].double()
    acc, Sacc = A @ W.t(), A.abs() @ W.abs().t()
    b = ops_.bias.double()[None, :] if c.bias else torch.zeros(1, c.N, dtype=torch.float64)
    if c.ln:
        mu, rs, dmu, drs = fold_terms(c, ops_)
        cs = ops_.ln_colsum.double()[None, :]
        pre = rs * (acc - mu * cs) + b
        S = rs * (Sacc + (mu * cs).abs()) + b.abs()
        extra = drs * (acc - mu * cs).abs() + rs * dmu * cs.abs()
    else:
        pre, S, extra = acc + b, Sacc + b.abs(), 0.0
    E = (c.K + 8) * u * S + extra
    sc = abs(c.out_scale)
    res = torch.as_strided(ops_.residual, (c.M, c.N), (c.ldr, 1)).double() if c.residual == 1 else torch.zeros(1, 1, dtype=torch.float64)
    if c.epilogue == GEGLU:
        blk, eb = pre.reshape(c.M, c.N // 32, 2, 16), E.reshape(c.M, c.N // 32, 2, 16)
        v, g, dv, dg = blk[:, :, 0], blk[:, :, 1], eb[:, :, 0], eb[:, :, 1]
        if c.dt != "f32" and c.want_wide:      # the polynomial gate (geglu_pair): as the row-panel bound has it
            gate = g * Phi(g)
            val = v * gate
            rest = dv * gate.abs() + v.abs() * (DG * dg + g.abs() * (PHI_ERR + phi_rounding(g))) + DG * dv * dg + 3 * u * val.abs()
        else:                                  # gelu_erf_f, one product
            gate = gelu_exact(g)
            val = v * gate
            rest = dv * gate.abs() + v.abs() * (DG * dg + GELU_AS_ERR + gelu_as(g)[1]) + DG * dv * dg + u * val.abs()
        return val.reshape(c.M, c.N // 2), rest.reshape(c.M, c.N // 2)
    if c.act:
        if c.act == 1:
            y, ey = gelu_exact(pre), DG * E + GELU_AS_ERR + gelu_as(pre)[1]
        else:
            y, ev = quick_gelu(pre)
            ey = DQ * E + ev
        return (y + res) * c.out_scale, sc * (ey + 2 * u * (y.abs() + res.abs()))
    # LINEAR and HEADS: the residual and the scale are two more of the K + 8 roundings, as kernel_compare.element_bound has them
    return (pre + res) * c.out_scale, sc * ((c.K + 8) * u * (S + res.abs()) + extra)


def epilogue_reference(c, ops_):
    """(reference buffers, [bound per window]): EmuOps(acc=float64) as it stands, run into copies of the guarded buffers; bound = ulp_T of what it stored + analysis()'s rest.
    The exact values of analysis() must round to what the emulator stored, to within one unit: that ties the bound's indexing to the emulator's"""
    from kernel_compare import ulp
    T = DT[c.dt]
    bufs = [b.clone() for b in ops_.bufs]
    a, w, out, kw = gemm_kwargs(c, ops_, bufs if c.heads is not None else bufs[0])
    emulator(torch.float64).gemm(a, w, out, **kw)
    val, rest = analysis(c, ops_)
    bounds = []
    for (name, bi, view, lab), v, r in zip(windows(c), to_windows(c, val), to_windows(c, rest)):
        ref = view(bufs[bi]).double()
        assert ((v.to(T).double() - ref).abs() <= ulp(ref, c.dt)).all(), f"{c.name} {name}: the analysis and the emulator disagree"
        bounds.append(ulp(ref, c.dt) + r)
    return bufs, bounds


def judge(c, ops_, got_bufs, ref_bufs, bounds):
    """every window of a case through kernel_compare.compare(bound=...): global, per row, per column, per element, and nothing outside the mask written"""
    from kernel_compare import RTOL, Guard, compare
    figs = []
    for (name, bi, view, lab), bound in zip(windows(c), bounds):
        got = got_bufs[bi].cpu()
        figs.append(compare(view(got), view(ref_bufs[bi]), dtype=c.dt, bound=bound, rtol=RTOL[c.dt], labels=lab, lines=True, guard=Guard(ops_.bufs[bi], got, ops_.masks[bi]),
                            tag=f"{c.name} {name}"))
    return figs


def problem_key(c):
    """what operands, reference and bound depend on: not the tile, the tuning keys or the intent - except that the bound of a GEGLU case knows which gate its form
    evaluates (the polynomial in the 16-bit wide forms, gelu_erf_f elsewhere), so that bit of the intent stays in the key"""
    return replace(c, name="", tile=0, ring=0, tuning=(), chan=False, cs_rows=0, want_cfg=0, want_ring=0, want_wide=int(c.dt != "f32" and c.want_wide and c.epilogue == GEGLU),
                   want_split=False, want_form="", want_pre=False)


# ---- the torch model of the kernel's forms: f32 tensors combined in the kernel's order ----------------------------------------------------------
def _gelu_as32(g):
    """gelu_erf_f in f32, operation by operation (the reciprocal and the exponential correctly rounded, where the kernel's are within 1 ulp)"""
    from row_panel_cases import fma32
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    z = g.abs() * f(0.70710678118654752440)
    t = 1.0 / fma32(f(AS_P), z, f(1.0))
    p = fma32(f(AS_A[0]), t, f(AS_A[1]))
    for cf in AS_A[2:]:
        p = fma32(p, t, f(cf))
    e = p * t * torch.exp(-(z * z))
    return (0.5 * g) * torch.where(g >= 0, 2.0 - e, e)


def _gelu_tanh32(g):
    return 0.5 * g * (1.0 + torch.tanh(0.7978845608028654 * (g + 0.044715 * g * g * g)))


DEFECTS = {
    "geglu": ("crossed_pair",),                                     # value and gate blocks crossed for one 16-column pair
    "heads": ("straddle_first_head", "vt_run_shifted", "vt_pad_write"),
    "lnfold": ("stats_next_row", "fold_after_bias"),
    "dualk": ("a2_lda", "k_switch_late"),
    "t3": ("t3_across_clips",),
    "act": ("act_after_residual", "gelu_tanh"),
}


def model(c, ops_, defect=None):
    """the guarded buffers after a torch model of the form the case declares (want_form, want_wide) ran: the f32 matrix product, the fold as the source has it - two packed
    FMAs in the packed forms (gemm_kernel.h::epilogue_linear_packed, epilogue_heads_packed, epilogue_geglu_packed), a product and a difference elsewhere (the three forms of gemm_epilogue itself) -, the polynomial or the Abramowitz-Stegun gate, the
    residual and the scale in the source's order, one rounding to the storage type.  `defect`: one of DEFECTS, planted at a single site"""
    from row_panel_cases import fma32, geglu32
    T = DT[c.dt]
    A, W = operand_matrix(c, ops_, defect).float(), ops_.w[:, :c.K].float()
    acc = A @ W.t()
    b = ops_.bias[None, :] if c.bias else torch.zeros(1, c.N)
    scale = torch.tensor(c.out_scale, dtype=torch.float32)
    packed = c.want_form == "packed"
    if c.ln:
        mu, rs = fold_terms(c, ops_)[:2]
        if c.ln > 1:      # the kernel's own chain (gemm_kernel.h::ln_row)
            parts = ops_.ln_stats.reshape(c.M, c.ln, 2)
            t = parts[:, 0].clone()
            for i in range(1, c.ln):
                t = t + parts[:, i]
            inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(c.K), dtype=torch.float32)
            m32 = t[:, 0] * inv
            mu, rs = m32[:, None], torch.rsqrt((t[:, 1] * inv - m32 * m32).clamp_min(0) + torch.tensor(LN_EPS, dtype=torch.float32))[:, None]
        mu, rs = mu.float(), rs.float()
        if defect == "stats_next_row":
            mu, rs = mu.roll(-1, 0), rs.roll(-1, 0)
        cs = ops_.ln_colsum[None, :]
        if defect == "fold_after_bias":
            pre = rs * ((acc + b) - mu * cs)
        elif packed and c.epilogue == HEADS:      # out = fma(acc, rs * scale, scale * fma(-rs mu, colsum, bias))
            pre = fma32(acc, rs * scale, scale * fma32(-rs * mu, cs, b))
        elif packed:
            pre = fma32(acc, rs, fma32(-rs * mu, cs, b))
        else:
            pre = rs * (acc - mu * cs) + b
    else:
        pre = acc + b
    res = torch.as_strided(ops_.residual, (c.M, c.N), (c.ldr, 1)).float() if c.residual == 1 else None
    if c.epilogue == GEGLU:
        blk = pre.reshape(c.M, c.N // 32, 2, 16)
        v, g = blk[:, :, 0].clone(), blk[:, :, 1].clone()
        if defect == "crossed_pair":
            v[:, 7], g[:, 7] = blk[:, 7, 1], blk[:, 7, 0]
        y = geglu32(v, g) if (c.dt != "f32" and c.want_wide) else v * _gelu_as32(g)
        out = y.reshape(c.M, c.N // 2)
    elif c.epilogue == HEADS:
        out = pre if (packed and c.ln and defect != "fold_after_bias") else pre * scale
    else:
        y = pre
        if c.act and defect == "act_after_residual":
            y = y + res
            res = None
        if c.act == 1:
            y = _gelu_tanh32(y) if defect == "gelu_tanh" else _gelu_as32(y)
        elif c.act == 2:
            y = y / (1.0 + torch.exp(torch.tensor(-QUICK_C, dtype=torch.float32) * y))
        if res is not None:
            y = y + res
        out = y * scale
    bufs = [b_.clone() for b_ in ops_.bufs]
    for (name, bi, view, lab), wv in zip(windows(c), to_windows(c, out)):
        view(bufs[bi]).copy_(wv.to(T))
    if c.heads is not None and defect in DEFECTS["heads"]:
        sc_, H, tokens, tr, ld, off = c.heads
        d = sc_ // H
        if defect == "straddle_first_head":
            # the 16-column block [32, 48) of segment 0 covers head 0's channels 32..39 and head 1's 0..7: written wholly to head 0, whose "channels 40..47" are the next token's 0..7
            assert d == 40 and not tr[0]
            s0, fresh = FRONT + off[0], ops_.bufs[0]
            w0, f0 = view_of(c, 0, bufs[0]), view_of(c, 0, fresh)
            vals = w0.reshape(-1, H, tokens, d)[:, 1, :, 0:8].clone()                                  # what head 1 should have got
            w0.reshape(-1, H, tokens, d)[:, 1, :, 0:8] = f0.reshape(-1, H, tokens, d)[:, 1, :, 0:8]      # ... stays unwritten
            flat = bufs[0][s0:]
            Bn = c.M // tokens
            for bb in range(Bn):
                for t in range(tokens):
                    o = ((bb * H + 0) * tokens + t) * d + 40
                    flat[o:o + 8] = vals[bb, t]
        else:
            s = tr.index(1)
            rows, cols, pitch, _ = seg_geometry(c, s)
            wv, fv = view_of(c, s, bufs[s]), view_of(c, s, ops_.bufs[s])
            row = (1 * H + min(2, H - 1)) * d + 5                      # batch 1, head 2, channel 5
            if defect == "vt_run_shifted":
                run = wv[row, 8:16].clone()
                wv[row, 8:16] = fv[row, 8:16]
                torch.as_strided(bufs[s], (8,), (1,), FRONT + off[s] + row * pitch + 16).copy_(run)
            else:                                                       # vt_pad_write: eight values behind the last token of a V^T row
                assert pitch >= tokens + 8 or pitch > tokens
                n = min(8, pitch - tokens)
                torch.as_strided(bufs[s], (n,), (1,), FRONT + off[s] + row * pitch + tokens).copy_(wv[row, :n].clone())
    return bufs


def view_of(c, s, buf):
    return windows(c)[s][2](buf)

