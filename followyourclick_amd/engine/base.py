"""Shared host helpers of the UNet / VAE engines: buffer allocation, the fused GroupNorm statistics and thin op wrappers."""
from __future__ import annotations

import os
from typing import Optional, Sequence, Tuple

import torch

from .. import _lib as L

Tensor = torch.Tensor

# Debug aid: ALLOC_FILL = a byte value makes every buffer the engines allocate start as that byte pattern instead of whatever the
# caching allocator hands back (0xFF = NaN in bf16 / f16 / f32 / f64).  A kernel that reads memory nobody wrote - rows past M, partial-sum
# slots the producer skipped - then shows up as a result that depends on the fill: tests/test_uninit_gpu.py runs the forward under two
# fills and demands identical bits.  FYC_ALLOC_FILL=255 sets it from the environment.
ALLOC_FILL = int(os.environ["FYC_ALLOC_FILL"]) if os.environ.get("FYC_ALLOC_FILL") else None


def empty(*shape, dtype, device) -> Tensor:
    t = torch.empty(*shape, dtype=dtype, device=device)
    if ALLOC_FILL is not None and t.numel():
        t.view(torch.uint8).fill_(ALLOC_FILL)
    return t


def conv_out_size(Hin: int, Win: int, stride: int = 1, pad: int = 1, up2: bool = False, up_size=None) -> Tuple[int, int]:
    """output size of the 3x3 convolution (nearest-x2 upsampling folded into its gather: `up_size`, or exactly twice the input)"""
    if up2:
        return up_size if up_size is not None else (2 * Hin, 2 * Win)
    return (Hin + pad - 2) // stride + 1, (Win + pad - 2) // stride + 1


class ChanStats:
    """what the producer of an activation [rows][C] knows about its channel sums, for a GroupNorm whose sample has `out_rows` rows:
    `parts` = the row-tile partial {sum, sum of squares} per channel its epilogue wrote ([tile][slot][C][2] f32: `tile_rows` rows per
    tile, `slots` samples of `stat_rows` rows - a frame - per tile, fyc_gemm_stat_layout), `cs` = the same folded to
    per-(sample of out_rows rows, channel) f64 sums ([rows / out_rows][C][2]): given, or made by EngineBase._stats on first use"""
    __slots__ = ("C", "out_rows", "parts", "tile_rows", "slots", "rows", "stat_rows", "cs")

    def __init__(self, C: int, out_rows: int, parts: Optional[Tensor] = None, tile_rows: int = 0, slots: int = 0, rows: int = 0,
                 stat_rows: int = 0, cs: Optional[Tensor] = None):
        self.C, self.out_rows, self.parts, self.tile_rows, self.slots = C, out_rows, parts, tile_rows, slots
        self.rows, self.stat_rows, self.cs = rows, stat_rows, cs


# The attention call sites beside the UNet - the VAE's mid block (one head of 512) and the encoders (CLIP text: causal; CLIP vision; Resampler) - as one
# fyc_attention launch for the whole batch (ABI 308) instead of zeros + score GEMM + fyc_softmax_rows + P V GEMM.  Per (shape family, dtype word): is the fused
# launch the default?  A family is fused by default iff its slowest fused round beat its fastest materialised round (profiles/wide_attention.txt section 2, the
# criterion of profiles/f32x3_attention.txt); one that lost stays materialised and is reached with FYC_SIDE_FLASH=force.
SIDE_FLASH_DEFAULT = {
    ("vae", "bf16"): False, ("vae", "f16"): False, ("vae", "f32"): False,      # d = 512, 16 x 4096 / 4 x 9216 tokens: fused takes 2.0 - 2.6 x (16-bit), 1.8 - 2.2 x (f32 split) the materialised time
    ("clip_text", "bf16"): True, ("clip_text", "f16"): True, ("clip_text", "f32"): True,
    ("clip_vision", "bf16"): True, ("clip_vision", "f16"): True, ("clip_vision", "f32"): True,
    ("resampler", "bf16"): True, ("resampler", "f16"): True, ("resampler", "f32"): True,
}
_DT_WORD = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}


def side_flash(ops, dtype, family: str, d: int, causal: bool = False) -> bool:
    """Does this call site take the fused launch?  Read at every call, like FYC_F32_FLASH.  The precondition: 16-bit tensors, or f32 with the ops' f32_products ==
    "split" (exact f32 stays materialised: there is no exact fused kernel), and an ops object that answers both capability queries - the CPU emulator of the tests
    and an A/B library of an earlier ABI do not, and keep the materialised sequence call for call.  FYC_SIDE_FLASH: unset / 1 = fused where SIDE_FLASH_DEFAULT says
    so, 0 = never, force = wherever the precondition holds."""
    sw = os.environ.get("FYC_SIDE_FLASH", "1")
    if sw == "0":
        return False
    if dtype == torch.float32 and getattr(ops, "f32_products", "exact") != "split":
        return False
    can_causal, max_d = getattr(ops, "attention_causal_supported", None), getattr(ops, "attention_max_head_dim", None)
    if can_causal is None or max_d is None or d % 8 or d > max_d() or (d > 160 and d % 32) or (causal and not can_causal()):
        return False
    return sw == "force" or SIDE_FLASH_DEFAULT[family, _DT_WORD[dtype]]


class EngineBase:
    """Expects self.ops, self.dtype, self.device and self.groups (GroupNorm group count)."""
    fuse_stats = True           # producers write channel sums in their epilogues
    direct_stats = False        # consumers fold the row-tile partials themselves where _direct allows it (the UNet engine's switch)

    # ---- buffers -----------------------------------------------------------------------------
    def new(self, *shape, dtype=None) -> Tensor:
        return empty(*shape, dtype=dtype or self.dtype, device=self.device)

    def zeros(self, *shape, dtype=None) -> Tensor:
        return torch.zeros(*shape, dtype=dtype or self.dtype, device=self.device)

    # ---- fused statistics: producer -> ChanStats -> consumer ---------------------------------------------------------------------
    def _cs_plan(self, rows: int, stat_rows: int, N: int, K: int, mode: int, out_rows: int) -> Optional[ChanStats]:
        """the row-tile partial buffer for the epilogue of a producer of [rows][N] whose consumer is a GroupNorm over samples of
        out_rows rows, or None when the shape cannot be fused (rows per frame not a multiple of 16, or a row tile would touch more
        than 4 frames)"""
        if not self.fuse_stats or stat_rows % 16 or rows % stat_rows:
            return None
        # small M, long K - the 8x8 latents - run split-K: since ABI 301 its finish kernel writes the same partial sums and
        # fyc_gemm_stat_layout answers for it; an older A/B library (FYC_LIB_PATH) keeps the separate statistics pass
        if getattr(self.ops, "abi_version", L.FYC_VERSION) < 301 and self.ops.gemm_split_bytes(self.dtype, M=rows, N=N, K=K, mode=mode) > 0:
            return None
        nt, tile_rows, slots = self.ops.gemm_stat_layout(self.dtype, M=rows, N=N, K=K, cs_rows=stat_rows, mode=mode)
        if not 1 <= slots <= 4:
            return None
        return ChanStats(N, out_rows, parts=self.new(nt * slots * N * 2, dtype=torch.float32), tile_rows=tile_rows, slots=slots, rows=rows,
                         stat_rows=stat_rows)

    def _produced(self, st: Optional[ChanStats]) -> Optional[ChanStats]:
        """behind the producer that wrote st.parts: the reduce launch right away, unless consumers may fold the partials themselves"""
        if st is not None and not self.direct_stats:
            self._stats(st)
        return st

    def _stats(self, st: ChanStats) -> Tensor:
        """the reduced f64 sums at the consumer's granularity: one fyc_chan_stats_reduce launch, on first use"""
        if st.cs is None:
            st.cs = self.new(st.rows // st.out_rows, st.C, 2, dtype=torch.float64)
            self.ops.chan_stats_reduce(st.parts, st.cs, rows=st.rows, N=st.C, cs_rows=st.stat_rows, tile_rows=st.tile_rows, slots=st.slots,
                                       out_rows=st.out_rows)
        return st.cs

    def _direct_limit(self) -> int:
        """bytes of partials one consumer block may re-read (read per call: the UNet engine answers with its module-level cut-off)"""
        return 0

    def _direct(self, sts: Sequence[ChanStats], rows_per_sample: int) -> Optional[int]:
        """bytes of partials one consumer block reads when it folds the row-tile partials of `sts` itself, or None where it should not:
        sums already reduced, sources with different statistics samples, or more than the cut-off per block (the wide clip-level
        norms of the 64x64 and 32x32 levels: hundreds of KB per block against one small launch)"""
        if not self.direct_stats or any(st.parts is None or st.cs is not None for st in sts):
            return None
        srows = sts[0].stat_rows
        if any(st.stat_rows != srows for st in sts) or rows_per_sample % srows:
            return None
        nbytes = 0
        for st in sts:
            tiles = rows_per_sample // st.tile_rows if rows_per_sample % st.tile_rows == 0 else (rows_per_sample - 1) // st.tile_rows + 2
            nbytes += max(tiles, 1) * st.slots * st.C * 8
        return nbytes if nbytes <= self._direct_limit() else None

    def gn_from_stats(self, srcs: Sequence[Tuple[Tensor, Optional[ChanStats]]], gamma: Tensor, beta: Tensor, rows: int,
                      rows_per_sample: int, eps: float, silu: bool, groups: Optional[int] = None) -> Optional[Tensor]:
        """GroupNorm (+SiLU) of one activation, or of the channel concat of two, from their producers' sums: the one
        fyc_gn_apply_cs call.  None when a source has no sums at this granularity (the caller runs the statistics pass).
        `groups`: a norm whose group count is not the model's (TemporalConvBlock: always 32)."""
        sts = [st for _, st in srcs]
        if any(st is None or st.out_rows != sts[0].out_rows for st in sts) or rows_per_sample % sts[0].out_rows:
            return None
        s1 = sts[0]
        kw = {}
        if len(srcs) == 2:
            kw.update(x2=srcs[1][0], C2=sts[1].C)
        if self._direct(sts, rows_per_sample) is not None:      # every source from its partials (same rows per statistics sample)
            cs1 = None
            kw.update(parts1=s1.parts, tile_rows1=s1.tile_rows, slots1=s1.slots, parts_cs_rows=s1.stat_rows)
            if len(srcs) == 2:
                kw.update(parts2=sts[1].parts, tile_rows2=sts[1].tile_rows, slots2=sts[1].slots)
        else:
            cs1 = self._stats(s1)
            if len(srcs) == 2:
                kw.update(cs2=self._stats(sts[1]))
            kw.update(cs_rows=s1.out_rows)
        y = self.new(rows, sum(st.C for st in sts))
        self.ops.gn_apply_cs(srcs[0][0], cs1, gamma, beta, y, rows=rows, C1=s1.C, groups=groups or self.groups, rows_per_sample=rows_per_sample,
                             eps=eps, silu=silu, **kw)
        return y

    def _up_phases_group(self, w: Tensor, w_ph: Optional[Tensor], frames: int, Hin: int, Win: int, Ho: int, Wo: int, out_rows: int) -> int:
        """input rows per group G of the four-phase form of an upsampling convolution (fyc_conv_up_phases: K = 4 Cin instead of 9 Cin), or 0 where
        today's FYC_GEMM_CONV3X3_UP2 launch runs: no phase weights, a size that is not exactly 2x (`up_size` of an odd level), f32, an ops
        object without the op (the CPU emulator and the recording backend of the tests, an A/B library), FYC_UP_PHASES=0, or a group the kernel's
        row tiles do not divide (per-frame norms at 8x8).  `out_rows`: output rows per sample of the consuming GroupNorm - a clip's or a frame's;
        a group is that sample's input rows, so that the epilogue's partial sums fold to it."""
        supported = getattr(self.ops, "conv_up_phases_supported", None)
        if (w_ph is None or supported is None or os.environ.get("FYC_UP_PHASES", "1") == "0" or self.dtype not in (torch.bfloat16, torch.float16)
                or (Ho, Wo) != (2 * Hin, 2 * Win)):
            return 0
        G = out_rows // 4 if out_rows else Hin * Win
        if G <= 0 or G % (Hin * Win) or (frames * Hin * Win) % G:
            return 0
        Cout, K = w.shape
        return G if supported(self.dtype, Cin=K // 9, Cout=Cout, Hin=Hin, Win=Win, group_rows=G, exact2=True) else 0

    def conv_stats(self, x: Tensor, w: Tensor, b: Tensor, frames: int, Hin: int, Win: int, nxt=None, per_frame: bool = False,
                   stride: int = 1, pad: int = 1, up2: bool = False, up_size=None, w_ph: Optional[Tensor] = None, **kw) -> Tuple[Tensor, Optional[ChanStats]]:
        """a 3x3 convolution whose output feeds a GroupNorm -> (output, its ChanStats or None).  `nxt` = (rows per statistics
        sample of the epilogue = one frame, rows per sample of the norm); per_frame: a per-frame norm, whatever size comes out.
        `w_ph` (up2): the phase weights beside `w` (engine/weights.py::pack_conv_up_phases) - where _up_phases_group allows, the four-phase
        launch runs and its statistics are per (group, phase) over VIRTUAL rows: stat_rows = G, out_rows = 4 G, which fyc_chan_stats_reduce and
        the consumers' own fold take as they are"""
        Cout, K = w.shape
        Ho, Wo = conv_out_size(Hin, Win, stride, pad, up2, up_size)
        if per_frame:
            nxt = (Ho * Wo, Ho * Wo)
        G = self._up_phases_group(w, w_ph, frames, Hin, Win, Ho, Wo, nxt[1] if nxt is not None else 0) if up2 and not kw else 0
        if G:
            st = None
            if nxt is not None and self.fuse_stats:
                nt, tile_rows, slots = self.ops.conv_up_phases_stat_layout(self.dtype, frames=frames, Hin=Hin, Win=Win, Cin=K // 9, Cout=Cout, group_rows=G)
                st = ChanStats(Cout, 4 * G, parts=self.new(nt * slots * Cout * 2, dtype=torch.float32), tile_rows=tile_rows, slots=slots,
                               rows=frames * Ho * Wo, stat_rows=G)
            out = self.new(frames * Ho * Wo, Cout)
            self.ops.conv_up_phases(x, w_ph, out, frames=frames, Hin=Hin, Win=Win, Cin=K // 9, Cout=Cout, group_rows=G, bias=b,
                                    chan_parts=None if st is None else st.parts)
            return out, self._produced(st)
        st = None
        if nxt is not None:
            st = self._cs_plan(frames * Ho * Wo, nxt[0], Cout, K, L.GEMM_CONV3X3_UP2 if up2 else L.GEMM_CONV3X3, nxt[1])
        out = self.conv(x, w, b, frames, Hin, Win, stride=stride, pad=pad, up2=up2, up_size=up_size, stats=st, **kw)
        return out, self._produced(st)

    # ---- primitive helpers -------------------------------------------------------------------
    def lin(self, x: Tensor, w: Tensor, rows: int, bias=None, residual=None, geglu=False, out=None) -> Tensor:
        N, K = w.shape
        cols = N // 2 if geglu else N
        out = out if out is not None else self.new(rows, cols, dtype=x.dtype)
        self.ops.gemm(x, w, out, M=rows, N=N, K=K, lda=K, ldw=K, ldo=cols, bias=bias, residual=residual, ldr=cols,
                      epilogue=L.EPI_GEGLU if geglu else L.EPI_LINEAR)
        return out

    def conv(self, x: Tensor, w: Tensor, b: Tensor, frames: int, Hin: int, Win: int, stride: int = 1, up2: bool = False,
             rowbias=None, rpb: int = 1, residual=None, ldrb: int = 0, up_size=None, pad: int = 1, stats: Optional[ChanStats] = None) -> Tensor:
        """`stats` (EngineBase._cs_plan): the epilogue also writes the row-tile partial channel sums"""
        Cout, K = w.shape
        Cin = K // 9
        Ho, Wo = conv_out_size(Hin, Win, stride, pad, up2, up_size)
        M = frames * Ho * Wo
        out = self.new(M, Cout)
        self.ops.gemm(x, w, out, M=M, N=Cout, K=K, lda=Cin, ldw=K, ldo=Cout, bias=b, rowbias=rowbias, rows_per_batch=rpb, ldrb=ldrb,
                      residual=residual, ldr=Cout, mode=L.GEMM_CONV3X3_UP2 if up2 else L.GEMM_CONV3X3,
                      conv=dict(Hout=Ho, Wout=Wo, Hin=Hin, Win=Win, Cin=Cin, stride=stride, pad=pad),
                      chan_parts=None if stats is None else stats.parts, cs_rows=0 if stats is None else stats.stat_rows)
        return out

    def group_norm(self, x: Tensor, g: Tensor, b: Tensor, rows: int, C: int, rows_per_sample: int, eps: float, silu: bool,
                   groups: Optional[int] = None) -> Tensor:
        groups = groups or self.groups
        stats = self.new(rows // rows_per_sample, groups, 2, dtype=torch.float64)
        self.ops.gn_stats(x, stats, rows=rows, C_=C, groups=groups, rows_per_sample=rows_per_sample)
        y = self.new(rows, C)
        self.ops.gn_apply(x, stats, g, b, y, rows=rows, C_=C, groups=groups, rows_per_sample=rows_per_sample,
                          eps=eps, silu=silu)
        return y

    def layer_norm(self, x: Tensor, gb, rows: int, C: int, pe=None, pe_div: int = 1, pe_rows: int = 1) -> Tensor:
        y = self.new(rows, C)
        self.ops.layernorm(x, gb[0], gb[1], y, rows=rows, C_=C, eps=1e-5, pe=pe, pe_div=pe_div, pe_rows=pe_rows)
        return y

