"""Tensor-level wrappers over the C ABI (include/fyc.h).

torch is plumbing here: it owns device memory and the stream; every op below only forwards raw
``data_ptr()``s and sizes to libfyc_hip.so.  There is no CPU implementation in the product: a tensor
that is not on a HIP device raises.  (The engine reaches these functions through the module-level
``impl`` object so that the CPU test-suite can exercise the host orchestration with an op emulator
that lives under tests/ - never in the product path.)
"""
from __future__ import annotations

import os

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib as L
from . import default_f32_products

Tensor = torch.Tensor


_DTYPE_CODES = {torch.bfloat16: L.FYC_BF16, torch.float16: L.FYC_F16, torch.float32: L.FYC_F32}


_PRODUCTS = {"exact": L.PRODUCTS_EXACT, "split": L.PRODUCTS_SPLIT_BF16}      # the words of HipOps.f32_products and of the `products` keyword -> the f32_products field (resolve_f32_products)


def resolve_f32_products(op: str, dtype: torch.dtype, products: Optional[str], instance_mode: str, *, fused_exact: bool = True) -> int:
    """The f32_products field of fyc_gemm_args / fyc_tattn_args / fyc_attn_args (include/fyc.h) for one call of entry point `op` on activations of `dtype`:
    the `products` keyword, or with None the HipOps instance's mode, on f32 tensors; 0 on 16-bit tensors whatever the mode.  An unknown word raises ValueError,
    "split" with 16-bit tensors TypeError.  fused_exact=False (attention): there is no fused kernel with exact f32 products, f32 tensors that resolve to
    "exact" raise FycError.  A pure function: the emulators of tests/ take the same decision from it."""
    if products is not None and products not in _PRODUCTS:
        raise ValueError(f"{op}: products {products!r}: expected None, 'exact' or 'split'")
    if dtype != torch.float32:
        if products == "split":
            raise TypeError(f"{op}: products='split' needs float32 tensors (got {dtype})")
        return L.PRODUCTS_EXACT
    mode = instance_mode if products is None else products
    if mode == "exact" and not fused_exact:
        raise L.FycError(f"{op}: float32 tensors run fused with products='split' only; with exact f32 products use the materialised path "
                         "(gemm, softmax_rows, gemm: engine/unet3d.py::_attend)")
    return _PRODUCTS[mode]


def _dtc(dtype: torch.dtype) -> int:
    """torch dtype of the activations / weights -> fyc_dtype (include/fyc.h): bf16 production, f16 (the reference's deployed
    fp16-autocast precision class), f32 parity mode"""
    try:
        return _DTYPE_CODES[dtype]
    except KeyError:
        raise TypeError(f"unsupported activation dtype {dtype}") from None


def _dt(t: Tensor) -> int:
    return _dtc(t.dtype)


def _p(t: Optional[Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise L.FycError("followyourclick_amd ops need HIP device tensors; there is no CPU fallback")
    return t.data_ptr()


def _f32(t: Optional[Tensor], what: str) -> Optional[int]:
    if t is not None and t.dtype != torch.float32:
        raise TypeError(f"{what} must be float32")
    return _p(t)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda idx: torch.cuda.current_stream(idx).cuda_stream)


class HipOps:
    """The product backend: libfyc_hip.so on the current torch HIP stream."""

    name = "hip"

    def __init__(self):
        self.lib = L.load()
        self.abi_version = int(self.lib.fyc_version())        # (differs from _lib.FYC_VERSION only for an A/B library, FYC_LIB_PATH)
        # longest clip temporal_attention() takes (UNet3DEngine._rope asks): 256 frames with the long-clip kernel, 64 for an A/B library from before it
        self.temporal_attention_max_frames = 256 if hasattr(self.lib, "fyc_temporal_attention_long") else 64
        self._zero = None
        self._ws = None              # scratch for split-K GEMMs: one buffer, grown on demand (all work is on one stream)
        self._ws_need = {}           # (shape, flags) -> split-K scratch bytes (fyc_gemm_workspace_bytes), see gemm()
        self._rescale_ws = None      # moments partials + factors of cfg_ddim_step_rescaled (its own buffer: a growing split-K scratch must not move it)
        self._q_cache = {}           # host-side layout queries (row parts, split bytes, statistics layout) per shape
        self._inited_dev = None
        self.f32_products = default_f32_products()      # "exact" | "split": the product rule of gemm(), attention() and temporal_attention() on f32 tensors (set_f32_products, resolve_f32_products)

    # -- library ---------------------------------------------------------------------------
    def ensure_init(self, device: torch.device) -> None:
        """One GPU per process (the library's zero page and tuning table are process-wide; the multi-GPU path is one process
        per GPU): the first device used is bound, any other raises."""
        if self._inited_dev is not None and getattr(device, "index", None) == self._inited_dev:
            return                                             # the ~900 calls of a DDIM step take this exit
        if not torch.cuda.is_available():
            raise L.FycError("no HIP device visible: followyourclick_amd has no CPU fallback")
        device = torch.device(device)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if self._inited_dev == idx:
            return
        if self._inited_dev is not None:
            raise L.FycError(f"followyourclick_amd is bound to cuda:{self._inited_dev}; use one process per GPU (asked for cuda:{idx})")
        self._zero = torch.zeros(4096, dtype=torch.uint8, device=torch.device("cuda", idx))
        L.check(self.lib.fyc_init(self._zero.data_ptr()), "fyc_init")
        self._inited_dev = idx
        for kv in filter(None, os.environ.get("FYC_TUNING", "").split(",")):   # A/B runs: FYC_TUNING="5=1,4=8" (fyc_set_tuning keys)
            k, v = kv.split("=")
            self.set_tuning(int(k), int(v))

    def device_caps(self):
        caps = (L.i64 * 8)()
        L.check(self.lib.fyc_device_caps(caps), "fyc_device_caps")
        return list(caps)

    def set_tuning(self, key: int, value: int) -> None:
        L.check(self.lib.fyc_set_tuning(key, value), "fyc_set_tuning")
        self._ws_need.clear()        # tile / split-K decisions depend on the tuning table
        self._q_cache.clear()

    def set_f32_products(self, mode: str) -> None:
        """"exact" or "split": the product rule of every later gemm(), temporal_attention() and attention() on f32 tensors that does not pass `products` itself
        (include/fyc.h, fyc_gemm_args.f32_products / fyc_tattn_args.f32_products / fyc_attn_args.f32_products); 16-bit tensors are not affected.  attention() on f32
        tensors exists in "split" only: in "exact" the engine takes the materialised path and a direct call raises.  A captured graph (FYC_HIPGRAPH=1) replays the
        mode it was captured in."""
        if mode not in _PRODUCTS:
            raise ValueError(f"f32 products {mode!r}: expected 'exact' or 'split'")
        self.f32_products = mode
        self._ws_need.clear()
        self._q_cache.clear()

    def _stream(self) -> int:
        """raw hipStream_t of torch's CURRENT stream on the bound device (a `with torch.cuda.stream(...)` block is honoured);
        the raw getter costs ~0.3 us, torch.cuda.current_stream().cuda_stream ~8 us - a third of the host time of a launch"""
        return _raw_stream(self._inited_dev if self._inited_dev is not None else torch.cuda.current_device())

    def _call(self, name: str, args) -> None:
        L.check(getattr(self.lib, name)(C.byref(args), self._stream()), name)

    # -- GEMM family -------------------------------------------------------------------------
    def gemm(self, a: Tensor, w: Tensor, out: Optional[Tensor], *, M: int, N: int, K: int, lda: int, ldw: int,
             ldo: int = 0, bias: Optional[Tensor] = None, rowbias: Optional[Tensor] = None, rows_per_batch: int = 1,
             residual: Optional[Tensor] = None, ldr: int = 0, ldrb: int = 0, out_scale: float = 1.0, epilogue: int = L.EPI_LINEAR,
             mode: int = L.GEMM_PLAIN, conv: Optional[dict] = None, batch: int = 1, stride_a: int = 0,
             stride_w: int = 0, stride_o: int = 0, heads: Optional[dict] = None, tile: int = 0,
             a2: Optional[Tensor] = None, k_split: int = 0, lda2: int = 0, act: int = L.ACT_NONE,
             ln_stats: Optional[Tensor] = None, ln_colsum: Optional[Tensor] = None, ln_nparts: int = 0, ln_eps: float = 1e-5,
             chan_parts: Optional[Tensor] = None, cs_rows: int = 0, row_parts: Optional[Tensor] = None, row_nparts: int = 0,
             products: Optional[str] = None) -> None:
        """products: None = this instance's f32_products, else "exact" / "split" (f32 tensors only: "split" with 16-bit tensors raises)"""
        self.ensure_init(a.device)
        f32_products = resolve_f32_products("gemm", a.dtype, products, self.f32_products)
        g = self._gemm_args(a, w, out, M=M, N=N, K=K, lda=lda, ldw=ldw, ldo=ldo, bias=bias, rowbias=rowbias, rows_per_batch=rows_per_batch,
                            residual=residual, ldr=ldr, ldrb=ldrb, out_scale=out_scale, epilogue=epilogue, mode=mode, conv=conv, batch=batch,
                            stride_a=stride_a, stride_w=stride_w, stride_o=stride_o, heads=heads, tile=tile, a2=a2, k_split=k_split,
                            lda2=lda2, act=act, ln_stats=ln_stats, ln_colsum=ln_colsum, ln_nparts=ln_nparts, ln_eps=ln_eps,
                            chan_parts=chan_parts, cs_rows=cs_rows, row_parts=row_parts, row_nparts=row_nparts)
        g.f32_products = f32_products
        # split-K scratch (small M, long K): the decision depends on the shape and the flags below only - cached, so that the ~300
        # GEMM launches of a DDIM step do not each pay a second ctypes call.  One grown-on-demand buffer: all work of a process is on
        # ONE stream (the engine's), a second stream would need its own HipOps.
        key = (M, N, K, mode, epilogue, act, batch, tile, g.dtype, ln_stats is not None, chan_parts is not None, row_parts is not None)
        need = self._ws_need.get(key)
        if need is None:
            need = int(self.lib.fyc_gemm_workspace_bytes(C.byref(g))) if hasattr(self.lib, "fyc_gemm_workspace_bytes") else 0
            self._ws_need[key] = need
        if need > 0:
            if self._ws is None or self._ws.numel() < need or self._ws.device != a.device:
                self._ws = torch.empty(need, dtype=torch.uint8, device=a.device)
            g.workspace, g.workspace_bytes = self._ws.data_ptr(), self._ws.numel()
        self._call("fyc_gemm", g)

    def gemm_row_parts(self, dtype: torch.dtype, *, M: int, N: int, K: int, mode: int = L.GEMM_PLAIN, batch: int = 1, tile: int = 0) -> int:
        """column tiles fyc_gemm will use for this problem = row_nparts of its `row_parts` output (fyc_gemm_row_parts)"""
        key = ("rp", dtype, M, N, K, mode, batch, tile)
        if key not in self._q_cache:
            g = L.GemmArgs()
            g.M, g.N, g.K, g.mode, g.batch, g.tile = M, N, K, mode, batch, tile
            g.dtype = _dtc(dtype)
            self._q_cache[key] = int(self.lib.fyc_gemm_row_parts(C.byref(g))) if hasattr(self.lib, "fyc_gemm_row_parts") else 0
        return self._q_cache[key]

    def gemm_split_bytes(self, dtype: torch.dtype, *, M: int, N: int, K: int, mode: int = L.GEMM_PLAIN) -> int:
        """scratch bytes a plain LINEAR-epilogue problem of this shape would use for split-K (0: it runs unsplit)"""
        key = ("sb", dtype, M, N, K, mode)
        if key not in self._q_cache:
            g = L.GemmArgs()
            g.M, g.N, g.K, g.mode, g.batch, g.epilogue = M, N, K, mode, 1, L.EPI_LINEAR
            g.dtype = _dtc(dtype)
            self._q_cache[key] = int(self.lib.fyc_gemm_workspace_bytes(C.byref(g))) if hasattr(self.lib, "fyc_gemm_workspace_bytes") else 0
        return self._q_cache[key]

    def gemm_stat_layout(self, dtype: torch.dtype, *, M: int, N: int, K: int, cs_rows: int, mode: int = L.GEMM_PLAIN, batch: int = 1,
                         tile: int = 0):
        """(row tiles, rows per tile, sample slots per tile) of the `chan_parts` output of this problem (fyc_gemm_stat_layout)"""
        key = ("sl", dtype, M, N, K, cs_rows, mode, batch, tile)
        if key not in self._q_cache:
            if not hasattr(self.lib, "fyc_gemm_stat_layout"):       # an older A/B library (FYC_LIB_PATH): no fused statistics
                self._q_cache[key] = (0, 0, 0)
            else:
                g = L.GemmArgs()
                g.M, g.N, g.K, g.mode, g.batch, g.tile, g.cs_rows = M, N, K, mode, batch, tile, cs_rows
                g.dtype = _dtc(dtype)
                tr, sl = L.i32(0), L.i32(0)
                n = int(self.lib.fyc_gemm_stat_layout(C.byref(g), C.byref(tr), C.byref(sl)))
                self._q_cache[key] = (n, int(tr.value), int(sl.value))
        return self._q_cache[key]

    def chan_stats_reduce(self, parts: Tensor, cs: Tensor, *, rows: int, N: int, cs_rows: int, tile_rows: int, slots: int,
                          out_rows: int = 0) -> None:
        if cs.dtype != torch.float64:
            raise TypeError("channel statistics must be float64")
        a = L.ChanStatsReduceArgs()
        a.parts, a.cs, a.rows, a.N, a.cs_rows, a.tile_rows, a.slots = _f32(parts, "parts"), _p(cs), rows, N, cs_rows, tile_rows, slots
        a.out_rows = out_rows
        self._call("fyc_chan_stats_reduce", a)

    # -- nearest-2x upsample + 3x3 convolution as four 2x2 phase convolutions (include/fyc.h, fyc_conv_up_phases) ---------------
    def conv_up_phases_supported(self, dtype: torch.dtype, *, Cin: int, Cout: int, Hin: int, Win: int, group_rows: int, exact2: bool = True) -> bool:
        """does fyc_conv_up_phases cover this shape?  (no launch; an A/B library of an earlier build, FYC_LIB_PATH, has no such entry: False)"""
        if not hasattr(self.lib, "fyc_conv_up_phases_supported") or dtype not in (torch.bfloat16, torch.float16):
            return False
        key = ("cups", dtype, Cin, Cout, Hin, Win, group_rows, bool(exact2))
        if key not in self._q_cache:
            self._q_cache[key] = bool(self.lib.fyc_conv_up_phases_supported(_dtc(dtype), Cin, Cout, Hin, Win, group_rows, int(bool(exact2))))
        return self._q_cache[key]

    @staticmethod
    def _conv_up_phases_args(dtype_code: int, frames: int, Hin: int, Win: int, Cin: int, Cout: int, ldw: int, ldo: int, group_rows: int):
        u = L.ConvUpPhasesArgs()
        g = u.gemm
        g.M, g.N, g.K, g.lda, g.ldw, g.ldo = 4 * frames * Hin * Win, Cout, 4 * Cin, Cin, ldw, ldo
        g.mode, g.epilogue, g.batch, g.out_scale, g.dtype = L.GEMM_CONV3X3_UP2, L.EPI_LINEAR, 1, 1.0, dtype_code
        g.Hout, g.Wout, g.Hin, g.Win, g.Cin, g.conv_stride, g.conv_pad = 2 * Hin, 2 * Win, Hin, Win, Cin, 1, 1
        u.group_rows = group_rows
        return u

    def conv_up_phases_stat_layout(self, dtype: torch.dtype, *, frames: int, Hin: int, Win: int, Cin: int, Cout: int, group_rows: int):
        """(row tiles, rows per tile, slots = 1) of the `chan_parts` output of conv_up_phases over its virtual rows (fyc_conv_up_phases_stat_layout)"""
        key = ("cupl", dtype, frames, Hin, Win, Cin, Cout, group_rows)
        if key not in self._q_cache:
            u = self._conv_up_phases_args(_dtc(dtype), frames, Hin, Win, Cin, Cout, 4 * Cin, Cout, group_rows)
            tr, sl = L.i32(0), L.i32(0)
            n = int(self.lib.fyc_conv_up_phases_stat_layout(C.byref(u), C.byref(tr), C.byref(sl)))
            self._q_cache[key] = (n, int(tr.value), int(sl.value))
        return self._q_cache[key]

    def conv_up_phases(self, x: Tensor, w_ph: Tensor, out: Tensor, *, frames: int, Hin: int, Win: int, Cin: int, Cout: int, group_rows: int,
                       bias: Optional[Tensor] = None, ldo: int = 0, chan_parts: Optional[Tensor] = None) -> None:
        """out [frames * 2 Hin * 2 Win][ldo] = conv3x3(nearest-2x(x)) + bias from the phase weights w_ph [4][Cout][4 * Cin]
        (engine/weights.py::pack_conv_up_phases); chan_parts: per (group of group_rows input rows, phase) partial sums"""
        self.ensure_init(x.device)
        if x.dtype != w_ph.dtype:
            raise TypeError(f"conv_up_phases: activation {x.dtype} vs weight {w_ph.dtype}")
        u = self._conv_up_phases_args(_dt(x), frames, Hin, Win, Cin, Cout, w_ph.shape[-1], ldo or Cout, group_rows)
        g = u.gemm
        g.a, g.w, g.bias, g.out = _p(x), _p(w_ph), _f32(bias, "bias"), _p(out)
        g.chan_parts, g.cs_rows = _f32(chan_parts, "chan_parts"), (group_rows if chan_parts is not None else 0)
        self._call("fyc_conv_up_phases", u)

    @staticmethod
    def _gemm_args(a, w, out, *, M, N, K, lda, ldw, ldo, bias, rowbias, rows_per_batch, residual, ldr, ldrb, out_scale, epilogue, mode,
                   conv, batch, stride_a, stride_w, stride_o, heads, tile, a2, k_split, lda2, act, ln_stats, ln_colsum, ln_nparts,
                   ln_eps, chan_parts, cs_rows, row_parts, row_nparts):
        g = L.GemmArgs()
        g.a, g.w, g.bias, g.rowbias = _p(a), _p(w), _f32(bias, "bias"), _f32(rowbias, "rowbias")
        g.residual, g.out = _p(residual), _p(out)
        g.M, g.N, g.K, g.lda, g.ldw, g.ldo, g.ldr, g.ldrb = M, N, K, lda, ldw, ldo, ldr, ldrb
        g.stride_a, g.stride_w, g.stride_o, g.batch = stride_a, stride_w, stride_o, batch
        g.mode, g.epilogue, g.rows_per_batch, g.out_scale, g.dtype = mode, epilogue, rows_per_batch, out_scale, _dt(a)
        g.tile, g.act = tile, act
        g.ln_stats, g.ln_colsum = _f32(ln_stats, "ln_stats"), _f32(ln_colsum, "ln_colsum")
        g.a2, g.k_split, g.lda2 = _p(a2), k_split, lda2
        if a.dtype != w.dtype:
            raise TypeError(f"gemm: activation {a.dtype} vs weight {w.dtype}")
        if conv is not None and mode == L.GEMM_CONV_T3:      # 3 taps along the frame axis: channels, frames per clip, rows per frame
            g.Cin, g.t3_frames, g.t3_rows = conv["Cin"], conv["frames"], conv["rows"]
        elif conv is not None:
            g.Hout, g.Wout, g.Hin, g.Win, g.Cin, g.conv_stride = (conv["Hout"], conv["Wout"], conv["Hin"], conv["Win"],
                                                                  conv["Cin"], conv.get("stride", 1))
            g.conv_pad = conv.get("pad", 1)
        if heads is not None:
            g.seg_cols, g.heads, g.tokens = heads["seg_cols"], heads["heads"], heads["tokens"]
            for i, (t, tr, ld) in enumerate(zip(heads["outs"], heads["transposed"], heads["ld"])):
                g.seg_out[i], g.seg_transposed[i], g.seg_ld[i] = _p(t), int(tr), int(ld)
        g.ln_nparts, g.ln_eps = ln_nparts, ln_eps
        g.chan_parts, g.cs_rows = _f32(chan_parts, "chan_parts"), cs_rows
        g.row_parts, g.row_nparts = _f32(row_parts, "row_parts"), row_nparts
        return g

    # -- attention ---------------------------------------------------------------------------
    def attention(self, q: Tensor, k: Tensor, vt: Tensor, o: Tensor, *, batch: int, heads: int, n_q: int, n_k: int,
                  d: int, ldo: int, ldvt: int, scale: float, kv_batch_div: int = 1, accumulate: bool = False,
                  o_scale: float = 1.0, q_batch_mod: int = 0, products: Optional[str] = None, causal: bool = False) -> None:
        """q_batch_mod > 0: q holds q_batch_mod batch elements, element b attends with the q of b % q_batch_mod.
        causal: key j counts for query i iff j <= i (n_q == n_k, q_batch_mod == 0): fyc_attention_masked.  d: a multiple of 8 up to 160, or of 32 up to attention_max_head_dim().
        products: None = this instance's f32_products (the switch gemm() reads), else "exact" / "split" (f32 tensors only: "split" with 16-bit tensors
        raises; with 16-bit tensors and None the field stays 0 whatever the instance's mode).  f32 tensors run the fused kernel with split-bf16 products
        only (include/fyc.h): a resolved "exact" raises - the exact f32 mode is the materialised sequence gemm / softmax_rows / gemm (engine/unet3d.py::_attend)"""
        f32_products = resolve_f32_products("attention", q.dtype, products, self.f32_products, fused_exact=False)
        self.ensure_init(q.device)
        m = L.AttnMaskArgs()
        a = m.attn
        a.q, a.k, a.vt, a.o = _p(q), _p(k), _p(vt), _p(o)
        a.batch, a.heads, a.n_q, a.n_k, a.d, a.ldo, a.ldvt = batch, heads, n_q, n_k, d, ldo, ldvt
        a.kv_batch_div, a.o_accumulate, a.scale, a.o_scale, a.dtype = kv_batch_div, int(accumulate), scale, o_scale, _dt(q)
        a.q_batch_mod, a.f32_products = q_batch_mod, f32_products
        if not causal:
            self._call("fyc_attention", a)      # (the entry every earlier ABI has: an A/B library takes these calls unchanged)
            return
        m.causal = 1
        self._call("fyc_attention_masked", m)

    def attention_q_batch_mod_supported(self) -> bool:
        return True

    def attention_causal_supported(self) -> bool:
        """attention(causal=True) exists (ABI 308; an A/B library of an earlier ABI, FYC_LIB_PATH, has no fyc_attention_masked)"""
        return self.abi_version >= 308

    def attention_max_head_dim(self) -> int:
        """the largest d attention() takes: 512 (multiples of 32 above 160) from ABI 308 on, 160 before"""
        return 512 if self.abi_version >= 308 else 160

    def repeat(self, src: Tensor, dst: Tensor, *, times: int) -> None:
        """dst = `times` back-to-back copies of src (both contiguous, any dtype)"""
        self.ensure_init(src.device)
        nbytes = src.numel() * src.element_size()
        if src.dtype != dst.dtype or dst.numel() != times * src.numel() or not (src.is_contiguous() and dst.is_contiguous()):
            raise ValueError("repeat: dst must be a contiguous tensor of src's dtype holding `times` copies of src")
        a = L.RepeatArgs()
        a.src, a.dst, a.bytes, a.times = src.data_ptr(), dst.data_ptr(), nbytes, times
        self._call("fyc_repeat", a)

    def temporal_attention(self, qkv: Tensor, o: Tensor, *, clips: int, frames: int, pixels: int, heads: int, d: int,
                           scale: float, rope: Optional[Tuple[Tensor, Tensor]] = None, products: Optional[str] = None,
                           kernel: Optional[str] = None) -> None:
        """rope = (cos, sin): f32 device tables [frames][d/2]; q and k are rotated per frame before the score product (include/fyc.h).
        products: None = this instance's f32_products (the switch gemm() reads), else "exact" / "split" (f32 tensors only: "split" with 16-bit tensors
        raises; with 16-bit tensors and None the field stays 0 whatever the instance's mode)
        kernel: None = fyc_temporal_attention (frames <= 256; the long-clip kernel above 64 frames); "long" = fyc_temporal_attention_long, the
        long-clip kernel for any 16 < frames <= 256 (16-bit tensors only)"""
        if kernel not in (None, "long"):
            raise ValueError(f"temporal_attention: kernel {kernel!r}: expected None or 'long'")
        f32_products = resolve_f32_products("temporal_attention", qkv.dtype, products, self.f32_products)
        self.ensure_init(qkv.device)
        a = L.TAttnArgs()
        a.qkv, a.o, a.clips, a.frames, a.pixels, a.heads, a.d, a.scale, a.dtype = (_p(qkv), _p(o), clips, frames, pixels,
                                                                                  heads, d, scale, _dt(qkv))
        if rope is not None:
            cos, sin = rope
            for t in (cos, sin):
                if t.dtype != torch.float32 or not t.is_contiguous() or t.device != qkv.device or tuple(t.shape) != (frames, d // 2):
                    raise ValueError(f"temporal_attention: rope tables must be contiguous f32 [{frames}][{d // 2}] tensors on {qkv.device}")
            a.rope_cos, a.rope_sin = cos.data_ptr(), sin.data_ptr()
        a.f32_products = f32_products
        self._call("fyc_temporal_attention_long" if kernel == "long" else "fyc_temporal_attention", a)

    def _tblock_args(self, x, out, w_qkv, colsum, bias, pe_bias, w_out, b_out, clips, frames, pixels, heads, d, scale, eps):
        a = L.TemporalBlockArgs()
        a.x, a.out, a.w_qkv, a.w_out = _p(x), _p(out), _p(w_qkv), _p(w_out)
        a.colsum, a.bias, a.pe_bias, a.b_out = _f32(colsum, "colsum"), _f32(bias, "bias"), _f32(pe_bias, "pe_bias"), _f32(b_out, "b_out")
        a.clips, a.frames, a.pixels, a.heads, a.d, a.C = clips, frames, pixels, heads, d, heads * d
        a.scale, a.eps, a.dtype = scale, eps, _dt(x)
        return a

    def temporal_block_supported(self, dtype: torch.dtype, *, clips: int, frames: int, pixels: int, heads: int, d: int) -> bool:
        """does fyc_temporal_block (the fused temporal sub-block) cover this shape?  (no launch)"""
        if not hasattr(self.lib, "fyc_temporal_block_supported"):
            return False
        a = L.TemporalBlockArgs()
        a.clips, a.frames, a.pixels, a.heads, a.d, a.C = clips, frames, pixels, heads, d, heads * d
        a.dtype = _dtc(dtype)
        return bool(self.lib.fyc_temporal_block_supported(C.byref(a)))

    def temporal_block(self, x: Tensor, out: Tensor, *, w_qkv: Tensor, colsum: Tensor, bias: Tensor, pe_bias: Optional[Tensor],
                       w_out: Tensor, b_out: Tensor, clips: int, frames: int, pixels: int, heads: int, d: int, scale: float,
                       eps: float = 1e-5, wstream: Optional[Tensor] = None) -> None:
        """out = x + Attn_F(LayerNorm(x) + pe) Wo^T + bo in one kernel (csrc/temporal_block.hip); with `wstream`
        (engine/weights.py::pack_temporal_stream) the register-resident kernel (csrc/temporal_block_rr.hip) runs instead"""
        self.ensure_init(x.device)
        a = self._tblock_args(x, out, w_qkv, colsum, bias, pe_bias, w_out, b_out, clips, frames, pixels, heads, d, scale, eps)
        if wstream is not None and hasattr(self.lib, "fyc_temporal_block_wstream_bytes"):
            if "tbw" not in self._q_cache:
                self._q_cache["tbw"] = int(self.lib.fyc_temporal_block_wstream_bytes())
            if wstream.numel() * wstream.element_size() != self._q_cache["tbw"]:
                raise ValueError(f"temporal_block: wstream has {wstream.numel() * wstream.element_size()} bytes, expected {self._q_cache['tbw']}")
            a.wstream = _p(wstream)
        self._call("fyc_temporal_block", a)

    def ff_block_supported(self, dtype: torch.dtype, *, rows: int, C_: int, hidden: int, cs_rows: int = 0) -> bool:
        """does fyc_ff_block (the fused GEGLU feed-forward block) cover this shape?  (no launch); cs_rows > 0: with the fused
        output statistics for a GroupNorm whose statistics sample has cs_rows rows"""
        if not hasattr(self.lib, "fyc_ff_block_supported"):
            return False
        key = ("ffs", dtype, rows, C_, hidden, cs_rows)
        if key in self._q_cache:
            return self._q_cache[key]
        a = L.FFBlockArgs()
        a.rows, a.C, a.hidden, a.cs_rows = rows, C_, hidden, cs_rows
        a.chan_parts = 16 if cs_rows > 0 else None         # only tested for null / alignment by the query
        a.dtype = _dtc(dtype)
        self._q_cache[key] = bool(self.lib.fyc_ff_block_supported(C.byref(a)))
        return self._q_cache[key]

    def ff_block_wstream_bytes(self) -> int:
        if "ffw" not in self._q_cache:
            self._q_cache["ffw"] = int(self.lib.fyc_ff_block_wstream_bytes())
        return self._q_cache["ffw"]

    def ff_block(self, x: Tensor, residual: Optional[Tensor], out: Tensor, *, wstream: Tensor, b_out: Tensor, rows: int, C_: int,
                 hidden: int, eps: float = 1e-5, chan_parts: Optional[Tensor] = None, cs_rows: int = 0) -> None:
        """out = residual + b_out + [x | GEGLU(LN(x) W1^T + b1)] [Wp | Wp W2]^T in one kernel (csrc/ff_block.hip); `wstream`
        from engine/weights.py::pack_ff_block"""
        self.ensure_init(x.device)
        if wstream.numel() * wstream.element_size() != self.ff_block_wstream_bytes():
            raise ValueError(f"ff_block: wstream has {wstream.numel() * wstream.element_size()} bytes, expected {self.ff_block_wstream_bytes()}")
        a = L.FFBlockArgs()
        a.x, a.residual, a.out, a.wstream, a.b_out = _p(x), _p(residual), _p(out), _p(wstream), _f32(b_out, "b_out")
        a.chan_parts, a.cs_rows = _f32(chan_parts, "chan_parts"), cs_rows
        a.rows, a.C, a.hidden, a.eps, a.dtype = rows, C_, hidden, eps, _dt(x)
        self._call("fyc_ff_block", a)

    def panel_linear_supported(self, dtype: torch.dtype, *, rows: int, N: int, K: int, gn_rows_per_sample: int = 0, gn_groups: int = 32) -> bool:
        """does fyc_panel_linear (row-panel linear, optionally with the input's GroupNorm on the operand registers) cover this shape?"""
        if not hasattr(self.lib, "fyc_panel_linear_supported"):
            return False
        key = ("pls", dtype, rows, N, K, gn_rows_per_sample, gn_groups)
        if key not in self._q_cache:
            a = L.PanelLinearArgs()
            a.rows, a.N, a.K = rows, N, K
            a.dtype = _dtc(dtype)
            if gn_rows_per_sample > 0:
                a.gn_cs, a.gn_rows_per_sample, a.gn_stat_samples, a.gn_groups = 16, gn_rows_per_sample, 1, gn_groups     # pointer only tested for null
            self._q_cache[key] = bool(self.lib.fyc_panel_linear_supported(C.byref(a)))
        return self._q_cache[key]

    def panel_linear(self, x: Tensor, out: Tensor, *, wstream: Tensor, rows: int, N: int, K: int, bias: Optional[Tensor] = None,
                     residual: Optional[Tensor] = None, gn_cs: Optional[Tensor] = None, gn_gamma: Optional[Tensor] = None,
                     gn_beta: Optional[Tensor] = None, gn_rows_per_sample: int = 0, gn_stat_samples: int = 1, gn_groups: int = 32,
                     gn_eps: float = 1e-6, gn_parts: Optional[Tensor] = None, gn_tile_rows: int = 0, gn_slots: int = 0) -> None:
        """out = [GroupNorm](x) W^T + bias (+ residual) in one kernel (csrc/panel_linear.hip); `wstream` from
        engine/weights.py::pack_panel_linear; gn_cs = the f64 per-(statistics sample, channel) sums of x, or gn_parts = the row-tile
        partials of x's producer (gn_tile_rows / gn_slots from gemm_stat_layout), folded by the kernel itself"""
        self.ensure_init(x.device)
        key = ("plw", N, K)
        if key not in self._q_cache:
            self._q_cache[key] = int(self.lib.fyc_panel_linear_wstream_bytes(N, K))
        need = self._q_cache[key]
        if wstream.numel() * wstream.element_size() != need:
            raise ValueError(f"panel_linear: wstream has {wstream.numel() * wstream.element_size()} bytes, expected {need}")
        if gn_cs is not None and gn_cs.dtype != torch.float64:
            raise TypeError("panel_linear: gn_cs must be float64")
        a = L.PanelLinearArgs()
        a.x, a.residual, a.out, a.wstream, a.bias = _p(x), _p(residual), _p(out), _p(wstream), _f32(bias, "bias")
        a.gn_cs, a.gn_gamma, a.gn_beta = _p(gn_cs), _f32(gn_gamma, "gn_gamma"), _f32(gn_beta, "gn_beta")
        a.gn_rows_per_sample, a.gn_stat_samples, a.gn_groups, a.gn_eps = gn_rows_per_sample, gn_stat_samples, gn_groups, gn_eps
        a.rows, a.N, a.K, a.dtype = rows, N, K, _dt(x)
        a.gn_parts, a.gn_tile_rows, a.gn_slots = _f32(gn_parts, "gn_parts"), gn_tile_rows, gn_slots
        self._call("fyc_panel_linear", a)

    # -- normalisation -----------------------------------------------------------------------
    def gn_stats(self, x: Tensor, stats: Tensor, *, rows: int, C_: int, groups: int, rows_per_sample: int) -> None:
        a = L.GnStatsArgs()
        if stats.dtype != torch.float64:
            raise TypeError("gn stats buffer must be float64")
        a.x, a.stats, a.rows, a.C, a.groups, a.rows_per_sample, a.dtype = _p(x), _p(stats), rows, C_, groups, rows_per_sample, _dt(x)
        key = ("gnws", rows, groups, rows_per_sample)
        need = self._q_cache.get(key)
        if need is None:
            # (an older A/B library - FYC_LIB_PATH - may predate the entry point: it then reduces without a workspace)
            need = self._q_cache[key] = int(self.lib.fyc_gn_stats_workspace(C.byref(a))) if hasattr(self.lib, "fyc_gn_stats_workspace") else 0
        if need > 0:     # chunk partial sums of the ordered (atomic-free) reduction: the split-K scratch buffer, same stream
            if self._ws is None or self._ws.numel() < need or self._ws.device != x.device:
                self._ws = torch.empty(need, dtype=torch.uint8, device=x.device)
            a.workspace, a.workspace_bytes = self._ws.data_ptr(), self._ws.numel()
        self._call("fyc_gn_stats", a)

    def gn_apply(self, x: Tensor, stats: Tensor, gamma: Tensor, beta: Tensor, y: Tensor, *, rows: int, C_: int,
                 groups: int, rows_per_sample: int, eps: float, silu: bool) -> None:
        a = L.GnApplyArgs()
        a.x, a.stats, a.gamma, a.beta, a.y = _p(x), _p(stats), _f32(gamma, "gamma"), _f32(beta, "beta"), _p(y)
        a.rows, a.C, a.groups, a.rows_per_sample, a.eps, a.silu, a.dtype = rows, C_, groups, rows_per_sample, eps, int(silu), _dt(x)
        self._call("fyc_gn_apply", a)

    direct_stats_supported = True      # gn_apply_cs / panel_linear take the producer's raw partials (parts1 / parts2 / gn_parts)

    def gn_apply_cs(self, x1: Tensor, cs1: Optional[Tensor], gamma: Tensor, beta: Tensor, y: Tensor, *, rows: int, C1: int, groups: int,
                    rows_per_sample: int, eps: float, silu: bool, x2: Optional[Tensor] = None, cs2: Optional[Tensor] = None,
                    C2: int = 0, cs_rows: int = 0, parts1: Optional[Tensor] = None, parts2: Optional[Tensor] = None,
                    tile_rows1: int = 0, slots1: int = 0, tile_rows2: int = 0, slots2: int = 0, parts_cs_rows: int = 0) -> None:
        """per source either the reduced f64 sums (cs) or the producer's row-tile partials (parts + tile_rows / slots from
        gemm_stat_layout, parts_cs_rows rows per statistics sample), which the kernel folds itself"""
        a = L.GnApplyCsArgs()
        for t in (cs1, cs2):
            if t is not None and t.dtype != torch.float64:
                raise TypeError("channel statistics must be float64")
        a.x1, a.cs1, a.x2, a.cs2 = _p(x1), _p(cs1), _p(x2), _p(cs2)
        a.gamma, a.beta, a.y = _f32(gamma, "gamma"), _f32(beta, "beta"), _p(y)
        a.C1, a.C2, a.rows, a.groups, a.rows_per_sample, a.eps, a.silu, a.dtype = C1, C2, rows, groups, rows_per_sample, eps, int(silu), _dt(x1)
        a.cs_rows = cs_rows
        a.parts1, a.parts2 = _f32(parts1, "parts1"), _f32(parts2, "parts2")
        a.tile_rows1, a.slots1, a.tile_rows2, a.slots2, a.parts_cs_rows = tile_rows1, slots1, tile_rows2, slots2, parts_cs_rows
        self._call("fyc_gn_apply_cs", a)

    def layernorm(self, x: Tensor, gamma: Tensor, beta: Tensor, y: Tensor, *, rows: int, C_: int, eps: float = 1e-5,
                  pe: Optional[Tensor] = None, pe_div: int = 1, pe_rows: int = 1) -> None:
        a = L.LayerNormArgs()
        a.x, a.gamma, a.beta, a.pe, a.y = _p(x), _f32(gamma, "gamma"), _f32(beta, "beta"), _f32(pe, "pe"), _p(y)
        a.rows, a.C, a.eps, a.pe_div, a.pe_rows, a.dtype = rows, C_, eps, pe_div, pe_rows, _dt(x)
        self._call("fyc_layernorm", a)

    def row_stats(self, x: Tensor, stats: Tensor, *, rows: int, C_: int, eps: float = 1e-5) -> None:
        a = L.RowStatsArgs()
        a.x, a.stats, a.rows, a.C, a.eps, a.dtype = _p(x), _f32(stats, "stats"), rows, C_, eps, _dt(x)
        self._call("fyc_row_stats", a)

    def softmax_rows(self, x: Tensor, *, rows: int, cols: int, ld: int, causal_rows: int = 0) -> None:
        a = L.SoftmaxArgs()
        a.x, a.rows, a.cols, a.ld, a.dtype, a.causal_rows = _p(x), rows, cols, ld, _dt(x), causal_rows
        self._call("fyc_softmax_rows", a)

    # -- elementwise / layout ------------------------------------------------------------------
    def concat_channels(self, a_: Tensor, b_: Tensor, y: Tensor, *, rows: int, c1: int, c2: int) -> None:
        a = L.ConcatArgs()
        a.a, a.b, a.y, a.rows, a.c1, a.c2, a.dtype = _p(a_), _p(b_), _p(y), rows, c1, c2, _dt(a_)
        self._call("fyc_concat_channels", a)

    def embed_tokens(self, ids: Tensor, table: Tensor, pos: Tensor, out: Tensor, *, rows: int, seq: int, C_: int) -> None:
        if ids.dtype != torch.int64 or table.dtype != torch.float32 or pos.dtype != torch.float32:
            raise TypeError("embed_tokens: ids must be int64, tables float32")
        a = L.EmbedArgs()
        a.ids, a.table, a.pos, a.out = _p(ids), _p(table), _p(pos), _p(out)
        a.rows, a.seq, a.C, a.vocab, a.dtype = rows, seq, C_, table.shape[0], _dt(out)
        self._call("fyc_embed_tokens", a)

    def patchify(self, image: Tensor, out: Tensor, *, B: int, Cin: int, H: int, W: int, P: int, ld: int) -> None:
        if image.dtype != torch.float32:
            raise TypeError("patchify: image must be float32 NCHW")
        a = L.PatchifyArgs()
        a.image, a.out, a.B, a.Cin, a.H, a.W, a.P, a.ld, a.dtype = _p(image), _p(out), B, Cin, H, W, P, ld, _dt(out)
        self._call("fyc_patchify", a)

    def pack_conv3x3(self, w: Tensor, out: Tensor) -> None:
        """(O, I, 3, 3) f32 on the device -> the K order of the implicit-GEMM conv (engine/weights.py::pack_conv3x3)"""
        a = L.PackConv3x3Args()
        a.w, a.out, a.O, a.I, a.dtype = _f32(w, "w"), _p(out), w.shape[0], w.shape[1], _dt(out)
        self._call("fyc_pack_conv3x3", a)

    def pack_geglu(self, w: Tensor, b: Optional[Tensor], w_out: Tensor, b_out: Optional[Tensor]) -> None:
        """ff.net.0.proj rows -> 16 value rows, their 16 gate rows, ... (engine/weights.py::pack_geglu)"""
        a = L.PackGegluArgs()
        a.w, a.b, a.w_out, a.b_out = _f32(w, "w"), _f32(b, "b"), _p(w_out), _f32(b_out, "b_out")
        a.O, a.I, a.dtype = w.shape[0], w.shape[1], _dt(w_out)
        self._call("fyc_pack_geglu", a)

    def silu_f32(self, x: Tensor, y: Tensor) -> None:
        a = L.SiluArgs()
        a.x, a.y, a.n = _f32(x, "x"), _f32(y, "y"), x.numel()
        self._call("fyc_silu_f32", a)

    def cast_from_f32(self, x: Tensor, y: Tensor, *, rows: int, cols: int, ld: int) -> None:
        a = L.CastArgs()
        a.x, a.y, a.rows, a.cols, a.ld, a.dtype = _f32(x, "x"), _p(y), rows, cols, ld, _dt(y)
        self._call("fyc_cast_from_f32", a)

    def cast_to_f32(self, x: Tensor, y: Tensor, *, rows: int, cols: int, ld: int) -> None:
        a = L.CastArgs()
        a.x, a.y, a.rows, a.cols, a.ld, a.dtype = _p(x), _f32(y, "y"), rows, cols, ld, _dt(x)
        self._call("fyc_cast_to_f32", a)

    def unet_input(self, latents: Tensor, mask: Optional[Tensor], first: Optional[Tensor], x: Tensor, *, B: int, F: int,
                   HW: int, c_latent: int, c_pad: int, cfg_dup: int, mask_frames: int = 1, mode: int = 0) -> None:
        self.ensure_init(latents.device)
        a = L.UnetInputArgs()
        a.latents, a.mask, a.first, a.x = _f32(latents, "latents"), _f32(mask, "mask"), _f32(first, "first"), _p(x)
        a.B, a.F, a.HW, a.c_latent, a.c_pad, a.cfg_dup, a.mask_frames, a.dtype, a.mode = B, F, HW, c_latent, c_pad, cfg_dup, mask_frames, _dt(x), mode
        self._call("fyc_unet_input", a)

    def cfg_ddim_step(self, pred: Tensor, latents: Tensor, coef: Tensor, *, B: int, F: int, HW: int, c_latent: int,
                      ld: int, cfg: bool, guidance: float, pred_type: int, clip_sample: bool,
                      pred_single: Optional[Tensor] = None, video_scale: float = 0.0, variance_noise: Optional[Tensor] = None,
                      sigma: float = 0.0, clipped_model_output: bool = False) -> None:
        a = L.CfgDdimArgs()
        self._fill_cfg_ddim(a, pred, latents, coef, B, F, HW, c_latent, ld, cfg, guidance, pred_type, clip_sample, pred_single, video_scale,
                            variance_noise, sigma, clipped_model_output)
        self._call("fyc_cfg_ddim_step", a)

    @staticmethod
    def _fill_cfg_common(a, pred, latents, coef, B, F, HW, c_latent, ld, cfg, guidance, pred_single, video_scale, who, shaped=()) -> None:
        """the fields every cfg step's arguments start with; `shaped`: (name, tensor or None) pairs that must have the latents' size"""
        for name, t in shaped:
            if t is not None and t.numel() != latents.numel():
                raise ValueError(f"{who}: {name} must have the latents' shape")
        if pred_single is not None and pred_single.dtype != pred.dtype:
            raise TypeError(f"{who}: pred_single dtype differs from pred")
        a.pred, a.latents, a.coef = _p(pred), _f32(latents, "latents"), _f32(coef, "coef")
        a.B, a.F, a.HW, a.c_latent, a.ld, a.cfg, a.guidance, a.dtype = B, F, HW, c_latent, ld, int(cfg), guidance, _dt(pred)
        a.pred_single, a.video_scale = _p(pred_single), video_scale

    def _rescale_workspace(self, key, query: str, args, device: torch.device) -> None:
        """args.workspace / .workspace_bytes <- the moments workspace of the guidance rescale, if `query` (asked once per key) wants one: this
        object's one buffer (a fixed address under a captured graph), grown on demand"""
        need = self._ws_need.get(key)
        if need is None:
            need = self._ws_need[key] = int(getattr(self.lib, query)(C.byref(args)))
        if need > 0:
            if self._rescale_ws is None or self._rescale_ws.numel() < need or self._rescale_ws.device != device:
                self._rescale_ws = torch.empty(need, dtype=torch.uint8, device=device)
            args.workspace, args.workspace_bytes = self._rescale_ws.data_ptr(), self._rescale_ws.numel()

    @staticmethod
    def _fill_cfg_ddim(a, pred, latents, coef, B, F, HW, c_latent, ld, cfg, guidance, pred_type, clip_sample, pred_single, video_scale,
                       variance_noise, sigma, clipped_model_output) -> None:
        HipOps._fill_cfg_common(a, pred, latents, coef, B, F, HW, c_latent, ld, cfg, guidance, pred_single, video_scale, "cfg_ddim_step",
                                [("variance_noise", variance_noise)])
        a.variance_noise, a.sigma, a.clipped_model_output = _f32(variance_noise, "variance_noise"), float(sigma), int(clipped_model_output)
        a.pred_type, a.clip_sample = pred_type, int(clip_sample)

    def cfg_ddim_step_rescaled(self, pred: Tensor, latents: Tensor, coef: Tensor, *, guidance_rescale: float, B: int, F: int, HW: int,
                               c_latent: int, ld: int, cfg: bool, guidance: float, pred_type: int, clip_sample: bool,
                               pred_single: Optional[Tensor] = None, video_scale: float = 0.0, variance_noise: Optional[Tensor] = None,
                               sigma: float = 0.0, clipped_model_output: bool = False) -> None:
        """cfg_ddim_step with the guided prediction of every sample rescaled towards the standard deviation of its conditional prediction
        (include/fyc.h, fyc_cfg_ddim_step_rescaled; guidance_rescale = 0 is cfg_ddim_step).  The moments workspace is this object's: sized by the
        library's query per shape, one buffer kept (a fixed address under a captured graph) and grown on demand."""
        self.ensure_init(pred.device)
        r = L.CfgDdimRescaleArgs()
        self._fill_cfg_ddim(r.step, pred, latents, coef, B, F, HW, c_latent, ld, cfg, guidance, pred_type, clip_sample, pred_single,
                            video_scale, variance_noise, sigma, clipped_model_output)
        r.guidance_rescale = float(guidance_rescale)
        self._rescale_workspace(("cfg_rescale", B, F, HW, c_latent, ld, r.guidance_rescale > 0, bool(cfg)), "fyc_cfg_ddim_rescale_workspace_bytes", r,
                                pred.device)
        self._call("fyc_cfg_ddim_step_rescaled", r)

    def cfg_solver_step(self, pred: Tensor, latents: Tensor, coef: Tensor, *, hist_out: Tensor, hist_1: Optional[Tensor] = None,
                        hist_2: Optional[Tensor] = None, order: int, B: int, F: int, HW: int, c_latent: int, ld: int, cfg: bool,
                        guidance: float, pred_single: Optional[Tensor] = None, video_scale: float = 0.0,
                        guidance_rescale: float = 0.0) -> None:
        """guidance + one DPM-Solver multistep update (include/fyc.h, fyc_cfg_solver_step): coef f32[8] = {a_x, a_v, c_x, c_0, c_1, c_2, -, -};
        latents are updated in place, hist_out receives this step's converted output, hist_1 / hist_2 hold those of the two steps before
        (read only at order >= 2 / 3).  The moments workspace of the guidance rescale is the one cfg_ddim_step_rescaled keeps."""
        self.ensure_init(pred.device)
        if coef.numel() < 8:
            raise ValueError(f"cfg_solver_step: coef holds {coef.numel()} values, the kernel's table row has 8")
        a = L.CfgSolverArgs()
        self._fill_cfg_common(a, pred, latents, coef, B, F, HW, c_latent, ld, cfg, guidance, pred_single, video_scale, "cfg_solver_step",
                              [("hist_out", hist_out), ("hist_1", hist_1), ("hist_2", hist_2)])
        a.hist_out, a.hist_1, a.hist_2, a.order = _f32(hist_out, "hist_out"), _f32(hist_1, "hist_1"), _f32(hist_2, "hist_2"), int(order)
        a.guidance_rescale = float(guidance_rescale)
        self._rescale_workspace(("cfg_solver", B, F, HW, c_latent, ld, a.guidance_rescale > 0, bool(cfg)), "fyc_cfg_solver_workspace_bytes", a, pred.device)
        self._call("fyc_cfg_solver_step", a)

    def cfg_sigma_step(self, pred: Tensor, latents: Tensor, coef: Tensor, *, hist_out: Optional[Tensor] = None, hist_1: Optional[Tensor] = None,
                       hist_2: Optional[Tensor] = None, hist_3: Optional[Tensor] = None, order: int = 1, noise: Optional[Tensor] = None,
                       B: int, F: int, HW: int, c_latent: int, ld: int, cfg: bool, guidance: float, pred_single: Optional[Tensor] = None,
                       video_scale: float = 0.0, guidance_rescale: float = 0.0) -> None:
        """guidance + one Euler / Euler-ancestral / LMS update (include/fyc.h, fyc_cfg_sigma_step): coef f32[8] = {a_x, a_v, c_x, c_0, c_1, c_2,
        c_3, c_n}; latents are updated in place, hist_out (None = not stored) receives this step's derivative, hist_k holds that of k steps ago
        (read only at order > k), noise (None = none) is the ancestral step's.  The moments workspace of the guidance rescale is the one
        cfg_ddim_step_rescaled keeps."""
        self.ensure_init(pred.device)
        if coef.numel() < 8:
            raise ValueError(f"cfg_sigma_step: coef holds {coef.numel()} values, the kernel's table row has 8")
        a = L.CfgSigmaArgs()
        self._fill_cfg_common(a, pred, latents, coef, B, F, HW, c_latent, ld, cfg, guidance, pred_single, video_scale, "cfg_sigma_step",
                              [("hist_out", hist_out), ("hist_1", hist_1), ("hist_2", hist_2), ("hist_3", hist_3), ("noise", noise)])
        a.hist_out, a.hist_1, a.hist_2, a.hist_3 = _f32(hist_out, "hist_out"), _f32(hist_1, "hist_1"), _f32(hist_2, "hist_2"), _f32(hist_3, "hist_3")
        a.order, a.noise = int(order), _f32(noise, "noise")
        a.guidance_rescale = float(guidance_rescale)
        self._rescale_workspace(("cfg_sigma", B, F, HW, c_latent, ld, a.guidance_rescale > 0, bool(cfg)), "fyc_cfg_sigma_workspace_bytes", a, pred.device)
        self._call("fyc_cfg_sigma_step", a)

    def cfg_pndm_step(self, pred: Tensor, latents: Tensor, coef: Tensor, *, sample_in: Optional[Tensor] = None, sample_out: Optional[Tensor] = None,
                      hist_out: Optional[Tensor] = None, hist_1: Optional[Tensor] = None, hist_2: Optional[Tensor] = None,
                      hist_3: Optional[Tensor] = None, order: int = 1, acc_in: Optional[Tensor] = None, acc_out: Optional[Tensor] = None,
                      B: int, F: int, HW: int, c_latent: int, ld: int, cfg: bool, guidance: float, pred_single: Optional[Tensor] = None,
                      video_scale: float = 0.0, guidance_rescale: float = 0.0) -> None:
        """guidance + one PNDM evaluation, PLMS or Runge-Kutta mode (include/fyc.h, fyc_cfg_pndm_step): coef f32[6] = {c_x, c_0, c_1, c_2, c_3,
        s_g}; latents are updated in place from sample_in (None = from themselves); sample_out (None = not stored) receives the latents as they
        were, hist_out the guided prediction, acc_out = acc_in + s_g g (acc_in None = 0; acc_in may be acc_out); hist_k is the stored prediction
        k places back (read only at order > k).  The moments workspace of the guidance rescale is the one cfg_ddim_step_rescaled keeps."""
        self.ensure_init(pred.device)
        if coef.numel() < 6:
            raise ValueError(f"cfg_pndm_step: coef holds {coef.numel()} values, the kernel's table row has 6")
        a = L.CfgPndmArgs()
        self._fill_cfg_common(a, pred, latents, coef, B, F, HW, c_latent, ld, cfg, guidance, pred_single, video_scale, "cfg_pndm_step",
                              [("sample_in", sample_in), ("sample_out", sample_out), ("hist_out", hist_out), ("hist_1", hist_1), ("hist_2", hist_2),
                               ("hist_3", hist_3), ("acc_in", acc_in), ("acc_out", acc_out)])
        a.sample_in, a.sample_out = _f32(sample_in, "sample_in"), _f32(sample_out, "sample_out")
        a.hist_out, a.hist_1, a.hist_2, a.hist_3 = _f32(hist_out, "hist_out"), _f32(hist_1, "hist_1"), _f32(hist_2, "hist_2"), _f32(hist_3, "hist_3")
        a.order, a.acc_in, a.acc_out = int(order), _f32(acc_in, "acc_in"), _f32(acc_out, "acc_out")
        a.guidance_rescale = float(guidance_rescale)
        self._rescale_workspace(("cfg_pndm", B, F, HW, c_latent, ld, a.guidance_rescale > 0, bool(cfg)), "fyc_cfg_pndm_workspace_bytes", a, pred.device)
        self._call("fyc_cfg_pndm_step", a)

    def unet_input_scaled(self, latents: Tensor, mask: Optional[Tensor], first: Optional[Tensor], x: Tensor, *, denom: float, scale_cond: bool,
                          B: int, F: int, HW: int, c_latent: int, c_pad: int, cfg_dup: int, mask_frames: int = 1, mode: int = 0) -> None:
        """unet_input with every stored value divided by denom = sqrt(sigma^2 + 1) (include/fyc.h, fyc_unet_input_scaled); scale_cond: the mask
        channel and the first-frame block of mode 0 are divided too"""
        self.ensure_init(latents.device)
        s = L.UnetInputScaledArgs()
        a = s.base
        a.latents, a.mask, a.first, a.x = _f32(latents, "latents"), _f32(mask, "mask"), _f32(first, "first"), _p(x)
        a.B, a.F, a.HW, a.c_latent, a.c_pad, a.cfg_dup, a.mask_frames, a.dtype, a.mode = B, F, HW, c_latent, c_pad, cfg_dup, mask_frames, _dt(x), mode
        s.denom, s.scale_cond = float(denom), int(scale_cond)
        self._call("fyc_unet_input_scaled", s)

    @staticmethod
    def _contiguous(what: str, *tensors) -> None:
        if any(t is not None and not t.is_contiguous() for t in tensors):
            raise ValueError(f"{what}: every tensor must be contiguous")

    def posterior_latents(self, moments: Tensor, latents: Tensor, *, noise_post: Optional[Tensor] = None, noise_add: Optional[Tensor] = None,
                          clean_out: Optional[Tensor] = None, scale: float, c_x: float = 1.0, c_n: float = 0.0) -> None:
        """VAE moments (N, 2C, h, w) f32 -> noised start latents (N, C, h, w) f32 (include/fyc.h, fyc_posterior_latents): z = (mean + std *
        noise_post) * scale (noise_post None: the mode, mean * scale), clean_out = z (None = not stored), latents = c_x z + c_n noise_add
        (noise_add None: c_x z)"""
        self.ensure_init(moments.device)
        N, C2, H, W = moments.shape
        if C2 % 2 or tuple(latents.shape) != (N, C2 // 2, H, W):
            raise ValueError(f"posterior_latents: moments {tuple(moments.shape)} do not give latents {tuple(latents.shape)}")
        for name, t in (("noise_post", noise_post), ("noise_add", noise_add), ("clean_out", clean_out)):
            if t is not None and tuple(t.shape) != tuple(latents.shape):
                raise ValueError(f"posterior_latents: {name} must have the latents' shape")
        self._contiguous("posterior_latents", moments, latents, noise_post, noise_add, clean_out)
        a = L.PosteriorLatentsArgs()
        a.moments, a.noise_post, a.noise_add = _f32(moments, "moments"), _f32(noise_post, "noise_post"), _f32(noise_add, "noise_add")
        a.latents, a.clean_out = _f32(latents, "latents"), _f32(clean_out, "clean_out")
        a.N, a.C, a.HW, a.scale, a.c_x, a.c_n = N, C2 // 2, H * W, float(scale), float(c_x), float(c_n)
        self._call("fyc_posterior_latents", a)

    def inpaint_prepare(self, image: Optional[Tensor], mask: Tensor, *, masked: Optional[Tensor] = None, mask_latent: Optional[Tensor] = None) -> None:
        """image (N, 3, H, W) f32 in [-1, 1], mask (N, 1, H, W) f32 in [0, 1] -> masked (N, 3, H, W) = image * (mask < 0.5), mask_latent
        (N, 1, H/8, W/8) = the binarised mask at pixel (8i, 8j) (include/fyc.h, fyc_inpaint_prepare); an output left None is not stored"""
        self.ensure_init(mask.device)
        N, one, H, W = mask.shape
        if one != 1 or H % 8 or W % 8:
            raise ValueError(f"inpaint_prepare: mask {tuple(mask.shape)} must be (N, 1, H, W) with H and W multiples of 8")
        if masked is not None and (image is None or tuple(image.shape) != (N, 3, H, W) or tuple(masked.shape) != (N, 3, H, W)):
            raise ValueError(f"inpaint_prepare: image and masked must be ({N}, 3, {H}, {W})")
        if mask_latent is not None and tuple(mask_latent.shape) != (N, 1, H // 8, W // 8):
            raise ValueError(f"inpaint_prepare: mask_latent must be ({N}, 1, {H // 8}, {W // 8})")
        self._contiguous("inpaint_prepare", image, mask, masked, mask_latent)
        a = L.InpaintPrepareArgs()
        a.image, a.mask, a.masked, a.mask_latent = _f32(image, "image"), _f32(mask, "mask"), _f32(masked, "masked"), _f32(mask_latent, "mask_latent")
        a.N, a.H, a.W = N, H, W
        self._call("fyc_inpaint_prepare", a)

    def renoise_blend(self, latents: Tensor, orig: Tensor, noise: Tensor, mask: Tensor, *, c_x: float, c_n: float, B: int, C_: int, F: int,
                      HW: int) -> None:
        """latents (B, C, F, HW) f32 in place = (c_x orig + c_n noise) * mask + latents * (1 - mask) (include/fyc.h, fyc_renoise_blend); mask
        (B, 1, HW); orig and noise (B, C, HW) - broadcast over the frames - or the latents' shape"""
        self.ensure_init(latents.device)
        n = B * C_ * F * HW
        if latents.numel() != n or mask.numel() != B * HW or orig.numel() != noise.numel() or orig.numel() not in (n, n // F):
            raise ValueError(f"renoise_blend: latents {tuple(latents.shape)}, orig {tuple(orig.shape)}, noise {tuple(noise.shape)}, mask "
                             f"{tuple(mask.shape)} do not fit B = {B}, C = {C_}, F = {F}, HW = {HW}")
        self._contiguous("renoise_blend", latents, orig, noise, mask)
        a = L.RenoiseBlendArgs()
        a.latents, a.orig, a.noise, a.mask = _f32(latents, "latents"), _f32(orig, "orig"), _f32(noise, "noise"), _f32(mask, "mask")
        a.B, a.C, a.F, a.HW, a.src_frames, a.c_x, a.c_n = B, C_, F, HW, (F if orig.numel() == n else 1), float(c_x), float(c_n)
        self._call("fyc_renoise_blend", a)

    def nchw_to_nhwc(self, z: Tensor, x: Tensor, *, N: int, C_: int, HW: int, c_pad: int, scale: float) -> None:
        self.ensure_init(z.device)
        a = L.NchwInArgs()
        a.z, a.x, a.N, a.C, a.HW, a.c_pad, a.scale, a.dtype = _f32(z, "z"), _p(x), N, C_, HW, c_pad, scale, _dt(x)
        self._call("fyc_nchw_to_nhwc", a)

    def nhwc_to_nchw(self, x: Tensor, y: Tensor, *, N: int, C_: int, HW: int, ld: int, mul: float = 1.0, add: float = 0.0,
                     lo: float = -3.0e38, hi: float = 3.0e38) -> None:
        a = L.NhwcOutArgs()
        a.x, a.y, a.N, a.C, a.HW, a.ld, a.mul, a.add, a.lo, a.hi, a.dtype = _p(x), _f32(y, "y"), N, C_, HW, ld, mul, add, lo, hi, _dt(x)
        self._call("fyc_nhwc_to_nchw", a)


impl = None  # type: Optional[HipOps]


def get() -> HipOps:
    """The active backend; created on first use.  Raises if libfyc_hip.so is missing."""
    global impl
    if impl is None:
        impl = HipOps()
    return impl
