"""fyc_attention's causal mask and head dims up to 512 (ABI 308), without a GPU: the two rules as specified against the bounds the GPU cases are judged by
(tests/attn_wide_spec.py), the reach of the case list, the discriminating causal operands, the refusals of the built library, the Python surface, and the engines'
choice between one fused launch and the materialised sequence - on the new emulator (tests/emu_ops_wide.py) and, unchanged, on plain EmuOps."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import attention_cases as A
import attn_wide_spec as WS
import kernel_compare as KC
from emu_ops import EmuOps
from emu_ops_wide import WideEmuOps
from followyourclick_amd.engine import base as EB
from followyourclick_amd.engine import encoders as EN
from followyourclick_amd.engine import vae as EV
from followyourclick_amd.engine.weights import Packed
from kernel_compare import Guard, compare
from oracle import encoders as E


@pytest.mark.parametrize("lag", [0.0, 5.7])
@pytest.mark.parametrize("case", WS.CASES, ids=WS.case_ids(WS.CASES))
def test_spec_inside_the_bound(case, lag):
    """the rule of the case's dtype family, with the true row maximum and with one that lags it by 5.7 log2 units, against f64 attention of the unrounded operands over
    the visible keys: every element inside the bound, global rel-L2 inside the tolerance, nothing outside the output written"""
    c, f = case, case.f
    ops, ref, bound = WS.reference(c)
    got = WS.emulate(c, ops, lag=lag)
    compare(A.window(f, got), A.window(f, ref), dtype=f.dt, bound=bound, rtol=f.rtol, labels=WS.labels(c), guard=Guard(ops.buf, got, ops.mask), tag=c.name)


DISC = [c for c in WS.CASES if c.recipe == "discriminating"]


@pytest.mark.parametrize("case", DISC, ids=WS.case_ids(DISC))
def test_discriminating_operands_tell_a_missing_mask(case):
    """every removed score exceeds every kept one of its row by >= 40 log2 units; the masked f64 reference is finite and the unmasked one is more than 0.5 rel-L2 away;
    a rule that lets the removed keys into the maximum (and only there) leaves the bound or is not finite - from 8 queries on, where the last key leads the first by 280
    log2 units and p underflows (with two keys p = 2^-40 is a number, and the normalisation hides the wrong maximum)"""
    c, f = case, case.f
    ops, ref, bound = WS.reference(c)
    r = A.window(f, ref).double()
    assert torch.isfinite(r).all()
    if f.n_q == 1:
        return                                  # one query sees its only key: nothing is removed
    assert WS.check_discriminating(c, ops) >= WS.GAP
    un = WS.unmasked_reference(c, ops)
    prev = A.window(f, ops.buf).double() if f.accumulate else 0.0
    assert ((prev + f.o_scale * un - r).norm() / r.norm()).item() > 0.5
    if f.n_q < 8:
        return
    got = A.window(f, WS.emulate(c, ops, defect="mask_after_max")).double()
    over = torch.nan_to_num((got - r).abs() / bound, nan=float("inf"))
    assert over.max().item() > 1.0


def test_case_list_reaches_every_instantiation():
    t = {c.name: WS.traits(c) for c in WS.CASES}
    assert {x["instance"] for x in t.values()} == WS.built()
    wide = [c for c in WS.CASES if c.f.d > 160]
    for dt in WS.DTS:
        mine = [c for c in wide if c.f.dt == dt and not c.causal]
        assert {c.f.d for c in mine} == set(WS.WIDE_D)                                              # 1.5 / 2 / 2.5 / 4 chunks of 128
        assert {t[c.name]["chunks"] for c in mine} == {1.5, 2.0, 2.5, 4.0}
        assert {(c.f.n_q, c.f.n_k) for c in mine} >= set(WS.WIDE_SHAPES) and {(c.f.B, c.f.H) for c in mine} >= set(WS.WIDE_BH)
        assert {t[c.name]["ragged_tile"] for c in mine} == {True, False}                           # 32, 64 keys: full tiles; 1, 31, 33, 65, 81: ragged
        assert {t[c.name]["tiles"] for c in mine} >= {1, 2, 3, 5}                                   # one, two and several ring stages of key tiles
        assert {min(t[c.name]["units"], WS.NS) for c in mine} == {WS.NS} and min(t[c.name]["units"] for c in mine) >= WS.NS - 1
        assert {(t[c.name]["query_blocks"] > 1, t[c.name]["ragged_queries"]) for c in mine} >= {(False, True), (True, True), (False, False)}
        assert any(c.f.accumulate and c.f.o_scale != 1.0 for c in mine) and any(c.f.div == 2 for c in mine) and any(c.f.ldvt - c.f.n_k >= 8 for c in mine)
        assert {t[c.name]["xcd"] for c in mine} == {True, False}
        cz = [c for c in WS.CASES if c.f.dt == dt and c.causal]
        assert {c.f.d for c in cz} == set(WS.CAUSAL_D) | {320} and {c.f.n_q for c in cz} >= set(WS.CAUSAL_N)
        assert {c.recipe for c in cz} == {"random", "discriminating"}
        assert any(t[c.name]["skipped_tiles"] > 0 and t[c.name]["query_blocks"] > 1 for c in cz)   # a first query block that leaves key tiles out, a later one that does not
        assert any(t[c.name]["units"] == 2 for c in cz)                                             # fewer units than ring stages (d <= 128, one tile)
    # pad keys: finite, and as large as the type (16-bit) or its bf16 split (tier) allows
    c = next(c for c in wide if c.f.ldvt - c.f.n_k >= 8 and c.f.dt == "bf16")
    pad = WS.operands(c).vt[..., c.f.n_k:]
    assert torch.isfinite(pad.float()).all() and pad.float().abs().min().item() == torch.finfo(torch.bfloat16).max


# ---- the library's refusals, no device --------------------------------------------------------------------------------------------------------------
def _lib():
    from followyourclick_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib, _lib.load()


BAD = [(dict(causal=2), b"causal"), (dict(causal=-1), b"causal"), (dict(causal=1, n_k=32, ldvt=32), b"causal"), (dict(causal=1, q_batch_mod=1), b"causal"),
       (dict(d=168, ldo=168), b"d=168"), (dict(d=200, ldo=200), b"d=200"), (dict(d=520, ldo=520), b"d=520"), (dict(d=544, ldo=544), b"d=544")]


def _args(L, fields, dtype=1, products=0):
    """fyc_attn_mask_args around a valid 64 x 64 x 64 problem with `fields` written over it (`causal` into the outer struct, the rest into .attn)"""
    m = L.AttnMaskArgs()
    a = m.attn
    a.q, a.k, a.vt, a.o = 0x10000000, 0x20000000, 0x30000000, 0x40000000
    a.batch, a.heads, a.n_q, a.n_k, a.d, a.ldo, a.ldvt, a.kv_batch_div, a.scale, a.o_scale = 2, 1, 64, 64, 64, 64, 64, 1, 1.0, 1.0
    a.dtype, a.f32_products = dtype, products
    for k, v in fields.items():
        setattr(m if k == "causal" else a, k, v)
    return m


@pytest.mark.parametrize("dtype,products", [(1, 0), (2, 0), (0, 1)])
@pytest.mark.parametrize("fields,word", BAD, ids=[",".join(f"{k}={v}" for k, v in b[0].items()) for b in BAD])
def test_bad_arguments_are_refused_by_the_library_without_gpu(fields, word, dtype, products):
    """causal other than 0 / 1, causal = 1 with n_q != n_k or q_batch_mod > 0, d > 160 that is no multiple of 32, d > 512: refused before anything that needs a device
    or fyc_init (this process never calls fyc_init: a check behind it would report that instead), the message names the field.  The head-dim cases are refused by
    fyc_attention itself as well"""
    L, lib = _lib()
    m = _args(L, fields, dtype, products)
    assert lib.fyc_attention_masked(ctypes.byref(m), None) != 0
    msg = lib.fyc_last_error()
    assert word in msg and b"fyc_init" not in msg, msg
    if "causal" not in fields:
        assert lib.fyc_attention(ctypes.byref(m.attn), None) != 0
        msg = lib.fyc_last_error()
        assert word in msg and b"fyc_init" not in msg, msg


def test_good_arguments_reach_the_init_check():
    """the same struct with causal = 1 / d = 512 passes every argument check: what stops it here is the missing fyc_init, nothing earlier"""
    L, lib = _lib()
    for fields in (dict(causal=1), dict(d=512, ldo=512), dict(causal=1, d=512, ldo=512), dict(d=192, ldo=192), dict()):
        m = _args(L, fields)
        assert lib.fyc_attention_masked(ctypes.byref(m), None) != 0
        assert b"fyc_init" in lib.fyc_last_error()
    assert lib.fyc_attention_masked(None, None) != 0 and b"null" in lib.fyc_last_error()


def test_mask_struct_layout_matches_c(tmp_path):
    """fyc_attn_mask_args = the attention's arguments as ABI 307 left them, then `causal` (tests/test_abi.py's check, for the struct its table does not list)"""
    import subprocess
    from followyourclick_amd import _lib as L
    header = os.path.join(os.path.dirname(L.HERE), "include", "fyc.h")
    src = tmp_path / "abi.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{header}"\nint main(void){{printf("%zu %zu %zu %zu\\n", sizeof(fyc_attn_mask_args), '
                   'offsetof(fyc_attn_mask_args, attn), offsetof(fyc_attn_mask_args, causal), sizeof(fyc_attn_args));return 0;}')
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    size, off_attn, off_causal, inner = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert (size, off_attn, off_causal, inner) == (ctypes.sizeof(L.AttnMaskArgs), L.AttnMaskArgs.attn.offset, L.AttnMaskArgs.causal.offset, ctypes.sizeof(L.AttnArgs))


def test_binding_and_python_surface():
    from followyourclick_amd import _lib as L, ops
    assert [n for n, _ in L.AttnMaskArgs._fields_] == ["attn", "causal"] and L.AttnArgs._fields_[-1][0] == "f32_products" and L.FYC_VERSION == 308
    assert L.OPS["fyc_attention_masked"] is L.AttnMaskArgs
    with open(os.path.join(os.path.dirname(L.HERE), "include", "fyc.h")) as fh:
        head = fh.read()
    assert "#define FYC_VERSION 308" in head and "typedef struct { fyc_attn_args attn; int32_t causal; } fyc_attn_mask_args;" in head
    sig = inspect.signature(ops.HipOps.attention)
    assert sig.parameters["causal"].default is False and sig.parameters["causal"].kind is inspect.Parameter.KEYWORD_ONLY
    assert callable(ops.HipOps.attention_causal_supported) and callable(ops.HipOps.attention_max_head_dim)


# ---- the engines ---------------------------------------------------------------------------------------------------------------------------------------
class Counting:
    """counts the launches of an ops object by name, forwarding everything"""

    def __init__(self, inner):
        self.inner, self.count, self.order = inner, {}, []

    def __getattr__(self, name):
        v = getattr(self.inner, name)      # (AttributeError for a query the inner object does not answer: getattr(ops, name, None) stays None)
        if not callable(v) or name.startswith("attention_") or name in ("ensure_init",):
            return v

        def call(*a, **kw):
            self.count[name] = self.count.get(name, 0) + 1
            self.order.append(name)
            return v(*a, **kw)
        return call


def _load(golden_dir, name):
    return {k: torch.from_numpy(v) if v.shape and v.dtype.kind in "fi" else v for k, v in np.load(os.path.join(golden_dir, name)).items()}


def _cfg(cls, ocfg):
    return cls(**vars(ocfg))


def rel(a, b):
    return ((a - b).norm() / b.norm()).item()


def _ops(dtype, fused):
    """the new emulator (f32: split products, the precondition of the fused launch) or plain EmuOps"""
    return Counting(WideEmuOps(acc=torch.float32, f32_products="split") if fused else EmuOps())


def _expect(ops, fused, launches):
    if fused:
        assert ops.count.get("attention", 0) == launches and "softmax_rows" not in ops.count, ops.count
    else:      # the parent's sequence: every softmax_rows sits between its score GEMM and its P V GEMM, and no fused launch anywhere
        assert "attention" not in ops.count and ops.count.get("softmax_rows", 0) > 0, ops.count
        at = [i for i, n in enumerate(ops.order) if n == "softmax_rows"]
        assert all(ops.order[i - 1] == "gemm" and ops.order[i + 1] == "gemm" for i in at), ops.order


# (f32 on the new emulator runs the split rule in the attention and f32 GEMMs around it: the existing GPU tolerance of the f32 parametrisation, 2e-5, not the emulator's 1e-5)
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "plain-emu"])
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 3e-2)])
def test_clip_text_engine(golden_dir, monkeypatch, dtype, tol, fused):
    monkeypatch.delenv("FYC_SIDE_FLASH", raising=False)
    g = _load(golden_dir, "enc_clip_text.npz")
    sd = E.make_encoder_weights(E.clip_text_shapes(E.TINY_TEXT), int(g["weight_seed"]))
    ops = _ops(dtype, fused)
    eng = EN.ClipTextEngine(EN.pack_clip_text({"text_model." + k: v for k, v in sd.items()}, _cfg(EN.ClipTextConfig, E.TINY_TEXT), dtype, "cpu"), ops=ops)
    out = eng.encode(g["input_ids"])
    assert rel(out, g["last_hidden_state"]) < tol
    _expect(ops, fused, E.TINY_TEXT.num_hidden_layers)      # ONE launch per layer for the whole batch
    if fused:
        assert all(kw["causal"] and kw["batch"] == g["input_ids"].shape[0] for _, kw in ops.inner.calls)
        short = eng.encode(g["input_ids"][:, :20])                 # causal: a shorter prompt is a prefix computation
        assert rel(short, g["last_hidden_state"][:, :20]) < tol
        monkeypatch.setenv("FYC_SIDE_FLASH", "0")                  # read at every call: the same engine goes back to the materialised sequence
        ops.count.clear(), ops.order.clear()
        assert rel(eng.encode(g["input_ids"]), g["last_hidden_state"]) < tol
        _expect(ops, False, 0)
        assert ops.count["softmax_rows"] == E.TINY_TEXT.num_hidden_layers * g["input_ids"].shape[0]      # three launches per layer and batch element, as before


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "plain-emu"])
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 3e-2)])
def test_clip_vision_and_resampler_engines(golden_dir, monkeypatch, dtype, tol, fused):
    monkeypatch.delenv("FYC_SIDE_FLASH", raising=False)
    g = _load(golden_dir, "enc_clip_vision.npz")
    sd = E.make_encoder_weights(E.clip_vision_shapes(E.TINY_VISION), int(g["weight_seed"]))
    ops = _ops(dtype, fused)
    eng = EN.ClipVisionEngine(EN.pack_clip_vision(sd, _cfg(EN.ClipVisionConfig, E.TINY_VISION), dtype, "cpu"), ops=ops)
    out = eng.encode(g["pixel_values"], want=("image_embeds", "penultimate", "last"))
    for name in ("penultimate", "last", "image_embeds"):
        assert rel(out[name], g[name]) < tol, name
    _expect(ops, fused, E.TINY_VISION.num_hidden_layers)
    if fused:
        assert not any(kw["causal"] for _, kw in ops.inner.calls)
    gi = _load(golden_dir, "enc_ip_adapter.npz")
    sd_r = E.make_encoder_weights(E.resampler_shapes(E.TINY_RESAMPLER), int(gi["resampler_seed"]))
    ops = _ops(dtype, fused)
    res = EN.ResamplerEngine(EN.pack_resampler(sd_r, _cfg(EN.ResamplerConfig, E.TINY_RESAMPLER), dtype, "cpu"), ops=ops)
    assert rel(res.resample(gi["clip_hidden"]), gi["resampler_tokens"]) < tol
    _expect(ops, fused, E.TINY_RESAMPLER.depth)


def test_exact_f32_and_the_default_table_keep_a_call_site_materialised(monkeypatch):
    """exact f32 products: no fused launch whatever the switch says; a family the table lists as a loss is reached with FYC_SIDE_FLASH=force only"""
    monkeypatch.setenv("FYC_SIDE_FLASH", "force")
    exact = WideEmuOps(f32_products="exact")
    assert not EB.side_flash(exact, torch.float32, "vae", 512) and EB.side_flash(exact, torch.bfloat16, "vae", 512)
    assert not EB.side_flash(EmuOps(), torch.bfloat16, "vae", 512)                       # answers neither query
    assert not EB.side_flash(exact, torch.bfloat16, "vae", 544) and not EB.side_flash(exact, torch.bfloat16, "vae", 200)
    monkeypatch.setitem(EB.SIDE_FLASH_DEFAULT, ("vae", "bf16"), False)
    assert EB.side_flash(exact, torch.bfloat16, "vae", 512)
    monkeypatch.setenv("FYC_SIDE_FLASH", "1")
    assert not EB.side_flash(exact, torch.bfloat16, "vae", 512)
    monkeypatch.setenv("FYC_SIDE_FLASH", "0")
    assert not EB.side_flash(exact, torch.bfloat16, "clip_text", 64, True)
    assert set(EB.SIDE_FLASH_DEFAULT) == {(fam, dt) for fam in ("vae", "clip_text", "clip_vision", "resampler") for dt in ("bf16", "f16", "f32")}


# ---- the VAE's attention block -----------------------------------------------------------------------------------------------------------------------
VAE_C, VAE_HW, VAE_FRAMES = 512, 9, 2
# the block is four chained kernels - GroupNorm, the q | k | v GEMM, the attention, the output GEMM with the residual - each held to kernel_compare.RTOL of its dtype by
# its own tests; errors of a chain add at most linearly
VAE_TOL = {dt: 4 * KC.RTOL[dt] for dt in ("bf16", "f16", "f32")}


def vae_block_problem(dt):
    """-> (x [frames * 81][512] of the dtype, the packed attention weights, the f64 restatement of the block [frames * 81][512]); seeded, shared by the CPU and GPU tests"""
    T, g = A.DT[dt], torch.Generator().manual_seed(512 + 81)
    C, N, F = VAE_C, VAE_HW * VAE_HW, VAE_FRAMES
    x = torch.randn(F * N, C, generator=g).to(T)
    gw, gb = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    qkv_w, qkv_b = (torch.randn(3 * C, C, generator=g) * C ** -0.5).to(T), 0.1 * torch.randn(3 * C, generator=g)
    o_w, o_b = (torch.randn(C, C, generator=g) * C ** -0.5).to(T), 0.1 * torch.randn(C, generator=g)
    xd = x.double().reshape(F, N, 32, C // 32)
    mean, var = xd.mean(dim=(1, 3), keepdim=True), xd.var(dim=(1, 3), keepdim=True, unbiased=False)
    h = ((xd - mean) / torch.sqrt(var + 1e-6)).reshape(F, N, C) * gw.double() + gb.double()
    q, k, v = (h @ qkv_w.double().T + qkv_b.double()).split(C, dim=-1)
    att = torch.softmax(q @ k.transpose(-1, -2) * C ** -0.5, dim=-1) @ v
    ref = (att @ o_w.double().T + o_b.double()).reshape(F * N, C) + x.double()
    return x, dict(g=gw, b=gb, qkv_w=qkv_w, qkv_b=qkv_b, o_w=o_w, o_b=o_b), ref


def vae_engine(weights, dt, ops, device):
    eng = object.__new__(EV.VAEDecoderEngine)      # the block alone: no decoder weights
    eng.P, eng.cfg, eng.dtype, eng.ops, eng.device, eng.groups = None, None, A.DT[dt], ops, torch.device(device), 32
    return eng, Packed(**{k: v.to(device) for k, v in weights.items()})


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "plain-emu"])
@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_vae_attention_block(monkeypatch, dt, fused):
    monkeypatch.setenv("FYC_SIDE_FLASH", "force")      # the VAE's family lost the timing (engine/base.py::SIDE_FLASH_DEFAULT): fused on request only
    x, w, ref = vae_block_problem(dt)
    ops = _ops(A.DT[dt], fused)
    eng, a = vae_engine(w, dt, ops, "cpu")
    out = eng.attention(a, x, VAE_FRAMES, VAE_HW, VAE_HW)
    assert rel(out.double(), ref) < VAE_TOL[dt]
    _expect(ops, fused, 1)
    if fused:
        assert ops.inner.calls == [("attention", dict(batch=VAE_FRAMES, heads=1, n_q=81, n_k=81, d=512, causal=False))]
        monkeypatch.delenv("FYC_SIDE_FLASH")             # the default: the parent's sequence, also on an ops object that could run the fused launch
        ops.count.clear(), ops.order.clear()
        assert rel(eng.attention(a, x, VAE_FRAMES, VAE_HW, VAE_HW).double(), ref) < VAE_TOL[dt]
        _expect(ops, EB.SIDE_FLASH_DEFAULT["vae", dt], 1)
