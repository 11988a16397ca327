"""fyc_attention with the causal mask and with head dims above 160 (ABI 308, csrc/attention_wide.h) on the cases of tests/attn_wide_spec.py (what each case launches and
that the list reaches every built instantiation is proven on the CPU by tests/test_attn_wide.py).  Every case is one launch into an output inside a larger, prefilled
buffer (attention_cases: 64 elements in front, two rows and the pad columns behind), compared with plain f64 attention over the visible keys by kernel_compare.compare:
finite, global rel-L2 at the tolerance of the dtype's existing attention tests, EVERY element within the bound of its family, nothing outside the output touched.  Then
the one-key identities of the tier, two launches for the same bits, and the engines: the VAE's attention block at C = 512 and the three encoder goldens through the
fused launch.

FYC_ATTN_WIDE_FIGURES=<file>: append the figures of every comparison to that file (profiles/wide_attention_bound_coverage.txt was made from it)."""
import os

import pytest
import torch

import attention_cases as A
import attn_wide_spec as WS
import f32x3_spec as X
from followyourclick_amd.engine import encoders as EN
from kernel_compare import Guard, compare
from oracle import encoders as E
from test_attn_wide import VAE_FRAMES, VAE_HW, VAE_TOL, _cfg, _load, rel, vae_block_problem, vae_engine
from test_kernels_gpu import hip  # noqa: F401  (the module-scoped library fixture)

pytestmark = pytest.mark.gpu

FIGURES = os.environ.get("FYC_ATTN_WIDE_FIGURES")


def launch(hip, c, ops):  # noqa: F811
    """one launch of the case into a fresh copy of its guarded buffer; returns that buffer (CPU)"""
    f = c.f
    buf = ops.buf.cuda()
    hip.attention(ops.q.cuda(), ops.k.cuda(), ops.vt.cuda(), A.out_view(f, buf), batch=f.B, heads=f.H, n_q=f.n_q, n_k=f.n_k, d=f.d, ldo=f.ldo, ldvt=f.ldvt, scale=f.scale,
                  kv_batch_div=f.div, q_batch_mod=f.mod, accumulate=f.accumulate, o_scale=f.o_scale, causal=c.causal, products="split" if f.dt == "f32" else None)
    torch.cuda.synchronize()
    return buf.cpu()


def _run(hip, c):  # noqa: F811
    f = c.f
    ops, ref, bound = WS.reference(c)
    got = launch(hip, c, ops)
    fig = compare(A.window(f, got), A.window(f, ref), dtype=f.dt, bound=bound, rtol=f.rtol, labels=WS.labels(c), guard=Guard(ops.buf, got, ops.mask), tag=c.name)
    print(f"{c.name}: global rel-L2 {fig['global_rel']:.3e} (tolerance {f.rtol:.1e}), worst element at {fig['elem_ratio']:.3f} of its bound")
    if FIGURES:
        with open(FIGURES, "a") as fh:
            fh.write(f"{f.group} {f.dt} {'causal' if c.causal else 'full'} {c.recipe} {c.name} {fig['global_rel']:.3e} {fig['elem_ratio']:.4f}\n")
    return got


WIDE, CAUSAL = WS.by_group("W", "X"), WS.by_group("C")


@pytest.mark.parametrize("case", WIDE, ids=WS.case_ids(WIDE))
def test_wide_heads_inside_the_bound(hip, case):  # noqa: F811
    """W, X: d = 192, 256, 320, 512 in bf16, f16 and f32 with split products; the (n_q, n_k) and (batch, heads) lists; accumulate, kv_batch_div, pad keys, the XCD order"""
    _run(hip, case)


@pytest.mark.parametrize("case", CAUSAL, ids=WS.case_ids(CAUSAL))
def test_causal_inside_the_bound(hip, case):  # noqa: F811
    """C: d = 8 .. 160, 320 and 512 with the mask, n = 1 .. 130, random operands and the discriminating set (every removed score at least 40 log2 units above every kept
    one: a removed key that reaches the maximum or the sum takes the row over)"""
    _run(hip, case)


def _tier_case(d, n_q, n_k, causal, B=2, H=3):
    return WS._case("K", "f32", B, H, n_q, n_k, d, causal=causal)


def _bits(c, buf):
    return A.window(c.f, buf).contiguous().view(torch.int32)


@pytest.mark.parametrize("d", [40, 160, 512])
def test_causal_row_zero_is_hi_plus_lo_of_v0(hip, d):  # noqa: F811
    """the tier's one-key property (ABI 307) under the mask: query 0 sees key 0 only, so p = l = 1 and row 0 is hi(v_0) + lo(v_0) bit for bit - not v_0"""
    c = _tier_case(d, 33, 33, True)
    f = c.f
    ops = WS.operands(c)
    got = A.window(f, launch(hip, c, ops)).reshape(f.B, f.n_q, f.H, f.d)[:, 0]
    v0 = torch.stack([ops.vt[A.kv_of(f, b), :, :, 0] for b in range(f.B)])
    hi, lo = X.split_bf16(v0)
    assert torch.equal(got.contiguous().view(torch.int32), (hi + lo).contiguous().view(torch.int32))
    assert (got != v0).float().mean().item() >= 0.5


@pytest.mark.parametrize("d", [192, 320, 512])
def test_wide_one_key_returns_hi_plus_lo(hip, d):  # noqa: F811
    c = _tier_case(d, 70, 1, False)
    f = c.f
    ops = WS.operands(c)
    got = A.window(f, launch(hip, c, ops)).reshape(f.B, f.n_q, f.H, f.d)
    v = torch.stack([ops.vt[A.kv_of(f, b), :, :, 0] for b in range(f.B)])[:, None].expand(f.B, f.n_q, f.H, f.d)
    hi, lo = X.split_bf16(v.contiguous())
    assert torch.equal(got.contiguous().view(torch.int32), (hi + lo).view(torch.int32))
    assert (got != v).float().mean().item() >= 0.5


@pytest.mark.parametrize("name", ["X-bf16-d512-b2h1-nq65-nk33-acc", "X-f32-d256-b1h1-nq270-nk150", "C-f16-d64-b2h12-nq77-nk77-causal", "C-f32-d512-b1h1-nq130-nk130-causal-disc"])
def test_two_launches_give_the_same_bits(hip, name):  # noqa: F811
    c = next(c for c in WS.CASES if c.name == name)
    ops = WS.reference(c)[0]
    a, b = launch(hip, c, ops), launch(hip, c, ops)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


# ---- engines -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def split_ops(hip, monkeypatch):  # noqa: F811
    """the process's HipOps with split products for f32 tensors, restored afterwards; FYC_SIDE_FLASH=force: the fused launch whatever the measured default says"""
    before = hip.f32_products
    hip.set_f32_products("split")
    monkeypatch.setenv("FYC_SIDE_FLASH", "force")
    yield hip
    hip.set_f32_products(before)


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_vae_attention_block_fused_and_materialised(split_ops, monkeypatch, dt):
    """C = 512 on a 9 x 9 latent, 2 frames: the fused launch against the f64 restatement of the block, and against the same engine with FYC_SIDE_FLASH=0"""
    x, w, ref = vae_block_problem(dt)
    eng, a = vae_engine(w, dt, split_ops, "cuda")
    fused = eng.attention(a, x.cuda(), VAE_FRAMES, VAE_HW, VAE_HW).cpu().double()
    monkeypatch.setenv("FYC_SIDE_FLASH", "0")
    mat = eng.attention(a, x.cuda(), VAE_FRAMES, VAE_HW, VAE_HW).cpu().double()
    print(f"vae block {dt}: fused {rel(fused, ref):.3e}, materialised {rel(mat, ref):.3e}, fused vs materialised {rel(fused, mat):.3e} (tolerance {VAE_TOL[dt]:.1e})")
    assert rel(fused, ref) < VAE_TOL[dt] and rel(mat, ref) < VAE_TOL[dt]
    assert rel(fused, mat) < 2 * VAE_TOL[dt]
    assert not torch.equal(fused, mat)      # two different launch sequences ran


class _Spy:
    def __init__(self, inner):
        self.inner, self.attn = inner, []

    def __getattr__(self, name):
        v = getattr(self.inner, name)
        if name != "attention":
            return v

        def call(*a, **kw):
            self.attn.append(kw)
            return v(*a, **kw)
        return call


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 3e-2)])
def test_encoder_goldens_through_the_fused_launch(golden_dir, split_ops, dtype, tol):
    """the three encoder goldens at the tolerances of tests/test_encoders_gpu.py (f32: here with split products), one fyc_attention launch per layer; the prefix
    property of the causal text tower"""
    g = _load(golden_dir, "enc_clip_text.npz")
    sd = E.make_encoder_weights(E.clip_text_shapes(E.TINY_TEXT), int(g["weight_seed"]))
    spy = _Spy(split_ops)
    eng = EN.ClipTextEngine(EN.pack_clip_text({"text_model." + k: v for k, v in sd.items()}, _cfg(EN.ClipTextConfig, E.TINY_TEXT), dtype, "cuda"), ops=spy)
    assert rel(eng.encode(g["input_ids"]).cpu(), g["last_hidden_state"]) < tol
    assert len(spy.attn) == E.TINY_TEXT.num_hidden_layers and all(kw["causal"] and kw["batch"] == g["input_ids"].shape[0] for kw in spy.attn)
    assert rel(eng.encode(g["input_ids"][:, :20]).cpu(), g["last_hidden_state"][:, :20]) < tol

    g = _load(golden_dir, "enc_clip_vision.npz")
    sd = E.make_encoder_weights(E.clip_vision_shapes(E.TINY_VISION), int(g["weight_seed"]))
    spy = _Spy(split_ops)
    eng = EN.ClipVisionEngine(EN.pack_clip_vision(sd, _cfg(EN.ClipVisionConfig, E.TINY_VISION), dtype, "cuda"), ops=spy)
    out = eng.encode(g["pixel_values"], want=("image_embeds", "penultimate", "last"))
    for name in ("penultimate", "last", "image_embeds"):
        assert rel(out[name].cpu(), g[name]) < tol, name
    assert len(spy.attn) == E.TINY_VISION.num_hidden_layers

    g = _load(golden_dir, "enc_ip_adapter.npz")
    sd_r = E.make_encoder_weights(E.resampler_shapes(E.TINY_RESAMPLER), int(g["resampler_seed"]))
    spy = _Spy(split_ops)
    res = EN.ResamplerEngine(EN.pack_resampler(sd_r, _cfg(EN.ResamplerConfig, E.TINY_RESAMPLER), dtype, "cuda"), ops=spy)
    assert rel(res.resample(g["clip_hidden"]).cpu(), g["resampler_tokens"]) < tol
    assert len(spy.attn) == E.TINY_RESAMPLER.depth
