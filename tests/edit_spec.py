"""The f64 specification of the three kernels of the image-editing front end (a helper, not a test module): fyc_posterior_latents, fyc_inpaint_prepare and
fyc_renoise_blend (csrc/image_edit.hip), from the very inputs the kernels get, with the per-element bounds their f32 evaluation is held to.

The bound is solver_spec's: every formula is evaluated twice, in f64 and with absolute values and additions (the pairs of P); an f32 evaluation whose longest path
makes K roundings differs from the exact value by at most gamma(K) S = ((1 + 2^-24)^K - 1) S.  Scalars (scale, c_x, c_n) are taken at their f32 values, as the
kernel gets them, and cost nothing.

The exponential.  The HIP math API's accuracy table (HIP documentation, "HIP math API", single-precision functions: `expf`, maximum error 1 ULP; it is the
figure tests/kernel_compare.py already charges expf in the softmax bound) gives expf at most 1 ulp, and 1 ulp of an f32 number is up to 2^-23 of its value, i.e.
2 roundings' worth: EXPF_ROUNDINGS = 2.  The table is not among the files ROCm installs; the figure is quoted from the published page.  The argument
0.5 * clamp(logvar, -30, 20) is exact in f32 (a power-of-two scaling of an f32 number inside [-30, 20]), so the exponential sees no argument error.

fyc_inpaint_prepare has no rounding at all: image * 1, image * 0, and the constants 0 and 1 are exact.  Both outputs are compared bit for bit.
"""
from collections import namedtuple

import torch

import sampling_spec as SS
from solver_spec import P, gamma, inside  # noqa: F401

VAE_SCALE = 0.18215

# ---- rounding counts, one f32 rounding each -------------------------------------------------------------------------------------------------------------
# fyc_posterior_latents, the longest path of a latents element with both noises: expf = EXPF_ROUNDINGS = 2 (0.5 * lv and the clamp are exact), std * noise_post = 3,
# mean + . = 4, * scale = 5 - this is z, K_CLEAN -, c_x * z = 6, + c_n * noise_add = 7 (c_n * noise_add itself is a shorter parallel branch).  Without
# noise_post z = mean * scale is one rounding and the latents three; the bound of the long path covers them.
EXPF_ROUNDINGS = 2
K_CLEAN = 3 + EXPF_ROUNDINGS
K_LATENTS = 5 + EXPF_ROUNDINGS
# The reference's own f32 path (DiagonalGaussianDistribution.sample, `0.18215 *`, add_noise) makes the same operations in the same order - torch.exp on the
# host is charged the same two -, so its results lie inside the same counts (tools/make_golden_edit.py asserts it).
# fyc_renoise_blend: c_x * orig = 1, + c_n * noise = 2, * m = 3; latents * (1 - m): 1 - m = 1, the product = 2 (the shorter branch); the sum = 4.
K_BLEND = 4


def f32(s):
    return float(torch.tensor(s, dtype=torch.float32))


def posterior_latents(moments, *, noise_post=None, noise_add=None, scale=VAE_SCALE, c_x=1.0, c_n=0.0):
    """moments (N, 2C, h, w) f32 -> dict(latents=(value f64, bound), clean=(value, bound)), all (N, C, h, w)"""
    C = moments.shape[1] // 2
    z = P(moments[:, :C])
    if noise_post is not None:
        std = torch.exp(0.5 * moments[:, C:].double().clamp(-30.0, 20.0))
        z = z + P(std * noise_post.double())
    z = f32(scale) * z
    lat = f32(c_x) * z
    if noise_add is not None:
        lat = lat + f32(c_n) * P(noise_add)
    return dict(latents=(lat.v, gamma(K_LATENTS) * lat.a), clean=(z.v, gamma(K_CLEAN) * z.a))


def inpaint_prepare(image, mask):
    """-> (masked (N, 3, H, W) f32, mask_latent (N, 1, H/8, W/8) f32): exact, compared bit for bit.  prepare_mask_and_masked_image and the nearest
    interpolation of the reference: binarise (< 0.5 -> 0, else 1), image * (mask < 0.5), the mask at pixel (8i, 8j)"""
    keep = (mask < 0.5).to(torch.float32)
    return image * keep, (1.0 - keep)[:, :, ::8, ::8].contiguous()


def renoise_blend(latents, orig, noise, mask, *, c_x, c_n, B, C, F, HW):
    """-> (value f64, bound), (B, C, F, HW)"""
    x = P(latents.reshape(B, C, F, HW))
    o, nz = P(orig.reshape(B, C, -1, HW)), P(noise.reshape(B, C, -1, HW))
    m = mask.reshape(B, 1, 1, HW).double()
    proper = f32(c_x) * o + f32(c_n) * nz
    keep, inv = P(proper.v * m, proper.a * m.abs()), 1.0 - m
    out = keep + P(x.v * inv, x.a * inv.abs())
    return out.v, gamma(K_BLEND) * out.a


# ---- the cases of the kernel tests (tests/test_edit.py on the emulator, tests/test_edit_gpu.py on the MI355X) ------------------------------------------
# (N, C, h, w): one element-quad; two samples, an odd row length; more than one block (3 * 4 * 33 * 31 = 12276 elements = 12 blocks of 256 quads), odd h and w
POSTERIOR_SHAPES = [(1, 4, 1, 1), (2, 4, 5, 7), (3, 4, 33, 31)]
# noise_post / noise_add / clean_out handed over or not: every nullable pointer, clean_out on and off
PostVariant = namedtuple("PostVariant", ["post", "add", "clean"])
POSTERIOR_VARIANTS = [PostVariant(p, a, c) for p in (False, True) for a in (False, True) for c in (False, True)]
POSTERIOR_COEF = (0.6523, 0.7580)                  # sqrt(abar), sqrt(1 - abar) near the middle of a Stable Diffusion schedule
# (N, H, W): one latent pixel; several, not square; two images, more than one block (2 * 264 * 248 / 4 = 32736 quads), H / 8 and W / 8 odd
PREPARE_SHAPES = [(1, 8, 8), (1, 40, 56), (2, 264, 248)]
MASK_VALUES = (0.0, 0.5, 1.0, 0.49999997, 0.50000003, 0.25, 0.75)       # exactly 0, 0.5, 1; the f32 neighbours of 0.5 on either side
BLEND_SHAPES = [(B, CL, F, HW) for (B, F, HW, CL, ld) in SS.SHAPES]        # the project's step-kernel shapes: HW = 20 takes the 16-byte path, 203 / 1031 / 37 the scalar one
BLEND_COEF = (0.6523, 0.7580)
_cache = {}


def posterior_operands(shape):
    """seeded moments and noises of a shape, built once and shared (never written).  The log-variances are spread over [-40, 30]: a part of them lies outside the
    clamp's [-30, 20] on either side"""
    if ("post", shape) not in _cache:
        N, C, h, w = shape
        g = torch.Generator().manual_seed(11 + 1000 * N + 10 * h + w)
        mean = torch.randn(N, C, h, w, generator=g)
        logvar = torch.rand(N, C, h, w, generator=g) * 70.0 - 40.0
        logvar.reshape(-1)[:2] = torch.tensor([-35.0, 25.0])[: logvar.numel()]
        _cache[("post", shape)] = dict(moments=torch.cat([mean, logvar], dim=1).contiguous(), noise_post=torch.randn(N, C, h, w, generator=g),
                                       noise_add=torch.randn(N, C, h, w, generator=g))
    return _cache[("post", shape)]


def posterior_reference(shape, var):
    o = posterior_operands(shape)
    return posterior_latents(o["moments"], noise_post=o["noise_post"] if var.post else None, noise_add=o["noise_add"] if var.add else None,
                             c_x=POSTERIOR_COEF[0], c_n=POSTERIOR_COEF[1])


def run_posterior(ops, shape, var, *, on=lambda t: t, nan_unread=False):
    """one launch on copies of the shared operands -> (latents, clean_out) on the ops' device; both start full of NaN, clean_out stays so when it is not handed
    over.  nan_unread: the log-variance half of the moments, which a variant without noise_post (the mode) does not read, is filled with NaN (the noises a
    variant does not read are NULL)"""
    o = posterior_operands(shape)
    N, C, h, w = shape
    moments = o["moments"].clone()
    if nan_unread and not var.post:
        moments[:, C:] = float("nan")
    lat, clean = on(torch.full(shape, float("nan"))), on(torch.full(shape, float("nan")))
    ops.posterior_latents(on(moments), lat, noise_post=on(o["noise_post"]) if var.post else None, noise_add=on(o["noise_add"]) if var.add else None,
                          clean_out=clean if var.clean else None, scale=VAE_SCALE, c_x=POSTERIOR_COEF[0], c_n=POSTERIOR_COEF[1])
    return lat, clean


def prepare_operands(shape):
    """seeded image in [-1, 1] and a mask whose pixels cycle through MASK_VALUES in a seeded order, so every value sits on sampled (8i, 8j) pixels and on others"""
    if ("prep", shape) not in _cache:
        N, H, W = shape
        g = torch.Generator().manual_seed(7 + 1000 * N + H + W)
        image = torch.rand(N, 3, H, W, generator=g) * 2.0 - 1.0
        vals = torch.tensor(MASK_VALUES, dtype=torch.float32)
        mask = vals[torch.randint(0, len(MASK_VALUES), (N, 1, H, W), generator=g)]
        mask[:, :, ::8, ::8] = vals[torch.arange(N * (H // 8) * (W // 8)).reshape(N, 1, H // 8, W // 8) % len(MASK_VALUES)]
        _cache[("prep", shape)] = dict(image=image.contiguous(), mask=mask.contiguous())
    return _cache[("prep", shape)]


def blend_operands(shape, full):
    """seeded latents, original, noise (full: the latents' shape, else (B, C, HW)) and a mask of exact 0 / 1 with a band of fractional values"""
    if ("blend", shape, full) not in _cache:
        B, C, F, HW = shape
        g = torch.Generator().manual_seed(23 + 1000 * B + 10 * F + HW + int(full))
        src = (B, C, F if full else 1, HW)
        mask = (torch.rand(B, 1, HW, generator=g) < 0.5).to(torch.float32)
        mask[:, :, ::5] = torch.rand(B, 1, len(range(0, HW, 5)), generator=g)
        _cache[("blend", shape, full)] = dict(latents=torch.randn(B, C, F, HW, generator=g), orig=torch.randn(src, generator=g),
                                              noise=torch.randn(src, generator=g), mask=mask.contiguous())
    return _cache[("blend", shape, full)]


def blend_reference(shape, full):
    B, C, F, HW = shape
    o = blend_operands(shape, full)
    return renoise_blend(o["latents"], o["orig"], o["noise"], o["mask"], c_x=BLEND_COEF[0], c_n=BLEND_COEF[1], B=B, C=C, F=F, HW=HW)


# ---- the cases of the golden file (tools/make_golden_edit.py writes them, tests/test_edit.py and tests/test_edit_gpu.py read them) ----------------------
STEPS, STRENGTH, T_START, GUIDANCE = 5, 0.6, 2, 8.0
PROMPT, NEGATIVE = "a corgi on the beach", "blurry"
SD_BETAS = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
# name -> (drop-in / reference scheduler class name, its constructor keywords)
SCHEDULERS = {
    "ddim": ("DDIMScheduler", dict(SD_BETAS, clip_sample=False, set_alpha_to_one=False, steps_offset=1, prediction_type="epsilon", rescale_betas_zero_snr=False)),
    "dpmpp2": ("DPMSolverMultistepScheduler", dict(SD_BETAS, solver_order=2, algorithm_type="dpmsolver++")),
    "euler": ("EulerDiscreteScheduler", dict(SD_BETAS)),
    "euler_a": ("EulerAncestralDiscreteScheduler", dict(SD_BETAS)),
    "lms": ("LMSDiscreteScheduler", dict(SD_BETAS)),
    "plms": ("PNDMScheduler", dict(SD_BETAS, skip_prk_steps=True, steps_offset=1)),
}
Case = namedtuple("Case", ["pipeline", "scheduler", "strength", "eta"])
CASES = ([Case("img2img", s, STRENGTH, 0.0) for s in SCHEDULERS] + [Case("img2img", "ddim", 1.0, 0.0), Case("img2img", "ddim", STRENGTH, 0.5)]
         + [Case("inpaint", s, None, 0.0) for s in ("ddim", "plms", "euler")] + [Case("legacy", s, STRENGTH, 0.0) for s in ("ddim", "plms", "euler")])
UNET_SEED, UNET9_SEED, VAE_SEED, INPUT_SEED, CALL_SEED = 12, 13, 3, 77, 5


def case_key(case):
    key = f"{case.pipeline}/{case.scheduler}"
    if case.strength is not None and case.strength != STRENGTH:
        key += f"/s{case.strength:g}"
    if case.eta:
        key += f"/eta{case.eta:g}"
    return key
