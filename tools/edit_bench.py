"""Measurements behind profiles/image_edit.txt (one MI355X).  bench.py is the yardstick of the animation clip; this tool times what the image-editing pipelines add in
front of and inside the 2-D loop, and the calls themselves.

  python tools/edit_bench.py kernels [--launches 200]      fyc_posterior_latents (both noises, clean_out), fyc_inpaint_prepare (both outputs) and fyc_renoise_blend
                                                           at the shapes of a 512 x 512 edit (64 x 64 latents, batch 1): device-event time per launch and the bytes
                                                           each launch must move -> achieved GB/s
  python tools/edit_bench.py calls [--steps 20] [--repeat 5] [--which t2i,img2img,inpaint,legacy]
                                                           whole pipeline calls at 512 x 512 with Stable Diffusion 1.5's widths (random weights, the stub text encoder,
                                                           bf16, DDIM, CFG 7.5): host clock around a call that ends in the decoded image on the host, median of --repeat
                                                           after one warm-up call.  img2img at strength 1.0 and legacy inpainting at strength 1.0 run all --steps
                                                           entries, so the difference to text-to-image is the front end (VAE encoder, the new kernels) and the blend
  python tools/edit_bench.py calls --tree PATH --which t2i another checkout's text-to-image call (the parent commit's, built there) with the same models and clock
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernels(launches):
    sys.path.insert(0, ROOT)
    from followyourclick_amd import ops
    hip, dev = ops.get(), "cuda:0"
    g = torch.Generator().manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)      # noqa: E731
    moments, n_post, n_add, lat, clean = rn(1, 8, 64, 64), rn(1, 4, 64, 64), rn(1, 4, 64, 64), rn(1, 4, 64, 64), rn(1, 4, 64, 64)
    image, mask = (torch.rand(1, 3, 512, 512, generator=g) * 2 - 1).to(dev), torch.rand(1, 1, 512, 512, generator=g).to(dev)
    masked, mask_lat = torch.empty_like(image), torch.empty(1, 1, 64, 64, device=dev)
    x0, x, orig, noise, m = rn(1, 4, 1, 4096), rn(1, 4, 1, 4096), rn(1, 4, 4096), rn(1, 4, 4096), (torch.rand(1, 1, 4096, generator=g) < 0.5).float().to(dev)
    f = 4          # bytes per f32
    calls = {
        # moments (mean and log-variance) + two noises read, latents + clean_out written
        "posterior_latents 1x4x64x64 (noise_post, noise_add, clean_out)": (lambda: hip.posterior_latents(moments, lat, noise_post=n_post, noise_add=n_add, clean_out=clean,
                                                                                                         scale=0.18215, c_x=0.65, c_n=0.76), (8 + 4 + 4 + 4 + 4) * 4096 * f),
        # image + mask read, masked image + latent-size mask written
        "inpaint_prepare 1x3x512x512 (masked, mask_latent)": (lambda: hip.inpaint_prepare(image, mask, masked=masked, mask_latent=mask_lat), (3 + 1 + 3) * 512 * 512 * f + 4096 * f),
        # latents read and written, original + noise + mask read
        "renoise_blend 1x4x1x4096": (lambda: hip.renoise_blend(x, orig, noise, m, c_x=0.65, c_n=0.76, B=1, C_=4, F=1, HW=4096), (4 + 4 + 4 + 4 + 1) * 4096 * f),
    }
    for name, (fn, nbytes) in calls.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
        for a, b in ev:
            x.copy_(x0)            # (the in-place blend of repeated launches: reset outside the timed pair)
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        us = sorted(1000.0 * a.elapsed_time(b) for a, b in ev)
        med = us[len(us) // 2]
        print(f"{name:66s} {launches} launches, device events: median {med:6.1f} us, min {us[0]:6.1f} us, max {us[-1]:6.1f} us; {nbytes / 1e3:8.1f} kB "
              f"-> {nbytes / med / 1e3:7.1f} GB/s at the median")


def calls(tree, steps, repeat, which):
    sys.path.insert(0, tree)
    import followyourclick_amd
    assert os.path.samefile(os.path.dirname(os.path.dirname(followyourclick_amd.__file__)), tree), followyourclick_amd.__file__
    followyourclick_amd.install_dropin(force=True)
    import diffusers
    from oracle import stubs
    dev, dtype = "cuda", torch.bfloat16
    torch.manual_seed(0)
    vae = diffusers.AutoencoderKL(block_out_channels=(128, 256, 512, 512), layers_per_block=2, latent_channels=4, compute_dtype=dtype)
    sched = lambda: diffusers.DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,      # noqa: E731
                                            set_alpha_to_one=False, steps_offset=1, prediction_type="epsilon")
    parts = dict(vae=vae, text_encoder=stubs.StubTextEncoder(768), tokenizer=stubs.FakeTokenizer(), safety_checker=None)
    unets = {}

    def unet(in_channels):
        if in_channels not in unets:
            unets[in_channels] = diffusers.UNet2DConditionModel(sample_size=64, in_channels=in_channels, cross_attention_dim=768, compute_dtype=dtype)
        return unets[in_channels]
    g = torch.Generator().manual_seed(1)
    image = torch.rand(1, 3, 512, 512, generator=g) * 2 - 1
    mask = torch.zeros(1, 1, 512, 512)
    mask[:, :, 128:384, 128:384] = 1.0
    kw = dict(num_inference_steps=steps, guidance_scale=7.5, output_type="np")
    for name in which:
        gen = lambda: torch.Generator().manual_seed(2)      # noqa: E731
        if name == "t2i":
            pipe = diffusers.StableDiffusionPipeline.from_pretrained("unused", unet=unet(4), scheduler=sched(), **parts).to(dev)
            fn = lambda: pipe("a corgi on the beach", height=512, width=512, generator=gen(), **kw)      # noqa: E731
        elif name == "img2img":
            pipe = diffusers.StableDiffusionImg2ImgPipeline.from_pretrained("unused", unet=unet(4), scheduler=sched(), **parts).to(dev)
            fn = lambda: pipe("a corgi on the beach", image=image, strength=1.0, generator=gen(), **kw)      # noqa: E731
        elif name == "legacy":
            pipe = diffusers.StableDiffusionInpaintPipelineLegacy.from_pretrained("unused", unet=unet(4), scheduler=sched(), **parts).to(dev)
            m4 = 1 - mask[:, :, ::8, ::8].expand(1, 4, 64, 64)
            fn = lambda: pipe("a corgi on the beach", image=image, mask_image=m4, strength=1.0, generator=gen(), **kw)      # noqa: E731
        else:
            pipe = diffusers.StableDiffusionInpaintPipeline.from_pretrained("unused", unet=unet(9), scheduler=sched(), **parts).to(dev)
            fn = lambda: pipe("a corgi on the beach", image=image, mask_image=mask.clone(), height=512, width=512, generator=gen(), **kw)      # noqa: E731
        pipe.progress_bar = lambda iterable=None, total=None: iterable          # no progress output in the timed window
        fn()                                                                    # warm-up: packs the weights, loads every kernel of every shape
        torch.cuda.synchronize()
        ms = []
        for _ in range(repeat):
            t0 = time.perf_counter()
            fn()                                                                # (ends in the decoded image on the host: a device synchronise)
            ms.append(1000.0 * (time.perf_counter() - t0))
        print(f"{name:8s} 512x512, {steps} steps, bf16, tree {tree}: median {statistics.median(ms):8.1f} ms per call, min {min(ms):8.1f}, max {max(ms):8.1f} ({repeat} calls)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    k = sub.add_parser("kernels")
    k.add_argument("--launches", type=int, default=200)
    c = sub.add_parser("calls")
    c.add_argument("--tree", default=ROOT)
    c.add_argument("--steps", type=int, default=20)
    c.add_argument("--repeat", type=int, default=5)
    c.add_argument("--which", default="t2i,img2img,inpaint,legacy")
    args = ap.parse_args()
    if args.mode == "kernels":
        kernels(args.launches)
    else:
        calls(os.path.abspath(args.tree), args.steps, args.repeat, args.which.split(","))
