// The front end of the image-editing pipelines (img2img, inpainting): encoded image -> noised start latents, mask and masked image, and the
// legacy inpainting loop's re-imposition of the known region.  Three HBM-bound f32 kernels: no atomics, no reductions, every output element is
// one fixed f32 expression of its inputs (the library is built with -ffp-contract=off), so the same call gives the same bits.  Each has a
// 16-byte path (four consecutive elements per lane and load / store) taken when the innermost extent is a multiple of four and every pointer
// is 16-byte aligned, and a scalar path for everything else.
#include "fyc_common.h"

namespace {

inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }
inline int blocks_for(long long n) {
  const long long b = ceil_div(n, 256);
  return (int)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- fyc_posterior_latents ----------------------------------------------------------------------------------------------------------------
// one element: z = (mean + expf(0.5 clamp(logvar, -30, 20)) * noise_post) * scale (POST; else z = mean * scale: the mode), in the order of
// DiagonalGaussianDistribution.sample, `0.18215 *`, add_noise: lat = c_x z + c_n noise_add (ADD; else lat = c_x z)
template <bool POST, bool ADD>
__device__ __forceinline__ void posterior_one(float mean, float logvar, float npost, float nadd, float scale, float c_x, float c_n,
                                              float& z, float& lat) {
  float s = mean;
  if (POST) {
    const float lv = fminf(fmaxf(logvar, -30.f), 20.f);
    s = mean + expf(0.5f * lv) * npost;
  }
  z = s * scale;
  lat = c_x * z;
  if (ADD) lat = lat + c_n * nadd;
}

// VEC = 4: `per` (= C h w, the elements of one sample's mean block) is a multiple of 4, so four consecutive elements never leave the block
template <int VEC, bool POST, bool ADD, bool CLEAN>
__global__ void __launch_bounds__(256) posterior_latents_kernel(const float* __restrict__ moments, const float* __restrict__ noise_post,
                                                                const float* __restrict__ noise_add, float* __restrict__ latents,
                                                                float* __restrict__ clean, long long chunks, long long per, float scale,
                                                                float c_x, float c_n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (long long)gridDim.x * 256) {
    const long long e = i * VEC;                  // first element of the chunk in (N, C, h, w) order
    const long long n = e / per;
    const long long m = e + n * per;              // its mean in (N, 2C, h, w): sample n starts at 2 n per; the log-variance `per` further
    float mean[VEC], lv[VEC], np[VEC], na[VEC], z[VEC], lat[VEC];
    if (VEC == 4) {
      ElemIO<float>::ld4(moments + m, mean);
      if (POST) { ElemIO<float>::ld4(moments + m + per, lv); ElemIO<float>::ld4(noise_post + e, np); }
      if (ADD) ElemIO<float>::ld4(noise_add + e, na);
    } else {
      mean[0] = moments[m];
      if (POST) { lv[0] = moments[m + per]; np[0] = noise_post[e]; }
      if (ADD) na[0] = noise_add[e];
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k)
      posterior_one<POST, ADD>(mean[k], POST ? lv[k] : 0.f, POST ? np[k] : 0.f, ADD ? na[k] : 0.f, scale, c_x, c_n, z[k], lat[k]);
    if (VEC == 4) {
      ElemIO<float>::st4(latents + e, lat);
      if (CLEAN) ElemIO<float>::st4(clean + e, z);
    } else {
      latents[e] = lat[0];
      if (CLEAN) clean[e] = z[0];
    }
  }
}

template <int VEC, bool POST, bool ADD>
void posterior_launch(const fyc_posterior_latents_args* a, long long chunks, long long per, hipStream_t st) {
  if (a->clean_out)
    hipLaunchKernelGGL((posterior_latents_kernel<VEC, POST, ADD, true>), dim3(blocks_for(chunks)), dim3(256), 0, st, a->moments, a->noise_post,
                       a->noise_add, a->latents, a->clean_out, chunks, per, a->scale, a->c_x, a->c_n);
  else
    hipLaunchKernelGGL((posterior_latents_kernel<VEC, POST, ADD, false>), dim3(blocks_for(chunks)), dim3(256), 0, st, a->moments, a->noise_post,
                       a->noise_add, a->latents, a->clean_out, chunks, per, a->scale, a->c_x, a->c_n);
}

template <int VEC>
void posterior_dispatch(const fyc_posterior_latents_args* a, long long chunks, long long per, hipStream_t st) {
  if (a->noise_post && a->noise_add) posterior_launch<VEC, true, true>(a, chunks, per, st);
  else if (a->noise_post) posterior_launch<VEC, true, false>(a, chunks, per, st);
  else if (a->noise_add) posterior_launch<VEC, false, true>(a, chunks, per, st);
  else posterior_launch<VEC, false, false>(a, chunks, per, st);
}

// ---- fyc_inpaint_prepare ------------------------------------------------------------------------------------------------------------------
// one lane: four pixels of one image row (W is a multiple of 8, so a chunk never leaves its row and chunk 0 / 2 of every eight pixels holds
// the pixel a latent-size mask element samples).  keep = mask < 0.5 as 1.f / 0.f and a true product, as the reference multiplies by the
// boolean: a negative pixel under the mask becomes -0.f there and here
template <bool IMG, bool LAT>
__global__ void __launch_bounds__(256) inpaint_prepare_kernel(const float* __restrict__ image, const float* __restrict__ mask,
                                                              float* __restrict__ masked, float* __restrict__ mask_latent, long long chunks,
                                                              int H, int W) {
  const int w4 = W >> 2;
  const long long plane = (long long)H * W;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (long long)gridDim.x * 256) {
    const int x = (int)(i % w4) << 2;
    const long long ny = i / w4;
    const int y = (int)(ny % H);
    const long long n = ny / H;
    float m[4];
    ElemIO<float>::ld4(mask + n * plane + (long long)y * W + x, m);
    if (IMG) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const long long o = (n * 3 + c) * plane + (long long)y * W + x;
        float v[4];
        ElemIO<float>::ld4(image + o, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v[k] * (m[k] < 0.5f ? 1.f : 0.f);
        ElemIO<float>::st4(masked + o, v);
      }
    }
    if (LAT && (y & 7) == 0 && (x & 7) == 0)
      mask_latent[(n * (H >> 3) + (y >> 3)) * (W >> 3) + (x >> 3)] = m[0] < 0.5f ? 0.f : 1.f;
  }
}

// the latent-size mask alone: one lane per output element, the image is not read
__global__ void __launch_bounds__(256) inpaint_mask_kernel(const float* __restrict__ mask, float* __restrict__ mask_latent, long long total,
                                                           int H, int W) {
  const int h8 = H >> 3, w8 = W >> 3;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int j = (int)(i % w8);
    const long long ni = i / w8;
    const int r = (int)(ni % h8);
    const long long n = ni / h8;
    mask_latent[i] = mask[(n * H + 8LL * r) * W + 8 * j] < 0.5f ? 0.f : 1.f;
  }
}

// ---- fyc_renoise_blend --------------------------------------------------------------------------------------------------------------------
// latents = (c_x orig + c_n noise) m + latents (1 - m), the order of add_noise and of the legacy inpainting loop's blend
template <int VEC>
__global__ void __launch_bounds__(256) renoise_blend_kernel(float* __restrict__ latents, const float* __restrict__ orig,
                                                            const float* __restrict__ noise, const float* __restrict__ mask, long long chunks,
                                                            int C, int F, int HW, int src_frames, float c_x, float c_n) {
  const int per_row = HW / VEC;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (long long)gridDim.x * 256) {
    const int p = (int)(i % per_row) * VEC;
    const long long bcf = i / per_row;
    const int f = (int)(bcf % F);
    const long long bc = bcf / F;
    const long long b = bc / C;
    const long long l = bcf * HW + p;
    const long long s = (bc * src_frames + (src_frames > 1 ? f : 0)) * HW + p;
    const long long mi = b * HW + p;
    float x[VEC], o[VEC], nz[VEC], m[VEC];
    if (VEC == 4) {
      ElemIO<float>::ld4(latents + l, x); ElemIO<float>::ld4(orig + s, o); ElemIO<float>::ld4(noise + s, nz); ElemIO<float>::ld4(mask + mi, m);
    } else {
      x[0] = latents[l]; o[0] = orig[s]; nz[0] = noise[s]; m[0] = mask[mi];
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) x[k] = (c_x * o[k] + c_n * nz[k]) * m[k] + x[k] * (1.f - m[k]);
    if (VEC == 4) ElemIO<float>::st4(latents + l, x);
    else latents[l] = x[0];
  }
}

}  // namespace

extern "C" int fyc_posterior_latents(const fyc_posterior_latents_args* a, void* stream) {
  FYC_REQUIRE(a && a->moments && a->latents, "fyc_posterior_latents: null pointer");
  FYC_REQUIRE(a->N > 0 && a->C > 0 && a->HW > 0, "fyc_posterior_latents: bad dims");
  const long long per = (long long)a->C * a->HW, n = per * a->N;
  auto overlaps = [n](const float* p, long long np, const float* q) { return p != nullptr && q != nullptr && p < q + n && q < p + np; };
  const float* ins[3] = {a->moments, a->noise_post, a->noise_add};
  const long long in_n[3] = {2 * n, n, n};
  const char* in_names[3] = {"moments", "noise_post", "noise_add"};
  for (int k = 0; k < 3; ++k) {
    FYC_REQUIRE(!overlaps(ins[k], in_n[k], a->latents), "fyc_posterior_latents: latents aliases %s", in_names[k]);
    FYC_REQUIRE(!overlaps(ins[k], in_n[k], a->clean_out), "fyc_posterior_latents: clean_out aliases %s", in_names[k]);
  }
  FYC_REQUIRE(!overlaps(a->latents, n, a->clean_out), "fyc_posterior_latents: clean_out aliases latents");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = per % 4 == 0 && aligned16(a->moments) && aligned16(a->latents) && (a->noise_post == nullptr || aligned16(a->noise_post)) &&
                   (a->noise_add == nullptr || aligned16(a->noise_add)) && (a->clean_out == nullptr || aligned16(a->clean_out));
  if (vec) posterior_dispatch<4>(a, n / 4, per, st);
  else posterior_dispatch<1>(a, n, per, st);
  FYC_CHECK_LAUNCH("fyc_posterior_latents");
  return 0;
}

extern "C" int fyc_inpaint_prepare(const fyc_inpaint_prepare_args* a, void* stream) {
  FYC_REQUIRE(a && a->mask, "fyc_inpaint_prepare: null pointer");
  FYC_REQUIRE(a->masked != nullptr || a->mask_latent != nullptr, "fyc_inpaint_prepare: neither output was handed over");
  FYC_REQUIRE(a->masked == nullptr || a->image != nullptr, "fyc_inpaint_prepare: the masked image needs the image");
  FYC_REQUIRE(a->N > 0 && a->H > 0 && a->W > 0 && a->H % 8 == 0 && a->W % 8 == 0, "fyc_inpaint_prepare: H = %d and W = %d must be positive multiples of 8", a->H, a->W);
  const long long px = (long long)a->N * a->H * a->W;
  auto overlaps = [](const float* p, long long np, const float* q, long long nq) { return p != nullptr && q != nullptr && p < q + nq && q < p + np; };
  FYC_REQUIRE(!overlaps(a->masked, 3 * px, a->image, 3 * px) && !overlaps(a->masked, 3 * px, a->mask, px), "fyc_inpaint_prepare: masked aliases an input");
  FYC_REQUIRE(!overlaps(a->mask_latent, px / 64, a->masked ? a->image : nullptr, 3 * px) && !overlaps(a->mask_latent, px / 64, a->mask, px) &&
              !overlaps(a->mask_latent, px / 64, a->masked, 3 * px), "fyc_inpaint_prepare: mask_latent aliases another buffer");
  hipStream_t st = (hipStream_t)stream;
  if (a->masked == nullptr) {
    hipLaunchKernelGGL(inpaint_mask_kernel, dim3(blocks_for(px / 64)), dim3(256), 0, st, a->mask, a->mask_latent, px / 64, a->H, a->W);
  } else {
    // (W % 8 == 0: rows keep the alignment of their plane)
    FYC_REQUIRE(aligned16(a->image) && aligned16(a->mask) && aligned16(a->masked), "fyc_inpaint_prepare: image, mask and masked must be 16-byte aligned");
    if (a->mask_latent)
      hipLaunchKernelGGL((inpaint_prepare_kernel<true, true>), dim3(blocks_for(px / 4)), dim3(256), 0, st, a->image, a->mask, a->masked, a->mask_latent, px / 4, a->H, a->W);
    else
      hipLaunchKernelGGL((inpaint_prepare_kernel<true, false>), dim3(blocks_for(px / 4)), dim3(256), 0, st, a->image, a->mask, a->masked, a->mask_latent, px / 4, a->H, a->W);
  }
  FYC_CHECK_LAUNCH("fyc_inpaint_prepare");
  return 0;
}

extern "C" int fyc_renoise_blend(const fyc_renoise_blend_args* a, void* stream) {
  FYC_REQUIRE(a && a->latents && a->orig && a->noise && a->mask, "fyc_renoise_blend: null pointer");
  FYC_REQUIRE(a->B > 0 && a->C > 0 && a->F > 0 && a->HW > 0, "fyc_renoise_blend: bad dims");
  FYC_REQUIRE(a->src_frames == 1 || a->src_frames == a->F, "fyc_renoise_blend: src_frames %d must be 1 or F = %d", a->src_frames, a->F);
  const long long n = (long long)a->B * a->C * a->F * a->HW, ns = (long long)a->B * a->C * a->src_frames * a->HW, nm = (long long)a->B * a->HW;
  auto overlaps = [a, n](const float* q, long long nq) { return a->latents < q + nq && q < a->latents + n; };
  FYC_REQUIRE(!overlaps(a->orig, ns) && !overlaps(a->noise, ns) && !overlaps(a->mask, nm), "fyc_renoise_blend: latents aliases an input");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = a->HW % 4 == 0 && aligned16(a->latents) && aligned16(a->orig) && aligned16(a->noise) && aligned16(a->mask);
  if (vec)
    hipLaunchKernelGGL(renoise_blend_kernel<4>, dim3(blocks_for(n / 4)), dim3(256), 0, st, a->latents, a->orig, a->noise, a->mask, n / 4, a->C, a->F, a->HW, a->src_frames, a->c_x, a->c_n);
  else
    hipLaunchKernelGGL(renoise_blend_kernel<1>, dim3(blocks_for(n)), dim3(256), 0, st, a->latents, a->orig, a->noise, a->mask, n, a->C, a->F, a->HW, a->src_frames, a->c_x, a->c_n);
  FYC_CHECK_LAUNCH("fyc_renoise_blend");
  return 0;
}
