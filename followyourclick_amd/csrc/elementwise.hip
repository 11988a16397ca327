// Small HBM-bound kernels around the UNet/VAE: layout changes at the API boundary
// ((b,c,f,h,w) f32 <-> channels-last), channel concat, guidance + DDIM update, casts.
#include <type_traits>

#include "fyc_common.h"

namespace {

template <typename T>
__global__ void __launch_bounds__(256) concat_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ y,
                                                     long long chunks, int c1_8, int c2_8) {
  const int ct8 = c1_8 + c2_8;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < chunks; idx += (long long)gridDim.x * 256) {
    const long long row = idx / ct8;
    const int c = (int)(idx - row * ct8);
    const u32x4* src = (c < c1_8) ? reinterpret_cast<const u32x4*>(a) + (row * c1_8 + c) * (int)(sizeof(T) * 8 / 16)
                                  : reinterpret_cast<const u32x4*>(b) + (row * c2_8 + (c - c1_8)) * (int)(sizeof(T) * 8 / 16);
    u32x4* dst = reinterpret_cast<u32x4*>(y) + idx * (int)(sizeof(T) * 8 / 16);
#pragma unroll
    for (int k = 0; k < (int)(sizeof(T) * 8 / 16); ++k) dst[k] = src[k];
  }
}

// dst = `times` back-to-back copies of src: every 16-byte chunk is read once and stored `times` times
__global__ void __launch_bounds__(256) repeat_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, long long chunks, int times) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (long long)gridDim.x * 256) {
    const u32x4 v = src[i];
    for (int t = 0; t < times; ++t) dst[t * chunks + i] = v;
  }
}

__global__ void __launch_bounds__(256) silu_kernel(const float* __restrict__ x, float* __restrict__ y, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) y[i] = silu_f(x[i]);
}

template <typename T>
__global__ void __launch_bounds__(256) cast_from_kernel(const float* __restrict__ x, T* __restrict__ y, long long rows, int cols, int ld) {
  const long long n = rows * ld;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long r = i / ld;
    const int c = (int)(i - r * ld);
    ElemIO<T>::st(y + i, c < cols ? x[r * cols + c] : 0.f);
  }
}
template <typename T>
__global__ void __launch_bounds__(256) cast_to_kernel(const T* __restrict__ x, float* __restrict__ y, long long rows, int cols, int ld) {
  const long long n = rows * cols;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long r = i / cols;
    const int c = (int)(i - r * cols);
    y[i] = ElemIO<T>::ld(x + r * ld + c);
  }
}

// one thread per output pixel-row (frame, pixel): writes c_pad channels
template <typename T>
__global__ void __launch_bounds__(256) unet_input_kernel(const float* __restrict__ lat, const float* __restrict__ mask,
                                                         const float* __restrict__ first, T* __restrict__ x, int B, int F,
                                                         int HW, int CL, int c_pad, int cfg_dup, int mask_frames, int mode) {
  const long long total = (long long)cfg_dup * B * F * HW;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int p = (int)(i % HW);
    const long long bf = i / HW;
    const int f = (int)(bf % F);
    const int b = (int)((bf / F) % B);  // CFG duplicates share the same latents
    T* o = x + i * c_pad;
    for (int c = 0; c < CL; ++c) ElemIO<T>::st(o + c, lat[(((long long)b * CL + c) * F + f) * HW + p]);
    if (mode == 1) {          // use_first_frame_condition_concat: the clean first-frame latents beside the latents of EVERY frame
      for (int c = 0; c < CL; ++c) ElemIO<T>::st(o + CL + c, first ? first[((long long)b * CL + c) * HW + p] : 0.f);
      for (int c = 2 * CL; c < c_pad; ++c) ElemIO<T>::st(o + c, 0.f);
      continue;
    }
    float m;
    if (mask) {
      const int mf = mask_frames > 1 ? f : 0;
      m = fminf(fmaxf(mask[((long long)b * mask_frames + mf) * HW + p], 0.f), 1.f);
    } else {
      m = (f == 0) ? 1.f : 0.f;
    }
    ElemIO<T>::st(o + CL, m);
    for (int c = 0; c < CL; ++c)
      ElemIO<T>::st(o + CL + 1 + c, (f == 0 && first) ? first[((long long)b * CL + c) * HW + p] : 0.f);
    for (int c = 2 * CL + 1; c < c_pad; ++c) ElemIO<T>::st(o + c, 0.f);
  }
}

// fyc_unet_input_scaled: unet_input_kernel with every stored value divided by `denom` (a sigma-space scheduler's scale_model_input,
// sqrt(sigma^2 + 1)): a true f32 division, as the reference divides, rounded once more to the storage type.  scale_cond: the mask channel
// and the first-frame block of mode 0 are divided as well (the reference scales the concatenated tensor); mode 1 divides the latents only.
template <typename T>
__global__ void __launch_bounds__(256) unet_input_scaled_kernel(const float* __restrict__ lat, const float* __restrict__ mask,
                                                                const float* __restrict__ first, T* __restrict__ x, int B, int F,
                                                                int HW, int CL, int c_pad, int cfg_dup, int mask_frames, int mode,
                                                                float denom, int scale_cond) {
  const long long total = (long long)cfg_dup * B * F * HW;
  const float cden = scale_cond ? denom : 1.f;                // (v / 1.f is v: the unscaled channels keep their bits)
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int p = (int)(i % HW);
    const long long bf = i / HW;
    const int f = (int)(bf % F);
    const int b = (int)((bf / F) % B);  // CFG duplicates share the same latents
    T* o = x + i * c_pad;
    for (int c = 0; c < CL; ++c) ElemIO<T>::st(o + c, lat[(((long long)b * CL + c) * F + f) * HW + p] / denom);
    if (mode == 1) {
      for (int c = 0; c < CL; ++c) ElemIO<T>::st(o + CL + c, first ? first[((long long)b * CL + c) * HW + p] : 0.f);
      for (int c = 2 * CL; c < c_pad; ++c) ElemIO<T>::st(o + c, 0.f);
      continue;
    }
    float m;
    if (mask) {
      const int mf = mask_frames > 1 ? f : 0;
      m = fminf(fmaxf(mask[((long long)b * mask_frames + mf) * HW + p], 0.f), 1.f);
    } else {
      m = (f == 0) ? 1.f : 0.f;
    }
    ElemIO<T>::st(o + CL, m / cden);
    for (int c = 0; c < CL; ++c)
      ElemIO<T>::st(o + CL + 1 + c, (f == 0 && first) ? first[((long long)b * CL + c) * HW + p] / cden : 0.f);
    for (int c = 2 * CL + 1; c < c_pad; ++c) ElemIO<T>::st(o + c, 0.f);
  }
}

// the guided prediction of one element from the unconditional, conditional and (optional) per-frame unconditional one: the one f32
// expression of the step kernels and of the moments pass of the guidance rescale
__device__ __forceinline__ float cfg_guided(float u, float cnd, bool has_single, float s1, float video_scale, float guidance) {
  if (has_single) return s1 + video_scale * (u - s1) + guidance * (cnd - u);
  return u + guidance * (cnd - u);
}

// the guided prediction of channel c of one pixel-row, as every step kernel forms it: the plain prediction without cfg; with it
// cfg_guided() of the two halves (and the per-frame row, single_row != NULL).  RESCALE: times factor_b, the sample's guidance-rescale factor
template <typename T, bool RESCALE>
__device__ __forceinline__ float guided_value(const T* pu, const T* pc, const T* single_row, int c, float guidance, float video_scale, int cfg,
                                              float factor_b) {
  float v = ElemIO<T>::ld(pu + c);
  if (cfg) {
    const float u = v, cnd = ElemIO<T>::ld(pc + c);
    v = cfg_guided(u, cnd, single_row != nullptr, single_row ? ElemIO<T>::ld(single_row + c) : 0.f, video_scale, guidance);
    if (RESCALE) v *= factor_b;
  }
  return v;
}

// pixel-row i = (b, f, p) of the channels-last prediction, and where its channel c lies in the (B, CL, F, HW) latents
struct PixelRow {
  int b, f, p;
  __device__ __forceinline__ PixelRow(long long i, int F, int HW) : p((int)(i % HW)) {
    const long long bf = i / HW;
    f = (int)(bf % F);
    b = (int)(bf / F);
  }
  __device__ __forceinline__ long long latent(int c, int CL, int F, int HW) const { return (((long long)b * CL + c) * F + f) * HW + p; }
};

// guidance + DDIM update of pixel-row i = (b, f, p): the body of the DDIM step kernel.  RESCALE: the guided prediction of sample b is
// multiplied by factor[b] (guidance rescale, fyc_cfg_ddim_step_rescaled) before anything else sees it
template <typename T, bool RESCALE>
__device__ __forceinline__ void cfg_ddim_row(long long i, const T* __restrict__ pred, float* __restrict__ lat, float sa, float sb,
                                             float sap, float sbp, int B, int F, int HW, int CL, int ld, int cfg, float guidance,
                                             int pred_type, int clip, const T* __restrict__ single, float video_scale,
                                             const float* __restrict__ noise, float sigma, int reclip,
                                             const float* __restrict__ factor) {
  const PixelRow r(i, F, HW);
  const T* pu = pred + i * ld;                                   // uncond (or the only) half
  const T* pc = pred + ((long long)B * F * HW + i) * ld;         // cond half
  const T* ps = single ? single + i * ld : nullptr;
  for (int c = 0; c < CL; ++c) {
    const float v = guided_value<T, RESCALE>(pu, pc, ps, c, guidance, video_scale, cfg, RESCALE ? factor[r.b] : 0.f);
    const long long j = r.latent(c, CL, F, HW);
    const float x = lat[j];
    float x0, eps;
    if (pred_type == 1) { x0 = sa * x - sb * v; eps = sa * v + sb * x; }
    else if (pred_type == 0) { x0 = (x - sb * v) / sa; eps = v; }
    else { x0 = v; eps = v; }
    if (clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
    if (reclip) eps = (x - sa * x0) / sb;                        // use_clipped_model_output (scheduling_ddim.py:342-344)
    float nx = sap * x0 + sbp * eps;
    if (noise) nx += sigma * noise[j];                           // eta > 0 (:346-363)
    lat[j] = nx;
  }
}

// fyc_cfg_ddim_step (RESCALE = false, factor = NULL) and fyc_cfg_ddim_step_rescaled (cfg is on: the host refuses the rest)
template <typename T, bool RESCALE>
__global__ void __launch_bounds__(256) cfg_ddim_kernel(const T* __restrict__ pred, float* __restrict__ lat,
                                                       const float* __restrict__ coef, int B, int F, int HW, int CL, int ld,
                                                       int cfg, float guidance, int pred_type, int clip,
                                                       const T* __restrict__ single, float video_scale,
                                                       const float* __restrict__ noise, float sigma, int reclip,
                                                       const float* __restrict__ factor) {
  const float sa = coef[0], sb = coef[1], sap = coef[2], sbp = coef[3];
  const long long total = (long long)B * F * HW;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256)
    cfg_ddim_row<T, RESCALE>(i, pred, lat, sa, sb, sap, sbp, B, F, HW, CL, ld, cfg, guidance, pred_type, clip, single, video_scale, noise,
                             sigma, reclip, factor);
}

// the optional buffers of a linear step, all (B, CL, F, HW) f32; NULL = not read / not written (one uniform branch each).  acc_in may be
// acc_out (element j is read and then written by the same thread), so nothing here is __restrict__
struct StepBuffers {
  const float* sample_in; float* sample_out;
  float* hist_out; const float* hist[3];
  const float* noise;
  const float* acc_in; float* acc_out;
};

// Guidance + one step of every sampler whose update is linear in the latents, the guided prediction and stored ones: the DPM-Solver
// multistep family (fyc_cfg_solver_step), the sigma-space samplers Euler, Euler ancestral and LMS (fyc_cfg_sigma_step) and PNDM in its
// PLMS and Runge-Kutta modes (fyc_cfg_pndm_step).  With v the guided (and rescaled) prediction and x the saved sample (sample_in) when one
// is handed over, the latents otherwise:
//   CONVERT:  coef = {a_x, a_v, row},  m = a_x x + a_v v   (the converted output m0 of the solver, the derivative d of the sigma samplers)
//   else:     coef = row,              m = v               (PNDM: the v-prediction conversion is folded into the row)
//   row = {c_x, c_0, c_1, c_2, c_3, tail}:  x' = c_x x + c_0 m + c_1 hist[0] + c_2 hist[1] + c_3 hist[2] + tail noise,  summed left to right
// ORDER is a template parameter so that a history the order does not use is never loaded: 0 * NaN is NaN, and the first step's history
// is whatever the allocator left.  Stores: the latents <- x';  sample_out <- the latents as they were (with sample_in and no sample_out
// the latents are not read);  hist_out <- m;  acc_out <- acc_in + tail m (acc_in NULL: tail m).  tail is c_n where there is noise, s_g
// where there is an accumulator, padding otherwise.
template <typename T, int ORDER, bool CONVERT, bool RESCALE>
__global__ void __launch_bounds__(256) cfg_linear_step_kernel(const T* __restrict__ pred, float* __restrict__ lat,
                                                              const float* __restrict__ coef, int B, int F, int HW, int CL, int ld,
                                                              int cfg, float guidance, const T* __restrict__ single, float video_scale,
                                                              StepBuffers buf, const float* __restrict__ factor) {
  const float ax = CONVERT ? coef[0] : 0.f, av = CONVERT ? coef[1] : 0.f;
  const float* row = coef + (CONVERT ? 2 : 0);
  const float cx = row[0], c0 = row[1], c1 = row[2], c2 = row[3], c3 = row[4], tail = row[5];
  const long long total = (long long)B * F * HW;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const PixelRow r(i, F, HW);
    const T* pu = pred + i * ld;                                   // uncond (or the only) half
    const T* pc = pred + ((long long)B * F * HW + i) * ld;         // cond half
    const T* ps = single ? single + i * ld : nullptr;
    for (int c = 0; c < CL; ++c) {
      const float v = guided_value<T, RESCALE>(pu, pc, ps, c, guidance, video_scale, cfg, RESCALE ? factor[r.b] : 0.f);
      const long long j = r.latent(c, CL, F, HW);
      const float before = (buf.sample_out || !buf.sample_in) ? lat[j] : 0.f;
      if (buf.sample_out) buf.sample_out[j] = before;
      const float x = buf.sample_in ? buf.sample_in[j] : before;
      const float m = CONVERT ? ax * x + av * v : v;
      float nx = cx * x + c0 * m;
      if (ORDER >= 2) nx += c1 * buf.hist[0][j];
      if (ORDER >= 3) nx += c2 * buf.hist[1][j];
      if (ORDER >= 4) nx += c3 * buf.hist[2][j];
      if (buf.noise) nx += tail * buf.noise[j];
      lat[j] = nx;
      if (buf.hist_out) buf.hist_out[j] = m;
      if (buf.acc_out) buf.acc_out[j] = (buf.acc_in ? buf.acc_in[j] : 0.f) + tail * m;
    }
  }
}

// Moments pass of the guidance rescale.  Block (b, part) owns rows [part * CFG_MOMENT_ROWS, +CFG_MOMENT_ROWS) of the F * HW pixel-rows
// of sample b - a run fixed by the shape; thread t takes rows t, t + 256, ... of the run.  c and v are the f32 values the step kernel
// forms; {sum c, sum c^2, sum v, sum v^2} are accumulated in f64 (the squares of f32 values are exact there), reduced over the block by a
// fixed tree in LDS and written as one partial [4] per block: no atomics, the same bits every time.
// VEC: c_latent == 4 and rows that start on a 4-element boundary - one 8-byte (16-bit) or 16-byte (f32) load per row and half
constexpr int CFG_MOMENT_ROWS = 1024;
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) cfg_moments_kernel(const T* __restrict__ pred, double* __restrict__ parts, int B, int rows, int CL,
                                                          int ld, int nparts, float guidance, const T* __restrict__ single,
                                                          float video_scale) {
  __shared__ double red[4][256];
  const int b = blockIdx.x / nparts, part = blockIdx.x - b * nparts, t = threadIdx.x;
  const int r_end = min(rows, (part + 1) * CFG_MOMENT_ROWS);
  double sc = 0.0, scc = 0.0, sv = 0.0, svv = 0.0;
  for (int r = part * CFG_MOMENT_ROWS + t; r < r_end; r += 256) {
    const long long i = (long long)b * rows + r;
    const T* pu = pred + i * ld;
    const T* pc = pred + ((long long)B * rows + i) * ld;
    const T* ps = single ? single + i * ld : nullptr;
    if (VEC) {
      float u[4], cn[4], s1[4] = {0.f, 0.f, 0.f, 0.f};
      ElemIO<T>::ld4(pu, u);
      ElemIO<T>::ld4(pc, cn);
      if (ps) ElemIO<T>::ld4(ps, s1);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double cd = (double)cn[c], vd = (double)cfg_guided(u[c], cn[c], ps != nullptr, s1[c], video_scale, guidance);
        sc += cd; scc += cd * cd; sv += vd; svv += vd * vd;
      }
    } else {
      for (int c = 0; c < CL; ++c) {
        const float cn = ElemIO<T>::ld(pc + c);
        const double cd = (double)cn;
        const double vd = (double)cfg_guided(ElemIO<T>::ld(pu + c), cn, ps != nullptr, ps ? ElemIO<T>::ld(ps + c) : 0.f, video_scale, guidance);
        sc += cd; scc += cd * cd; sv += vd; svv += vd * vd;
      }
    }
  }
  red[0][t] = sc; red[1][t] = scc; red[2][t] = sv; red[3][t] = svv;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int k = 0; k < 4; ++k) red[k][t] += red[k][t + s];
    }
    __syncthreads();
  }
  if (t < 4) parts[(long long)blockIdx.x * 4 + t] = red[t][0];
}

// One block per sample: the partials of the sample folded in index order, the factor  phi * s_text / s_cfg + (1 - phi)  formed in f64 from
// the unbiased variances and rounded once to f32.  A constant guided prediction (s_cfg = 0) keeps the factor 1.
__global__ void __launch_bounds__(64) cfg_rescale_factor_kernel(const double* __restrict__ parts, float* __restrict__ factor, int nparts,
                                                                double n, float phi) {
  __shared__ double sh[64][4];
  const double* p = parts + (long long)blockIdx.x * nparts * 4;
  double sc = 0.0, scc = 0.0, sv = 0.0, svv = 0.0;
  // 64 partials at a time: every lane fetches one (the loads overlap), lane 0 adds them in index order
  for (int k0 = 0; k0 < nparts; k0 += 64) {
    const int k = k0 + threadIdx.x;
    if (k < nparts) {
#pragma unroll
      for (int j = 0; j < 4; ++j) sh[threadIdx.x][j] = p[4 * k + j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = min(64, nparts - k0);
      for (int i = 0; i < m; ++i) { sc += sh[i][0]; scc += sh[i][1]; sv += sh[i][2]; svv += sh[i][3]; }
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double var_c = fmax(scc - sc * sc / n, 0.0) / (n - 1.0), var_v = fmax(svv - sv * sv / n, 0.0) / (n - 1.0);
  const double ph = (double)phi;
  factor[blockIdx.x] = var_v > 0.0 ? (float)(ph * (sqrt(var_c) / sqrt(var_v)) + (1.0 - ph)) : 1.f;
}

template <typename T>
__global__ void __launch_bounds__(256) nchw_to_nhwc_kernel(const float* __restrict__ z, T* __restrict__ x, int N, int C, int HW,
                                                           int c_pad, float scale) {
  const long long total = (long long)N * HW;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int p = (int)(i % HW);
    const long long n = i / HW;
    T* o = x + i * c_pad;
    for (int c = 0; c < C; ++c) ElemIO<T>::st(o + c, z[(n * C + c) * HW + p] * scale);
    for (int c = C; c < c_pad; ++c) ElemIO<T>::st(o + c, 0.f);
  }
}

template <typename T>
__global__ void __launch_bounds__(256) nhwc_to_nchw_kernel(const T* __restrict__ x, float* __restrict__ y, int N, int C, int HW,
                                                           int ld, float mul, float add, float lo, float hi) {
  const long long total = (long long)N * C * HW;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int p = (int)(i % HW);
    const long long nc = i / HW;
    const int c = (int)(nc % C);
    const long long n = nc / C;
    const float v = ElemIO<T>::ld(x + (n * HW + p) * ld + c) * mul + add;
    y[i] = fminf(fmaxf(v, lo), hi);
  }
}

// (O, I, 3, 3) f32 -> [O][slab][tap][c in slab] (see include/fyc.h): one thread per output element
template <typename T>
__global__ void __launch_bounds__(256) pack_conv3x3_kernel(const float* __restrict__ w, T* __restrict__ out, int O, int I, int Ip, int slab) {
  const long long total = (long long)O * 9 * Ip;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int k = (int)(i % (9 * Ip));
    const long long o = i / (9 * Ip);
    const int sl = k / (9 * slab), r = k - sl * 9 * slab, tap = r / slab, c = sl * slab + (r - tap * slab);
    ElemIO<T>::st(out + i, c < I ? w[(o * I + c) * 9 + tap] : 0.f);
  }
}

// value rows [0, O/2) and gate rows [O/2, O) interleaved in blocks of 16 (weight and bias)
template <typename T>
__global__ void __launch_bounds__(256) pack_geglu_kernel(const float* __restrict__ w, const float* __restrict__ b, T* __restrict__ wo,
                                                         float* __restrict__ bo, int O, int I) {
  const long long total = (long long)O * I;
  const int half = O / 2;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int col = (int)(i % I), row = (int)(i / I);
    const int blk = row >> 5, in = row & 31;
    const int src = (in < 16) ? blk * 16 + in : half + blk * 16 + (in - 16);
    ElemIO<T>::st(wo + i, w[(long long)src * I + col]);
    if (col == 0 && b != nullptr) bo[row] = b[src];
  }
}

inline int grid_for(long long n) {
  long long b = ceil_div64(n, 256);
  return (int)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}


// out[r][c8..] = table[ids[r]][c8..] + pos[r % seq][c8..]: one thread per 8 channels
template <typename T>
__global__ void __launch_bounds__(256) embed_tokens_kernel(const long long* __restrict__ ids, const float* __restrict__ table,
                                                           const float* __restrict__ pos, T* __restrict__ out, long long rows,
                                                           int seq, int C, int vocab) {
  const int C8 = C >> 3;
  const long long total = rows * C8;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long r = i / C8;
    const int c = (int)(i - r * C8) * 8;
    long long id = ids[r];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);   // host validates ids; clamp keeps a bad id from reading out of bounds
    const float* t = table + id * C + c;
    const float* pp = pos + (long long)(r % seq) * C + c;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = t[e] + pp[e];
    store8<T>(out + r * C + c, v);
  }
}

// one thread per output element; reads are P-contiguous runs of the image rows
template <typename T>
__global__ void __launch_bounds__(256) patchify_kernel(const float* __restrict__ img, T* __restrict__ out, int B, int Cin, int H,
                                                       int W, int P, int ld) {
  const int gh = H / P, gw = W / P, K = Cin * P * P;
  const long long total = (long long)B * gh * gw * ld;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int k = (int)(i % ld);
    const long long patch = i / ld;
    float v = 0.f;
    if (k < K) {
      const int px = k % P, py = (k / P) % P, c = k / (P * P);
      const int gx = (int)(patch % gw), gy = (int)((patch / gw) % gh), b = (int)(patch / ((long long)gw * gh));
      v = img[(((long long)b * Cin + c) * H + gy * P + py) * W + gx * P + px];
    }
    ElemIO<T>::st(out + i, v);
  }
}

}  // namespace

#define FYC_DT(a, call_bf16, call_f16, call_f32)               \
  do {                                                         \
    if ((a)->dtype == FYC_BF16) { call_bf16; }                 \
    else if ((a)->dtype == FYC_F16) { call_f16; }              \
    else if ((a)->dtype == FYC_F32) { call_f32; }              \
    else FYC_FAIL(-2, "bad dtype %d", (a)->dtype);             \
  } while (0)

extern "C" int fyc_concat_channels(const fyc_concat_args* a, void* stream) {
  FYC_REQUIRE(a && a->a && a->b && a->y, "fyc_concat_channels: null pointer");
  FYC_REQUIRE(a->c1 % 8 == 0 && a->c2 % 8 == 0 && a->rows > 0, "fyc_concat_channels: channels must be multiples of 8");
  hipStream_t st = (hipStream_t)stream;
  const long long chunks = a->rows * ((a->c1 + a->c2) / 8);
  FYC_DT(a,
         hipLaunchKernelGGL(concat_kernel<bf16_t>, dim3(grid_for(chunks)), dim3(256), 0, st, (const bf16_t*)a->a, (const bf16_t*)a->b, (bf16_t*)a->y, chunks, a->c1 / 8, a->c2 / 8),
         hipLaunchKernelGGL(concat_kernel<f16_t>, dim3(grid_for(chunks)), dim3(256), 0, st, (const f16_t*)a->a, (const f16_t*)a->b, (f16_t*)a->y, chunks, a->c1 / 8, a->c2 / 8),
         hipLaunchKernelGGL(concat_kernel<float>, dim3(grid_for(chunks)), dim3(256), 0, st, (const float*)a->a, (const float*)a->b, (float*)a->y, chunks, a->c1 / 8, a->c2 / 8));
  FYC_CHECK_LAUNCH("fyc_concat_channels");
  return 0;
}

extern "C" int fyc_repeat(const fyc_repeat_args* a, void* stream) {
  FYC_REQUIRE(a && a->src && a->dst, "fyc_repeat: null pointer");
  FYC_REQUIRE(a->bytes > 0 && a->bytes % 16 == 0 && a->times >= 1, "fyc_repeat: bytes %lld (multiple of 16), times %d", (long long)a->bytes, a->times);
  FYC_REQUIRE((((uintptr_t)a->src | (uintptr_t)a->dst) & 15) == 0, "fyc_repeat: src / dst must be 16-byte aligned");
  const char* s = (const char*)a->src;
  const char* d = (const char*)a->dst;
  FYC_REQUIRE(s + a->bytes <= d || d + a->bytes * a->times <= s, "fyc_repeat: src and dst overlap");
  const long long chunks = a->bytes / 16;
  hipLaunchKernelGGL(repeat_kernel, dim3(grid_for(chunks)), dim3(256), 0, (hipStream_t)stream, (const u32x4*)a->src, (u32x4*)a->dst, chunks, (int)a->times);
  FYC_CHECK_LAUNCH("fyc_repeat");
  return 0;
}

extern "C" int fyc_silu_f32(const fyc_silu_args* a, void* stream) {
  FYC_REQUIRE(a && a->x && a->y && a->n > 0, "fyc_silu_f32: bad args");
  hipLaunchKernelGGL(silu_kernel, dim3(grid_for(a->n)), dim3(256), 0, (hipStream_t)stream, a->x, a->y, (long long)a->n);
  FYC_CHECK_LAUNCH("fyc_silu_f32");
  return 0;
}

extern "C" int fyc_cast_from_f32(const fyc_cast_args* a, void* stream) {
  FYC_REQUIRE(a && a->x && a->y && a->rows > 0 && a->cols > 0 && a->ld >= a->cols, "fyc_cast_from_f32: bad args");
  hipStream_t st = (hipStream_t)stream;
  const long long n = a->rows * a->ld;
  FYC_DT(a,
         hipLaunchKernelGGL(cast_from_kernel<bf16_t>, dim3(grid_for(n)), dim3(256), 0, st, a->x, (bf16_t*)a->y, (long long)a->rows, a->cols, a->ld),
         hipLaunchKernelGGL(cast_from_kernel<f16_t>, dim3(grid_for(n)), dim3(256), 0, st, a->x, (f16_t*)a->y, (long long)a->rows, a->cols, a->ld),
         hipLaunchKernelGGL(cast_from_kernel<float>, dim3(grid_for(n)), dim3(256), 0, st, a->x, (float*)a->y, (long long)a->rows, a->cols, a->ld));
  FYC_CHECK_LAUNCH("fyc_cast_from_f32");
  return 0;
}

extern "C" int fyc_cast_to_f32(const fyc_cast_to_args* a, void* stream) {
  FYC_REQUIRE(a && a->x && a->y && a->rows > 0 && a->cols > 0 && a->ld >= a->cols, "fyc_cast_to_f32: bad args");
  hipStream_t st = (hipStream_t)stream;
  const long long n = a->rows * a->cols;
  FYC_DT(a,
         hipLaunchKernelGGL(cast_to_kernel<bf16_t>, dim3(grid_for(n)), dim3(256), 0, st, (const bf16_t*)a->x, a->y, (long long)a->rows, a->cols, a->ld),
         hipLaunchKernelGGL(cast_to_kernel<f16_t>, dim3(grid_for(n)), dim3(256), 0, st, (const f16_t*)a->x, a->y, (long long)a->rows, a->cols, a->ld),
         hipLaunchKernelGGL(cast_to_kernel<float>, dim3(grid_for(n)), dim3(256), 0, st, (const float*)a->x, a->y, (long long)a->rows, a->cols, a->ld));
  FYC_CHECK_LAUNCH("fyc_cast_to_f32");
  return 0;
}

extern "C" int fyc_unet_input(const fyc_unet_input_args* a, void* stream) {
  FYC_REQUIRE(a && a->latents && a->x, "fyc_unet_input: null pointer");
  FYC_REQUIRE(a->B > 0 && a->F > 0 && a->HW > 0 && a->c_latent > 0 && a->c_pad >= 2 * a->c_latent + (a->mode == 1 ? 0 : 1), "fyc_unet_input: bad dims");
  FYC_REQUIRE(a->mode == 0 || a->mode == 1, "fyc_unet_input: mode %d", a->mode);
  FYC_REQUIRE(a->cfg_dup == 1 || a->cfg_dup == 2, "fyc_unet_input: cfg_dup must be 1 or 2");
  FYC_REQUIRE(a->mask == nullptr || a->mask_frames == 1 || a->mask_frames == a->F, "fyc_unet_input: mask_frames must be 1 or F");
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)a->cfg_dup * a->B * a->F * a->HW;
  const int mf = a->mask ? a->mask_frames : 1;
  FYC_DT(a,
         hipLaunchKernelGGL(unet_input_kernel<bf16_t>, dim3(grid_for(n)), dim3(256), 0, st, a->latents, a->mask, a->first, (bf16_t*)a->x, a->B, a->F, a->HW, a->c_latent, a->c_pad, a->cfg_dup, mf, a->mode),
         hipLaunchKernelGGL(unet_input_kernel<f16_t>, dim3(grid_for(n)), dim3(256), 0, st, a->latents, a->mask, a->first, (f16_t*)a->x, a->B, a->F, a->HW, a->c_latent, a->c_pad, a->cfg_dup, mf, a->mode),
         hipLaunchKernelGGL(unet_input_kernel<float>, dim3(grid_for(n)), dim3(256), 0, st, a->latents, a->mask, a->first, (float*)a->x, a->B, a->F, a->HW, a->c_latent, a->c_pad, a->cfg_dup, mf, a->mode));
  FYC_CHECK_LAUNCH("fyc_unet_input");
  return 0;
}

extern "C" int fyc_unet_input_scaled(const fyc_unet_input_scaled_args* s, void* stream) {
  FYC_REQUIRE(s, "fyc_unet_input_scaled: null pointer");
  const fyc_unet_input_args* a = &s->base;
  FYC_REQUIRE(a->latents && a->x, "fyc_unet_input_scaled: null pointer");
  FYC_REQUIRE(a->mode == 0 || a->mode == 1, "fyc_unet_input_scaled: mode %d", a->mode);
  FYC_REQUIRE(a->B > 0 && a->F > 0 && a->HW > 0 && a->c_latent > 0 && a->c_pad >= 2 * a->c_latent + (a->mode == 1 ? 0 : 1), "fyc_unet_input_scaled: bad dims");
  FYC_REQUIRE(a->cfg_dup == 1 || a->cfg_dup == 2, "fyc_unet_input_scaled: cfg_dup must be 1 or 2");
  FYC_REQUIRE(a->mask == nullptr || a->mask_frames == 1 || a->mask_frames == a->F, "fyc_unet_input_scaled: mask_frames must be 1 or F");
  FYC_REQUIRE(a->dtype == FYC_BF16 || a->dtype == FYC_F16 || a->dtype == FYC_F32, "fyc_unet_input_scaled: bad dtype %d", a->dtype);
  FYC_REQUIRE(s->denom >= 1.f && s->denom <= 3.0e38f, "fyc_unet_input_scaled: denom %g must be finite and at least 1 (sqrt(sigma^2 + 1))", (double)s->denom);
  FYC_REQUIRE(s->scale_cond == 0 || s->scale_cond == 1, "fyc_unet_input_scaled: scale_cond %d", s->scale_cond);
  FYC_REQUIRE(a->mode == 0 || s->scale_cond == 0, "fyc_unet_input_scaled: scale_cond must be 0 in mode 1 (the UNet concatenates the clean first-frame latents behind the scaling)");
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)a->cfg_dup * a->B * a->F * a->HW;
  const int mf = a->mask ? a->mask_frames : 1;
  if (a->dtype == FYC_BF16) hipLaunchKernelGGL(unet_input_scaled_kernel<bf16_t>, dim3(grid_for(n)), dim3(256), 0, st, a->latents, a->mask, a->first, (bf16_t*)a->x, a->B, a->F, a->HW, a->c_latent, a->c_pad, a->cfg_dup, mf, a->mode, s->denom, s->scale_cond);
  else if (a->dtype == FYC_F16) hipLaunchKernelGGL(unet_input_scaled_kernel<f16_t>, dim3(grid_for(n)), dim3(256), 0, st, a->latents, a->mask, a->first, (f16_t*)a->x, a->B, a->F, a->HW, a->c_latent, a->c_pad, a->cfg_dup, mf, a->mode, s->denom, s->scale_cond);
  else hipLaunchKernelGGL(unet_input_scaled_kernel<float>, dim3(grid_for(n)), dim3(256), 0, st, a->latents, a->mask, a->first, (float*)a->x, a->B, a->F, a->HW, a->c_latent, a->c_pad, a->cfg_dup, mf, a->mode, s->denom, s->scale_cond);
  FYC_CHECK_LAUNCH("fyc_unet_input_scaled");
  return 0;
}

// fn(TypeTag<T>{}) for the element type T of a dtype code; false = no such dtype, nothing ran
template <typename T> struct TypeTag { using type = T; };
template <typename Fn>
static bool with_dtype(int dtype, Fn&& fn) {
  if (dtype == FYC_BF16) fn(TypeTag<bf16_t>{});
  else if (dtype == FYC_F16) fn(TypeTag<f16_t>{});
  else if (dtype == FYC_F32) fn(TypeTag<float>{});
  else return false;
  return true;
}

// the guidance operands every cfg step starts from: the leading fields of fyc_cfg_ddim_args, _solver_args, _sigma_args and _pndm_args
struct CfgOperands {
  const void* pred; float* latents; const float* coef;
  int B, F, HW, c_latent, ld, cfg; float guidance;
  int dtype;
  const void* pred_single; float video_scale;
};

template <typename A>
static CfgOperands cfg_operands(const A& a) {
  return {a.pred, a.latents, a.coef, a.B, a.F, a.HW, a.c_latent, a.ld, a.cfg, a.guidance, a.dtype, a.pred_single, a.video_scale};
}

// the argument checks of the DDIM step, shared by its two entry points
static int cfg_ddim_check(const fyc_cfg_ddim_args* a) {
  FYC_REQUIRE(a && a->pred && a->latents && a->coef, "fyc_cfg_ddim_step: null pointer");
  FYC_REQUIRE(a->B > 0 && a->F > 0 && a->HW > 0 && a->c_latent > 0 && a->ld >= a->c_latent, "fyc_cfg_ddim_step: bad dims");
  FYC_REQUIRE(a->pred_type >= 0 && a->pred_type <= 2, "fyc_cfg_ddim_step: pred_type %d", a->pred_type);
  FYC_REQUIRE(a->pred_single == nullptr || a->cfg, "fyc_cfg_ddim_step: pred_single needs classifier-free guidance (cfg = 1)");
  FYC_REQUIRE(a->variance_noise == nullptr || a->sigma >= 0.f, "fyc_cfg_ddim_step: sigma %g", (double)a->sigma);
  return 0;
}

template <typename T, bool RESCALE>
static void cfg_ddim_launch(const fyc_cfg_ddim_args* a, const float* factor, hipStream_t st) {
  const long long n = (long long)a->B * a->F * a->HW;
  hipLaunchKernelGGL((cfg_ddim_kernel<T, RESCALE>), dim3(grid_for(n)), dim3(256), 0, st, (const T*)a->pred, a->latents, a->coef, a->B, a->F,
                     a->HW, a->c_latent, a->ld, a->cfg, a->guidance, a->pred_type, a->clip_sample, (const T*)a->pred_single, a->video_scale,
                     a->variance_noise, a->sigma, a->clipped_model_output, factor);
}

extern "C" int fyc_cfg_ddim_step(const fyc_cfg_ddim_args* a, void* stream) {
  if (int rc = cfg_ddim_check(a)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!with_dtype(a->dtype, [&](auto tag) { cfg_ddim_launch<typename decltype(tag)::type, false>(a, nullptr, st); }))
    FYC_FAIL(-2, "bad dtype %d", a->dtype);
  FYC_CHECK_LAUNCH("fyc_cfg_ddim_step");
  return 0;
}

// ---- guidance rescale: moments pass, factor, step -------------------------------------------------------------------------------
// workspace = [B * nparts][4] f64 partials, then [B] f32 factors
struct CfgRescalePlan { int rows, nparts; int64_t part_bytes, bytes; };

static bool cfg_rescale_plan(int B, int F, int HW, int c_latent, int ld, CfgRescalePlan& pl) {
  if (!(B > 0 && F > 0 && HW > 0 && c_latent > 0 && ld >= c_latent)) return false;
  const int64_t rows = (int64_t)F * HW;
  if (rows > INT32_MAX - CFG_MOMENT_ROWS || rows * c_latent < 2) return false;
  const int64_t nparts = ceil_div64(rows, CFG_MOMENT_ROWS);
  if (nparts * B > INT32_MAX) return false;
  pl.rows = (int)rows;
  pl.nparts = (int)nparts;
  pl.part_bytes = nparts * B * 4 * (int64_t)sizeof(double);
  pl.bytes = (pl.part_bytes + (int64_t)B * (int64_t)sizeof(float) + 255) / 256 * 256;
  return true;
}

// what the four workspace queries answer: 0 without a rescale to do (phi outside (0, 1], NaN included, or no cfg) or for dims the step refuses
static int64_t rescale_workspace_bytes(int B, int F, int HW, int c_latent, int ld, int cfg, float phi) {
  CfgRescalePlan pl;
  return phi > 0.f && phi <= 1.f && cfg && cfg_rescale_plan(B, F, HW, c_latent, ld, pl) ? pl.bytes : 0;
}

extern "C" int64_t fyc_cfg_ddim_rescale_workspace_bytes(const fyc_cfg_ddim_rescale_args* a) {
  return a ? rescale_workspace_bytes(a->step.B, a->step.F, a->step.HW, a->step.c_latent, a->step.ld, a->step.cfg, a->guidance_rescale) : 0;
}

// the moments and factor launches, shared by every step -> the device factors [B] inside the workspace
template <typename T>
static const float* cfg_rescale_factors(const CfgOperands& g, void* workspace, float phi, const CfgRescalePlan& pl, hipStream_t st) {
  double* parts = (double*)workspace;
  float* factor = (float*)((char*)workspace + pl.part_bytes);
  const T* pred = (const T*)g.pred;
  const T* single = (const T*)g.pred_single;
  // one vector load per row: 4 latent channels, rows pitched in multiples of 4 elements from bases on such a boundary
  const uintptr_t row_align = 4 * sizeof(T);
  const bool vec = g.c_latent == 4 && g.ld % 4 == 0 && ((uintptr_t)pred % row_align) == 0 && ((uintptr_t)single % row_align) == 0;
  const dim3 grid((unsigned)(g.B * pl.nparts));
  if (vec) hipLaunchKernelGGL((cfg_moments_kernel<T, true>), grid, dim3(256), 0, st, pred, parts, g.B, pl.rows, g.c_latent, g.ld, pl.nparts, g.guidance, single, g.video_scale);
  else hipLaunchKernelGGL((cfg_moments_kernel<T, false>), grid, dim3(256), 0, st, pred, parts, g.B, pl.rows, g.c_latent, g.ld, pl.nparts, g.guidance, single, g.video_scale);
  hipLaunchKernelGGL(cfg_rescale_factor_kernel, dim3(g.B), dim3(64), 0, st, (const double*)parts, factor, pl.nparts, (double)pl.rows * g.c_latent, phi);
  return factor;
}

// what a positive guidance_rescale asks of cfg, the dims and the workspace, for every entry point that takes one (who: "fyc_cfg_<family>_step",
// whose workspace query is fyc_cfg_<family>_workspace_bytes)
static int cfg_rescale_check(const char* who, const char* query, const CfgOperands& g, float phi, const void* workspace, int64_t workspace_bytes,
                             CfgRescalePlan& pl) {
  FYC_REQUIRE(g.cfg, "%s: guidance_rescale %g needs classifier-free guidance (cfg = 1)", who, (double)phi);
  FYC_REQUIRE(cfg_rescale_plan(g.B, g.F, g.HW, g.c_latent, g.ld, pl), "%s: bad dims (F * HW * c_latent = %lld values per sample: 2 .. 2^31)", who, (long long)g.F * g.HW * g.c_latent);
  FYC_REQUIRE(workspace != nullptr && ((uintptr_t)workspace & 7) == 0, "%s: workspace is null or not 8-byte aligned", who);
  FYC_REQUIRE(workspace_bytes >= pl.bytes, "%s: workspace_bytes %lld < %lld (%s)", who, (long long)workspace_bytes, (long long)pl.bytes, query);
  return 0;
}

extern "C" int fyc_cfg_ddim_step_rescaled(const fyc_cfg_ddim_rescale_args* a, void* stream) {
  FYC_REQUIRE(a, "fyc_cfg_ddim_step_rescaled: null pointer");
  FYC_REQUIRE(a->guidance_rescale >= 0.f && a->guidance_rescale <= 1.f, "fyc_cfg_ddim_step_rescaled: guidance_rescale %g (0 = off .. 1)", (double)a->guidance_rescale);
  if (a->guidance_rescale == 0.f) return fyc_cfg_ddim_step(&a->step, stream);
  const fyc_cfg_ddim_args* s = &a->step;
  FYC_REQUIRE(s->cfg, "fyc_cfg_ddim_step_rescaled: guidance_rescale %g needs classifier-free guidance (cfg = 1)", (double)a->guidance_rescale);
  if (int rc = cfg_ddim_check(s)) return rc;
  FYC_REQUIRE(s->dtype == FYC_BF16 || s->dtype == FYC_F16 || s->dtype == FYC_F32, "fyc_cfg_ddim_step_rescaled: bad dtype %d", s->dtype);
  const CfgOperands g = cfg_operands(*s);
  CfgRescalePlan pl;
  if (int rc = cfg_rescale_check("fyc_cfg_ddim_step_rescaled", "fyc_cfg_ddim_rescale_workspace_bytes", g, a->guidance_rescale, a->workspace, a->workspace_bytes, pl)) return rc;
  FYC_REQUIRE(g_fyc_zero_page != nullptr, "fyc_cfg_ddim_step_rescaled: fyc_init() not called");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(s->dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    cfg_ddim_launch<T, true>(s, cfg_rescale_factors<T>(g, a->workspace, a->guidance_rescale, pl, st), st);
  });
  FYC_CHECK_LAUNCH("fyc_cfg_ddim_step_rescaled");
  return 0;
}

// ---- the linear steps (DPM-Solver multistep, sigma-space, PNDM): one host path for fyc_cfg_solver_step / _sigma_step / _pndm_step -----------
// one call of cfg_linear_step_kernel as an entry point describes it
struct StepCall {
  CfgOperands g;
  StepBuffers buf;
  int order, max_order;           // the histories read are hist[0 .. order - 2]
  bool convert;                   // coef starts with {a_x, a_v} (the kernel's CONVERT)
  bool needs_init;                // fyc_init() is asked for without a guidance rescale too
  float guidance_rescale; void* workspace; int64_t workspace_bytes;
  const char* who;                // the entry point, in front of every message
  const char* query;              // its workspace query, named where the workspace is short
};

// the fields the three argument structs share by name; the entry point adds its buffers
template <typename A>
static StepCall step_call(const A& a, int max_order, bool convert, bool needs_init, const char* who, const char* query) {
  return {cfg_operands(a), {}, a.order, max_order, convert, needs_init, a.guidance_rescale, a.workspace, a.workspace_bytes, who, query};
}

// pointers, dims, dtype, order, the histories the order reads, pred_single, the rescale and its workspace; pl is set with a positive rescale
static int step_check(const StepCall& c, CfgRescalePlan& pl) {
  const CfgOperands& g = c.g;
  FYC_REQUIRE(g.pred && g.latents && g.coef, "%s: null pointer", c.who);
  FYC_REQUIRE(g.B > 0 && g.F > 0 && g.HW > 0 && g.c_latent > 0 && g.ld >= g.c_latent, "%s: bad dims", c.who);
  FYC_REQUIRE(g.dtype == FYC_BF16 || g.dtype == FYC_F16 || g.dtype == FYC_F32, "%s: bad dtype %d", c.who, g.dtype);
  FYC_REQUIRE(c.order >= 1 && c.order <= c.max_order, "%s: order %d (1 .. %d)", c.who, c.order, c.max_order);
  for (int k = 1; k < c.order; ++k) FYC_REQUIRE(c.buf.hist[k - 1] != nullptr, "%s: order %d needs hist_%d", c.who, c.order, k);
  FYC_REQUIRE(g.pred_single == nullptr || g.cfg, "%s: pred_single needs classifier-free guidance (cfg = 1)", c.who);
  FYC_REQUIRE(c.guidance_rescale >= 0.f && c.guidance_rescale <= 1.f, "%s: guidance_rescale %g (0 = off .. 1)", c.who, (double)c.guidance_rescale);
  if (c.guidance_rescale > 0.f) return cfg_rescale_check(c.who, c.query, g, c.guidance_rescale, c.workspace, c.workspace_bytes, pl);
  return 0;
}

// The latents and the outputs are written while other threads still read the inputs: any overlap of the [n] f32 ranges is refused, not only
// equal bases.  Every row must be disjoint from every column and from the rows after it; NULL overlaps nothing.  The one alias allowed is
// acc_out == acc_in (element j is read, then written, by the same thread).
struct NamedBuffer { const char* name; const float* p; };
static const char kAccIn[] = "acc_in", kAccOut[] = "acc_out";

template <int n_rows, int n_cols>
static int step_overlap_check(const StepCall& c, const NamedBuffer (&rows)[n_rows], const NamedBuffer (&cols)[n_cols]) {
  const int64_t n = (int64_t)c.g.B * c.g.c_latent * c.g.F * c.g.HW;
  auto overlaps = [n](const float* p, const float* q) { return p != nullptr && q != nullptr && p < q + n && q < p + n; };
  for (int o = 0; o < n_rows; ++o) {
    for (int k = 0; k < n_cols; ++k) {
      if (rows[o].name == kAccOut && cols[k].name == kAccIn && rows[o].p == cols[k].p) continue;
      FYC_REQUIRE(!overlaps(rows[o].p, cols[k].p), "%s: %s aliases %s", c.who, rows[o].name, cols[k].name);
    }
    for (int k = o + 1; k < n_rows; ++k) FYC_REQUIRE(!overlaps(rows[o].p, rows[k].p), "%s: %s aliases %s", c.who, rows[o].name, rows[k].name);
  }
  return 0;
}

template <typename T, bool CONVERT, bool RESCALE>
static void step_launch_order(const StepCall& c, const float* factor, hipStream_t st) {
  const CfgOperands& g = c.g;
  const dim3 grid(grid_for((long long)g.B * g.F * g.HW));
  auto go = [&](auto order) {
    hipLaunchKernelGGL((cfg_linear_step_kernel<T, decltype(order)::value, CONVERT, RESCALE>), grid, dim3(256), 0, st, (const T*)g.pred, g.latents,
                       g.coef, g.B, g.F, g.HW, g.c_latent, g.ld, g.cfg, g.guidance, (const T*)g.pred_single, g.video_scale, c.buf, factor);
  };
  if (c.order == 1) go(std::integral_constant<int, 1>{});
  else if (c.order == 2) go(std::integral_constant<int, 2>{});
  else if (c.order == 3) go(std::integral_constant<int, 3>{});
  else go(std::integral_constant<int, 4>{});
}

// the rescale factors if asked for (pl is the plan step_check made), then the step
static int step_launch(const StepCall& c, const CfgRescalePlan& pl, void* stream) {
  const bool rescale = c.guidance_rescale > 0.f;
  FYC_REQUIRE(!(rescale || c.needs_init) || g_fyc_zero_page != nullptr, "%s: fyc_init() not called", c.who);
  hipStream_t st = (hipStream_t)stream;
  with_dtype(c.g.dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (rescale) {
      const float* factor = cfg_rescale_factors<T>(c.g, c.workspace, c.guidance_rescale, pl, st);
      c.convert ? step_launch_order<T, true, true>(c, factor, st) : step_launch_order<T, false, true>(c, factor, st);
    } else {
      c.convert ? step_launch_order<T, true, false>(c, nullptr, st) : step_launch_order<T, false, false>(c, nullptr, st);
    }
  });
  FYC_CHECK_LAUNCH(c.who);
  return 0;
}

template <typename A>
static int64_t step_workspace_bytes(const A* a) {
  return a ? rescale_workspace_bytes(a->B, a->F, a->HW, a->c_latent, a->ld, a->cfg, a->guidance_rescale) : 0;
}

extern "C" int64_t fyc_cfg_solver_workspace_bytes(const fyc_cfg_solver_args* a) { return step_workspace_bytes(a); }
extern "C" int64_t fyc_cfg_sigma_workspace_bytes(const fyc_cfg_sigma_args* a) { return step_workspace_bytes(a); }
extern "C" int64_t fyc_cfg_pndm_workspace_bytes(const fyc_cfg_pndm_args* a) { return step_workspace_bytes(a); }

// DPM-Solver multistep: m0 = a_x x + a_v v is always stored; fyc_init() only for the guidance rescale
extern "C" int fyc_cfg_solver_step(const fyc_cfg_solver_args* a, void* stream) {
  FYC_REQUIRE(a && a->hist_out, "fyc_cfg_solver_step: null pointer");
  StepCall c = step_call(*a, 3, true, false, "fyc_cfg_solver_step", "fyc_cfg_solver_workspace_bytes");
  c.buf.hist_out = a->hist_out; c.buf.hist[0] = a->hist_1; c.buf.hist[1] = a->hist_2;
  const NamedBuffer rows[] = {{"hist_out", a->hist_out}};
  const NamedBuffer cols[] = {{"latents", a->latents}, {"hist_1", a->hist_1}, {"hist_2", a->hist_2}};
  CfgRescalePlan pl;
  if (int rc = step_check(c, pl)) return rc;
  if (int rc = step_overlap_check(c, rows, cols)) return rc;
  return step_launch(c, pl, stream);
}

// sigma-space samplers (Euler, Euler ancestral, LMS): the derivative d = a_x x + a_v v, optionally stored, and optional noise
extern "C" int fyc_cfg_sigma_step(const fyc_cfg_sigma_args* a, void* stream) {
  FYC_REQUIRE(a, "fyc_cfg_sigma_step: null pointer");
  StepCall c = step_call(*a, 4, true, true, "fyc_cfg_sigma_step", "fyc_cfg_sigma_workspace_bytes");
  c.buf.hist_out = a->hist_out; c.buf.hist[0] = a->hist_1; c.buf.hist[1] = a->hist_2; c.buf.hist[2] = a->hist_3; c.buf.noise = a->noise;
  const NamedBuffer rows[] = {{"noise", a->noise}, {"hist_out", a->hist_out}};
  const NamedBuffer cols[] = {{"latents", a->latents}, {"hist_1", a->hist_1}, {"hist_2", a->hist_2}, {"hist_3", a->hist_3}};
  CfgRescalePlan pl;
  if (int rc = step_check(c, pl)) return rc;
  if (int rc = step_overlap_check(c, rows, cols)) return rc;
  return step_launch(c, pl, stream);
}

// PNDM (PLMS and Runge-Kutta modes): the update from the latents or the saved sample, the raw guided prediction as history
extern "C" int fyc_cfg_pndm_step(const fyc_cfg_pndm_args* a, void* stream) {
  FYC_REQUIRE(a, "fyc_cfg_pndm_step: null pointer");
  StepCall c = step_call(*a, 4, false, true, "fyc_cfg_pndm_step", "fyc_cfg_pndm_workspace_bytes");
  c.buf.sample_in = a->sample_in; c.buf.sample_out = a->sample_out; c.buf.acc_in = a->acc_in; c.buf.acc_out = a->acc_out;
  c.buf.hist_out = a->hist_out; c.buf.hist[0] = a->hist_1; c.buf.hist[1] = a->hist_2; c.buf.hist[2] = a->hist_3;
  const NamedBuffer sample_in[] = {{"sample_in", a->sample_in}}, latents[] = {{"latents", a->latents}};
  const NamedBuffer rows[] = {{"sample_out", a->sample_out}, {"hist_out", a->hist_out}, {kAccOut, a->acc_out}};
  const NamedBuffer cols[] = {{"latents", a->latents}, {"hist_1", a->hist_1}, {"hist_2", a->hist_2}, {"hist_3", a->hist_3}, {"sample_in", a->sample_in}, {kAccIn, a->acc_in}};
  CfgRescalePlan pl;
  if (int rc = step_check(c, pl)) return rc;
  if (int rc = step_overlap_check(c, sample_in, latents)) return rc;      // read where the latents are written
  if (int rc = step_overlap_check(c, rows, cols)) return rc;
  return step_launch(c, pl, stream);
}

extern "C" int fyc_nchw_to_nhwc(const fyc_nchw_in_args* a, void* stream) {
  FYC_REQUIRE(a && a->z && a->x && a->N > 0 && a->C > 0 && a->HW > 0 && a->c_pad >= a->C, "fyc_nchw_to_nhwc: bad args");
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)a->N * a->HW;
  FYC_DT(a,
         hipLaunchKernelGGL(nchw_to_nhwc_kernel<bf16_t>, dim3(grid_for(n)), dim3(256), 0, st, a->z, (bf16_t*)a->x, a->N, a->C, a->HW, a->c_pad, a->scale),
         hipLaunchKernelGGL(nchw_to_nhwc_kernel<f16_t>, dim3(grid_for(n)), dim3(256), 0, st, a->z, (f16_t*)a->x, a->N, a->C, a->HW, a->c_pad, a->scale),
         hipLaunchKernelGGL(nchw_to_nhwc_kernel<float>, dim3(grid_for(n)), dim3(256), 0, st, a->z, (float*)a->x, a->N, a->C, a->HW, a->c_pad, a->scale));
  FYC_CHECK_LAUNCH("fyc_nchw_to_nhwc");
  return 0;
}

extern "C" int fyc_nhwc_to_nchw(const fyc_nhwc_out_args* a, void* stream) {
  FYC_REQUIRE(a && a->x && a->y && a->N > 0 && a->C > 0 && a->HW > 0 && a->ld >= a->C, "fyc_nhwc_to_nchw: bad args");
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)a->N * a->C * a->HW;
  FYC_DT(a,
         hipLaunchKernelGGL(nhwc_to_nchw_kernel<bf16_t>, dim3(grid_for(n)), dim3(256), 0, st, (const bf16_t*)a->x, a->y, a->N, a->C, a->HW, a->ld, a->mul, a->add, a->lo, a->hi),
         hipLaunchKernelGGL(nhwc_to_nchw_kernel<f16_t>, dim3(grid_for(n)), dim3(256), 0, st, (const f16_t*)a->x, a->y, a->N, a->C, a->HW, a->ld, a->mul, a->add, a->lo, a->hi),
         hipLaunchKernelGGL(nhwc_to_nchw_kernel<float>, dim3(grid_for(n)), dim3(256), 0, st, (const float*)a->x, a->y, a->N, a->C, a->HW, a->ld, a->mul, a->add, a->lo, a->hi));
  FYC_CHECK_LAUNCH("fyc_nhwc_to_nchw");
  return 0;
}

extern "C" int fyc_embed_tokens(const fyc_embed_args* a, void* stream) {
  FYC_REQUIRE(a && a->ids && a->table && a->pos && a->out, "fyc_embed_tokens: null pointer");
  FYC_REQUIRE(a->rows > 0 && a->seq > 0 && a->vocab > 0 && a->C > 0 && a->C % 8 == 0, "fyc_embed_tokens: bad dims rows=%lld seq=%d C=%d", (long long)a->rows, a->seq, a->C);
  hipStream_t st = (hipStream_t)stream;
  const long long n = a->rows * (a->C / 8);
  FYC_DT(a,
         hipLaunchKernelGGL(embed_tokens_kernel<bf16_t>, dim3(grid_for(n)), dim3(256), 0, st, (const long long*)a->ids, a->table, a->pos, (bf16_t*)a->out, (long long)a->rows, a->seq, a->C, a->vocab),
         hipLaunchKernelGGL(embed_tokens_kernel<f16_t>, dim3(grid_for(n)), dim3(256), 0, st, (const long long*)a->ids, a->table, a->pos, (f16_t*)a->out, (long long)a->rows, a->seq, a->C, a->vocab),
         hipLaunchKernelGGL(embed_tokens_kernel<float>, dim3(grid_for(n)), dim3(256), 0, st, (const long long*)a->ids, a->table, a->pos, (float*)a->out, (long long)a->rows, a->seq, a->C, a->vocab));
  FYC_CHECK_LAUNCH("fyc_embed_tokens");
  return 0;
}

extern "C" int fyc_patchify(const fyc_patchify_args* a, void* stream) {
  FYC_REQUIRE(a && a->image && a->out, "fyc_patchify: null pointer");
  FYC_REQUIRE(a->B > 0 && a->Cin > 0 && a->P > 0 && a->H > 0 && a->W > 0 && a->H % a->P == 0 && a->W % a->P == 0,
              "fyc_patchify: image %dx%d is not a multiple of the patch size %d", a->H, a->W, a->P);
  FYC_REQUIRE(a->ld >= a->Cin * a->P * a->P, "fyc_patchify: ld=%d < Cin*P*P", a->ld);
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)a->B * (a->H / a->P) * (a->W / a->P) * a->ld;
  FYC_DT(a,
         hipLaunchKernelGGL(patchify_kernel<bf16_t>, dim3(grid_for(n)), dim3(256), 0, st, a->image, (bf16_t*)a->out, a->B, a->Cin, a->H, a->W, a->P, a->ld),
         hipLaunchKernelGGL(patchify_kernel<f16_t>, dim3(grid_for(n)), dim3(256), 0, st, a->image, (f16_t*)a->out, a->B, a->Cin, a->H, a->W, a->P, a->ld),
         hipLaunchKernelGGL(patchify_kernel<float>, dim3(grid_for(n)), dim3(256), 0, st, a->image, (float*)a->out, a->B, a->Cin, a->H, a->W, a->P, a->ld));
  FYC_CHECK_LAUNCH("fyc_patchify");
  return 0;
}

extern "C" int fyc_pack_conv3x3(const fyc_pack_conv3x3_args* a, void* stream) {
  FYC_REQUIRE(a && a->w && a->out && a->O > 0 && a->I > 0, "fyc_pack_conv3x3: bad args");
  hipStream_t st = (hipStream_t)stream;
  const int Ip = (a->I + 63) / 64 * 64;
  const long long n = (long long)a->O * 9 * Ip;
  FYC_DT(a,
         hipLaunchKernelGGL(pack_conv3x3_kernel<bf16_t>, dim3(grid_for(n)), dim3(256), 0, st, a->w, (bf16_t*)a->out, a->O, a->I, Ip, 64),
         hipLaunchKernelGGL(pack_conv3x3_kernel<f16_t>, dim3(grid_for(n)), dim3(256), 0, st, a->w, (f16_t*)a->out, a->O, a->I, Ip, 64),
         hipLaunchKernelGGL(pack_conv3x3_kernel<float>, dim3(grid_for(n)), dim3(256), 0, st, a->w, (float*)a->out, a->O, a->I, Ip, 32));
  FYC_CHECK_LAUNCH("fyc_pack_conv3x3");
  return 0;
}

extern "C" int fyc_pack_geglu(const fyc_pack_geglu_args* a, void* stream) {
  FYC_REQUIRE(a && a->w && a->w_out && a->O > 0 && a->I > 0, "fyc_pack_geglu: bad args");
  FYC_REQUIRE(a->O % 32 == 0, "fyc_pack_geglu: O=%d must be a multiple of 32 (16 value + 16 gate rows per block)", a->O);
  FYC_REQUIRE((a->b == nullptr) == (a->b_out == nullptr), "fyc_pack_geglu: bias in and out must both be given or both be null");
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)a->O * a->I;
  FYC_DT(a,
         hipLaunchKernelGGL(pack_geglu_kernel<bf16_t>, dim3(grid_for(n)), dim3(256), 0, st, a->w, a->b, (bf16_t*)a->w_out, a->b_out, a->O, a->I),
         hipLaunchKernelGGL(pack_geglu_kernel<f16_t>, dim3(grid_for(n)), dim3(256), 0, st, a->w, a->b, (f16_t*)a->w_out, a->b_out, a->O, a->I),
         hipLaunchKernelGGL(pack_geglu_kernel<float>, dim3(grid_for(n)), dim3(256), 0, st, a->w, a->b, (float*)a->w_out, a->b_out, a->O, a->I));
  FYC_CHECK_LAUNCH("fyc_pack_geglu");
  return 0;
}
