// Small / elementwise kernels: layout conversion at the NCFHW boundary, sinusoidal timestep
// embedding, skinny (M <= 32) linear layers, the fused guidance + scheduler update and the VAE
// post-processing.  All HBM- or latency-bound; none is worth an MFMA.
//
// Reference: audio_cond_unet_3d_condition.py:673-681 (time embedding), ff_spatio_temp_resnet_3d.py:170
// (time_emb_proj), ff_spatio_audio_temp_transformer_3d.py:348-349 (temporal position MLP),
// pipeline_audio_cond_animation.py:331-337 (latent duplication), :349-364 (guidance, scheduler.step on
// frames 1..), :206-213 (decode post-processing).  diffusers 0.29.2 get_timestep_embedding /
// PNDMScheduler.step_plms / DDIMScheduler.step supply the formulas.
#include "avsd_common.h"
#include "philox.h"

namespace {

// dst_lo != 0: split-precision planes (main + rest, avsd_common.h)
__global__ void ncfhw_to_rows_kernel(const float* src, h16_t* dst, int64_t dst_lo, int B, int C, int F, int HW, int cpad,
                                     int rep, float scale) {
  // one thread per (rep, b, f, p); writes cpad channels
  const int64_t n = (int64_t)rep * B * F * HW;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int p = (int)(i % HW);
    const int f = (int)((i / HW) % F);
    const int b = (int)((i / ((int64_t)HW * F)) % B);
    h16_t* o = dst + i * cpad;
    for (int c = 0; c < cpad; ++c) {
      float v = 0.f;
      if (c < C) v = src[(((int64_t)b * C + c) * F + f) * HW + p] * scale;
      const h16_t m = f2h(v);
      o[c] = m;
      if (dst_lo) o[dst_lo + c] = f2h(v - h2f(m));
    }
  }
}

__global__ void rows_to_ncfhw_kernel(const float* src, int ld, float* dst, int B, int C, int F, int HW) {
  const int64_t n = (int64_t)B * C * F * HW;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int p = (int)(i % HW);
    const int f = (int)((i / HW) % F);
    const int c = (int)((i / ((int64_t)HW * F)) % C);
    const int b = (int)(i / ((int64_t)HW * F * C));
    dst[i] = src[(((int64_t)b * F + f) * HW + p) * ld + c];
  }
}

__global__ void timestep_embedding_kernel(const float* t, float* out, int n, int dim) {
  const int half = dim / 2;
  const int i = blockIdx.x;
  const float tv = t[i];
  for (int j = threadIdx.x; j < half; j += blockDim.x) {
    const float w = expf(-9.210340371976184f * (float)j / (float)half);  // ln(10000)
    const float a = tv * w;
    out[(int64_t)i * dim + j] = cosf(a);          // flip_sin_to_cos: cos half first
    out[(int64_t)i * dim + half + j] = sinf(a);
  }
}

// out[m, n] = act_out(sum_k act_in(x[m, k]) * W[n, k] + bias[n]); one wave per n, 8 rows per block.y
__global__ void split_f32_kernel(const float* src, h16_t* dst, int64_t dst_lo, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = src[i];
    const h16_t m = f2h(v);
    dst[i] = m;
    if (dst_lo) dst[dst_lo + i] = f2h(v - h2f(m));
  }
}

template <bool X2>
__global__ __launch_bounds__(256) void linear_small_m_kernel(const float* x, const h16_t* W, int64_t w_lo, const float* bias,
                                                             float* out, int M, int N, int K, int ldw, int act_in,
                                                             int act_out) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const int m0 = blockIdx.y * 8;
  const int mcount = min(8, M - m0);
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  const h16_t* wrow = W + (int64_t)n * ldw;
  for (int k = lane * 8; k < K; k += 512) {
    float w[8];
    load8<X2>(wrow + k, w_lo, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i < mcount) {
        const float* xr = x + (int64_t)(m0 + i) * K + k;
        const float4 a0 = *reinterpret_cast<const float4*>(xr);
        const float4 a1 = *reinterpret_cast<const float4*>(xr + 4);
        float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float xv = act_in ? silu_f(a[e]) : a[e];
          acc[i] = fmaf(xv, w[e], acc[i]);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float v = wave_sum(acc[i]);
    if (lane == 0 && i < mcount) {
      float r = v + (bias ? bias[n] : 0.f);
      if (act_out) r = silu_f(r);
      out[(int64_t)(m0 + i) * N + n] = r;
    }
  }
}

// What the three scheduler-step kernels share: the CFG batch, the history ring and the latents (include/avsd.h)
struct StepArgs {
  const float* noise_pred; float* hist; const float* x_in; float* x_out;
  int n_branch, store_slot, n_hist;
  int hist_idx[4];
  float g, g2;
  int B, C, F, HW;
};

// guided epsilon of element i: e0 + g (e1 - e0) [+ g2 (e2 - e1)], audio-only / text-only guidance, or the dual form of
// pipeline_audio_cond_animation.py:349-353 with branches [uncond, text, text+audio], g = text scale, g2 = audio scale
__device__ __forceinline__ float guided_eps(const StepArgs& s, int64_t per, int64_t i) {
  float eps = s.noise_pred[i];
  if (s.n_branch >= 2) {
    const float e1 = s.noise_pred[per + i];
    float gsum = eps + s.g * (e1 - eps);
    if (s.n_branch == 3) gsum = gsum + s.g2 * (s.noise_pred[2 * per + i] - e1);
    eps = gsum;
  }
  return eps;
}

// element i lies in frame 0, the pinned image latent that no step updates
__device__ __forceinline__ bool first_frame(const StepArgs& s, int64_t i) {
  return (i % ((int64_t)s.F * s.HW)) / s.HW == 0;
}

struct GuidedArgs {
  StepArgs s;
  float w[4];
  float w_cur, ca, cb;
};

__global__ void guided_step_kernel(const GuidedArgs a) {
  const StepArgs& s = a.s;
  const int64_t per = (int64_t)s.B * s.C * s.F * s.HW;   // elements of one latent tensor
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < per; i += (int64_t)gridDim.x * blockDim.x) {
    const float eps = guided_eps(s, per, i);
    if (s.hist && s.store_slot >= 0) s.hist[(int64_t)s.store_slot * per + i] = eps;
    float e = a.w_cur * eps;
    for (int k = 0; k < s.n_hist; ++k) {
      // the freshly stored slot is read back from the register copy
      const float h = (s.hist_idx[k] == s.store_slot) ? eps : s.hist[(int64_t)s.hist_idx[k] * per + i];
      e = fmaf(a.w[k], h, e);
    }
    const float xin = s.x_in[i];
    s.x_out[i] = first_frame(s, i) ? xin : fmaf(a.ca, xin, a.cb * e);
  }
}

struct MultistepArgs {
  StepArgs s;
  float w[4];
  float ca, c_cur, s_x, s_e;
};

// DPM-Solver++ step: the ring holds data predictions d = s_x x + s_e eps of earlier steps (include/avsd.h)
__global__ void guided_multistep_kernel(const MultistepArgs a) {
  const StepArgs& s = a.s;
  const int64_t per = (int64_t)s.B * s.C * s.F * s.HW;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < per; i += (int64_t)gridDim.x * blockDim.x) {
    const float eps = guided_eps(s, per, i);
    const float xin = s.x_in[i];
    const float d = fmaf(a.s_x, xin, a.s_e * eps);
    if (s.hist && s.store_slot >= 0) s.hist[(int64_t)s.store_slot * per + i] = d;
    float acc = fmaf(a.c_cur, d, a.ca * xin);
    for (int k = 0; k < s.n_hist; ++k) {
      const float h = (s.hist_idx[k] == s.store_slot) ? d : s.hist[(int64_t)s.hist_idx[k] * per + i];
      acc = fmaf(a.w[k], h, acc);
    }
    s.x_out[i] = first_frame(s, i) ? xin : acc;
  }
}

// ---- the stochastic forms of the two kernels above (DDIM eta > 0, SDE-DPM-Solver++; include/avsd.h): the same update plus
// c_noise z, the normal z evaluated in registers (csrc/philox.h).  V = 4: a thread owns four consecutive elements of one frame row
// and moves them as float4 (HW % 4 == 0, every base pointer 16-byte aligned: the entry point decides); V = 1: one element per
// thread.  Every element goes through the same scalar expressions in both, so the two paths give the same bits.
struct NoiseArgs {
  float c_noise;
  philox::Key key;   // key.stream is the stream of batch row 0: row b draws from stream + b
};

template <int V>
__device__ __forceinline__ void ldv(const float* p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = *p;
  }
}

template <int V>
__device__ __forceinline__ void stv(float* p, const float (&v)[V]) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

// guided_eps for V consecutive elements
template <int V>
__device__ __forceinline__ void guided_eps_v(const StepArgs& s, int64_t per, int64_t i, float (&eps)[V]) {
  ldv<V>(s.noise_pred + i, eps);
  if (s.n_branch >= 2) {
    float e1[V], e2[V];
    ldv<V>(s.noise_pred + per + i, e1);
    if (s.n_branch == 3) ldv<V>(s.noise_pred + 2 * per + i, e2);
#pragma unroll
    for (int l = 0; l < V; ++l) {
      float gsum = eps[l] + s.g * (e1[l] - eps[l]);
      if (s.n_branch == 3) gsum = gsum + s.g2 * (e2[l] - e1[l]);
      eps[l] = gsum;
    }
  }
}

// history entry k for V consecutive elements: the freshly stored slot is read back from the register copy
template <int V>
__device__ __forceinline__ void hist_v(const StepArgs& s, int64_t per, int64_t i, int k, const float (&cur)[V], float (&h)[V]) {
  if (s.hist_idx[k] == s.store_slot) {
#pragma unroll
    for (int l = 0; l < V; ++l) h[l] = cur[l];
  } else {
    ldv<V>(s.hist + (int64_t)s.hist_idx[k] * per + i, h);
  }
}

// x_out[i .. i + V) = acc + c_noise z on frames 1.., x_in on frame 0.  Element (b, c, f >= 1, p) takes normal
// j = (c (F - 1) + (f - 1)) HW + p of (seed, stream + b, step): lane j & 3 of block j >> 2.  With V = 4, i and HW are multiples of
// 4, so j is one too and the four elements are the four lanes of one block.
template <int V>
__device__ __forceinline__ void store_noisy(const StepArgs& s, const NoiseArgs& nz, int64_t i, const float (&xin)[V],
                                            const float (&acc)[V]) {
  const int64_t fhw = (int64_t)s.F * s.HW;
  const int64_t bc = i / fhw, q = i - bc * fhw;    // bc = b C + c,  q = f HW + p
  if (q < s.HW) {                                   // frame 0: copied through, no normal spent
    stv<V>(s.x_out + i, xin);
    return;
  }
  const uint32_t b = (uint32_t)bc / (uint32_t)s.C, c = (uint32_t)bc - b * (uint32_t)s.C;     // B C < 2^31 (noise_require)
  const uint64_t j = (uint64_t)c * (uint64_t)(fhw - s.HW) + (uint64_t)(q - s.HW);
  philox::Key key = nz.key;
  key.stream += b;
  // an empty statement that only makes the key opaque here: the ten round keys are then derived inside the loop body instead of
  // being kept live across it in 20 scalar registers, which the float4 kernels do not have to spare.  Register allocation only:
  // without it the results are the same bits and asva_amd/resource_usage_gfx950.json shows two scalar spills in one kernel.
  asm volatile("" : "+s"(key.k0), "+s"(key.k1));
  float z[4], out[V];
  philox::normal4(key, j >> 2, z);
  if constexpr (V == 4) {
#pragma unroll
    for (int l = 0; l < 4; ++l) out[l] = fmaf(nz.c_noise, z[l], acc[l]);
  } else {
    const int lane = (int)(j & 3);
    const float zl = lane == 0 ? z[0] : lane == 1 ? z[1] : lane == 2 ? z[2] : z[3];
    out[0] = fmaf(nz.c_noise, zl, acc[0]);
  }
  stv<V>(s.x_out + i, out);
}

template <int V>
__global__ __launch_bounds__(256) void guided_step_sde_kernel(const GuidedArgs a, const NoiseArgs nz) {
  const StepArgs& s = a.s;
  const int64_t per = (int64_t)s.B * s.C * s.F * s.HW;
  for (int64_t i = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) * V; i < per; i += (int64_t)gridDim.x * blockDim.x * V) {
    float eps[V], e[V], xin[V], acc[V];
    guided_eps_v<V>(s, per, i, eps);
    if (s.hist && s.store_slot >= 0) stv<V>(s.hist + (int64_t)s.store_slot * per + i, eps);
#pragma unroll
    for (int l = 0; l < V; ++l) e[l] = a.w_cur * eps[l];
    for (int k = 0; k < s.n_hist; ++k) {
      float h[V];
      hist_v<V>(s, per, i, k, eps, h);
#pragma unroll
      for (int l = 0; l < V; ++l) e[l] = fmaf(a.w[k], h[l], e[l]);
    }
    ldv<V>(s.x_in + i, xin);
#pragma unroll
    for (int l = 0; l < V; ++l) acc[l] = fmaf(a.ca, xin[l], a.cb * e[l]);
    store_noisy<V>(s, nz, i, xin, acc);
  }
}

template <int V>
__global__ __launch_bounds__(256) void guided_multistep_sde_kernel(const MultistepArgs a, const NoiseArgs nz) {
  const StepArgs& s = a.s;
  const int64_t per = (int64_t)s.B * s.C * s.F * s.HW;
  for (int64_t i = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) * V; i < per; i += (int64_t)gridDim.x * blockDim.x * V) {
    float eps[V], xin[V], d[V], acc[V];
    guided_eps_v<V>(s, per, i, eps);
    ldv<V>(s.x_in + i, xin);
#pragma unroll
    for (int l = 0; l < V; ++l) d[l] = fmaf(a.s_x, xin[l], a.s_e * eps[l]);
    if (s.hist && s.store_slot >= 0) stv<V>(s.hist + (int64_t)s.store_slot * per + i, d);
#pragma unroll
    for (int l = 0; l < V; ++l) acc[l] = fmaf(a.c_cur, d[l], a.ca * xin[l]);
    for (int k = 0; k < s.n_hist; ++k) {
      float h[V];
      hist_v<V>(s, per, i, k, d, h);
#pragma unroll
      for (int l = 0; l < V; ++l) acc[l] = fmaf(a.w[k], h[l], acc[l]);
    }
    store_noisy<V>(s, nz, i, xin, acc);
  }
}

struct UniPCArgs {
  StepArgs s;
  float* x_last;
  int use_corrector;
  float wc[4], wp[4];
  float s_x, s_e, cc_last, cc_cur, cp_x, cp_cur;
};

// UniPC step: the corrector of the sample the UNet just saw, then the predictor for the next sigma (include/avsd.h).  Unlike the
// two kernels above, every history slot is read BEFORE this step's data prediction is stored, so the store may take the oldest one.
__global__ void guided_unipc_kernel(const UniPCArgs a) {
  const StepArgs& s = a.s;
  const int64_t per = (int64_t)s.B * s.C * s.F * s.HW;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < per; i += (int64_t)gridDim.x * blockDim.x) {
    const float eps = guided_eps(s, per, i);
    const float xin = s.x_in[i];
    const float d = fmaf(a.s_x, xin, a.s_e * eps);
    float h[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) h[k] = (k < s.n_hist) ? s.hist[(int64_t)s.hist_idx[k] * per + i] : 0.f;
    float xc = xin;
    if (a.use_corrector) {
      xc = fmaf(a.cc_cur, d, a.cc_last * a.x_last[i]);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < s.n_hist) xc = fmaf(a.wc[k], h[k], xc);
    }
    float acc = fmaf(a.cp_cur, d, a.cp_x * xc);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < s.n_hist) acc = fmaf(a.wp[k], h[k], acc);
    const bool first = first_frame(s, i);
    if (s.store_slot >= 0) s.hist[(int64_t)s.store_slot * per + i] = d;
    a.x_last[i] = first ? xin : xc;
    s.x_out[i] = first ? xin : acc;
  }
}

__global__ void vae_postprocess_kernel(const h16_t* src, int ld, int64_t src_lo, float* dst, int N, int HW) {
  const int64_t n = (int64_t)N * 3 * HW;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int p = (int)(i % HW);
    const int c = (int)((i / HW) % 3);
    const int im = (int)(i / ((int64_t)3 * HW));
    const int64_t o = ((int64_t)im * HW + p) * ld + c;
    const float x = h2f(src[o]) + (src_lo ? h2f(src[src_lo + o]) : 0.f);
    const float v = x * 0.5f + 0.5f;
    dst[i] = fminf(fmaxf(v, 0.f), 1.f);
  }
}

// channels-last bf16 rows [N*HW][ld] -> uint8 frames (N, H, W, 3): (clamp(x/2+0.5, 0, 1) * 255) truncated, i.e. the
// pipeline's post-processing (:212) followed by generate_videos' `(video.permute(0,2,3,1) * 255).byte()` (:448)
__global__ void vae_postprocess_u8_kernel(const h16_t* src, int ld, int64_t src_lo, uint8_t* dst, int64_t npix) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
    const h16_t* s = src + i * ld;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float x = h2f(s[c]) + (src_lo ? h2f(s[src_lo + c]) : 0.f);
      const float v = fminf(fmaxf(x * 0.5f + 0.5f, 0.f), 1.f);
      dst[i * 3 + c] = (uint8_t)(v * 255.0f);
    }
  }
}

inline unsigned grid_for(int64_t n, int block) {
  int64_t g = (n + block - 1) / block;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (unsigned)g;
}

// dst[r][i] = src[i], 16 bytes per thread per round: each vector is read once and written `rep` times
__global__ void copy_rep_kernel(const uint4* src, uint4* dst, int64_t nvec, int rep) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
    const uint4 v = src[i];
    for (int r = 0; r < rep; ++r) dst[(int64_t)r * nvec + i] = v;
  }
}

// four f32 with the alignment of one: a frame row starts at a multiple of HW floats, which is 16-byte aligned only when HW % 4 == 0
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// Turnover between two chained windows (include/avsd.h).  One work item = up to 4 consecutive floats of one (b, c, unit) row;
// unit 0 moves frame F-1 of x_prev to frame 0 of x_next AND writes frame F-1 of x_next, in that order and in the same thread, so
// that x_next == x_prev is safe: nobody else touches that piece of frame F-1.  Unit u >= 1 writes frame u (1 <= u <= F-2).
// The last item of a row (v == nvec) is the scalar tail of HW % 4 floats.
__global__ void window_turnover_kernel(const float* x_prev, const float* noise, float* x_next, float sigma, int F, int HW,
                                       int units, int per_row, int64_t total) {
  const int nvec = HW / 4;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int v = (int)(t % per_row);
    const int u = (int)((t / per_row) % units);
    const int64_t bc = t / ((int64_t)per_row * units);
    const int64_t xrow = bc * F * HW;               // (b, c) slab of the latents: F rows of HW
    const int64_t nrow = bc * (F - 1) * HW;         // ... of the noise: F - 1 rows
    const int fn = (u == 0) ? F - 1 : u;            // the frame this item fills with noise (none when F == 1)
    if (v < nvec) {
      const int o = v * 4;
      if (u == 0) {
        const f32x4_a4 last = *reinterpret_cast<const f32x4_a4*>(x_prev + xrow + (int64_t)(F - 1) * HW + o);
        *reinterpret_cast<f32x4_a4*>(x_next + xrow + o) = last;
      }
      if (fn >= 1) {
        const f32x4_a4 n4 = *reinterpret_cast<const f32x4_a4*>(noise + nrow + (int64_t)(fn - 1) * HW + o);
        *reinterpret_cast<f32x4_a4*>(x_next + xrow + (int64_t)fn * HW + o) = n4 * sigma;
      }
    } else {
      for (int o = nvec * 4; o < HW; ++o) {
        if (u == 0) {
          const float last = x_prev[xrow + (int64_t)(F - 1) * HW + o];
          x_next[xrow + o] = last;
        }
        if (fn >= 1) x_next[xrow + (int64_t)fn * HW + o] = noise[nrow + (int64_t)(fn - 1) * HW + o] * sigma;
      }
    }
  }
}

// one thread per (block b, key slot j < lk_pad, 8-channel chunk): K rows copied as they are, V written transposed; the
// padding slots j >= lk are written as zeros on every call (the fused kernel multiplies p = 0 by the V^T padding, so it
// must be finite whatever the allocator handed out — a replaying host binds fresh memory)
__global__ void xattn_pack_kv_kernel(const h16_t* kv, int rows, int C, const int32_t* idx, int n_frames, int nk, int lk,
                                     h16_t* k_out, h16_t* vt_out, int lk_pad, int64_t total) {
  const int c8n = C / 8;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int c8 = (int)(t % c8n);
    const int j = (int)((t / c8n) % lk_pad);
    const int b = (int)(t / ((int64_t)c8n * lk_pad));
    if (j >= lk) {
      *reinterpret_cast<uint4*>(k_out + ((int64_t)b * lk_pad + j) * C + c8 * 8) = make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 8; ++e) vt_out[((int64_t)b * C + c8 * 8 + e) * lk_pad + j] = 0;
      continue;
    }
    const int n = idx ? b / n_frames : b;
    const int key = idx ? idx[(b % n_frames) * nk + j] : j;
    const h16_t* src = kv + ((int64_t)n * rows + key) * 2 * C + c8 * 8;
    *reinterpret_cast<uint4*>(k_out + ((int64_t)b * lk_pad + j) * C + c8 * 8) = *reinterpret_cast<const uint4*>(src);
    const uint4 v = *reinterpret_cast<const uint4*>(src + C);
    const h16_t* ve = reinterpret_cast<const h16_t*>(&v);
#pragma unroll
    for (int e = 0; e < 8; ++e) vt_out[((int64_t)b * C + c8 * 8 + e) * lk_pad + j] = ve[e];
  }
}

// The checks of the three avsd_guided_* entry points on what they share, then `s` filled in with the ring table padded to 4
// entries; `who` prefixes the messages, `tables`: every weight table of the entry point is there.
int step_require(const char* who, StepArgs& s, const float* noise_pred, int n_branch, float g, float g2, float* hist, int store_slot,
                 const int32_t* hist_idx, bool tables, int n_hist, const float* x_in, float* x_out, int B, int C, int F, int HW) {
  AVSD_REQUIRE(noise_pred && x_in && x_out, "%s: null pointer", who);
  AVSD_REQUIRE(n_branch >= 1 && n_branch <= 3, "%s: n_branch must be 1, 2 or 3", who);
  AVSD_REQUIRE(n_hist >= 0 && n_hist <= 4, "%s: n_hist must be in [0, 4]", who);
  AVSD_REQUIRE((n_hist == 0 && store_slot < 0) || hist, "%s: history requested without hist", who);
  AVSD_REQUIRE(n_hist == 0 || (hist_idx && tables), "%s: null history tables", who);
  AVSD_REQUIRE(B > 0 && C > 0 && F > 0 && HW > 0, "%s: bad shape", who);
  s = StepArgs{noise_pred, hist, x_in, x_out, n_branch, store_slot, n_hist, {0, 0, 0, 0}, g, g2, B, C, F, HW};
  for (int k = 0; k < n_hist; ++k) s.hist_idx[k] = hist_idx[k];
  return AVSD_OK;
}

inline void pad4(float* dst, const float* src, int n) {
  for (int k = 0; k < 4; ++k) dst[k] = k < n ? src[k] : 0.f;
}

// What the two avsd_guided_*_sde entry points add to step_require: batch row b draws from stream + b, which must stay a 32-bit id,
// and the kernels split b C + c with a 32-bit division.
int noise_require(const char* who, NoiseArgs& nz, float c_noise, uint64_t seed, uint32_t stream, uint32_t step, int B, int C) {
  AVSD_REQUIRE((uint64_t)stream + (uint64_t)B <= (1ull << 32), "%s: stream + B exceeds 2^32 (stream=%u B=%d)", who, stream, B);
  AVSD_REQUIRE((int64_t)B * C <= INT32_MAX, "%s: B * C exceeds 2^31 - 1 (B=%d C=%d)", who, B, C);
  nz = NoiseArgs{c_noise, philox::make_key(seed, stream, step)};
  return AVSD_OK;
}

// the float4 path: whole frame rows of 4-element groups, and every pointer the kernel offsets by multiples of 16 bytes aligned
inline bool step_vectorizes(const StepArgs& s) {
  const uintptr_t bits = (uintptr_t)s.noise_pred | (uintptr_t)s.x_in | (uintptr_t)s.x_out | (uintptr_t)s.hist;
  return s.HW % 4 == 0 && bits % 16 == 0;
}

}  // namespace

extern "C" int avsd_ncfhw_to_rows_x2(const float* src, void* dst, int64_t dst_lo, int B, int C, int F, int HW, int cpad, int rep,
                                     float scale, void* stream) {
  AVSD_REQUIRE(src && dst && B > 0 && C > 0 && F > 0 && HW > 0 && cpad >= C && rep >= 1, "ncfhw_to_rows: bad arguments");
  const int64_t n = (int64_t)rep * B * F * HW;
  hipLaunchKernelGGL(ncfhw_to_rows_kernel, dim3(grid_for(n, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     src, (h16_t*)dst, dst_lo, B, C, F, HW, cpad, rep, scale);
  AVSD_CHECK_LAUNCH("ncfhw_to_rows launch");
  return AVSD_OK;
}

extern "C" int avsd_ncfhw_to_rows(const float* src, void* dst, int B, int C, int F, int HW, int cpad, int rep,
                                  float scale, void* stream) {
  return avsd_ncfhw_to_rows_x2(src, dst, 0, B, C, F, HW, cpad, rep, scale, stream);
}

extern "C" int avsd_split_f32(const float* src, void* dst, int64_t dst_lo, int64_t n, void* stream) {
  AVSD_REQUIRE(src && dst && n > 0, "split_f32: bad arguments");
  hipLaunchKernelGGL(split_f32_kernel, dim3(grid_for(n, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src,
                     (h16_t*)dst, dst_lo, n);
  AVSD_CHECK_LAUNCH("split_f32 launch");
  return AVSD_OK;
}

extern "C" int avsd_rows_to_ncfhw(const float* src, int ld, float* dst, int B, int C, int F, int HW, void* stream) {
  AVSD_REQUIRE(src && dst && B > 0 && C > 0 && F > 0 && HW > 0 && ld >= C, "rows_to_ncfhw: bad arguments");
  const int64_t n = (int64_t)B * C * F * HW;
  hipLaunchKernelGGL(rows_to_ncfhw_kernel, dim3(grid_for(n, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     src, ld, dst, B, C, F, HW);
  AVSD_CHECK_LAUNCH("rows_to_ncfhw launch");
  return AVSD_OK;
}

extern "C" int avsd_timestep_embedding(const float* t, float* out, int n, int dim, void* stream) {
  AVSD_REQUIRE(t && out && n > 0 && dim > 0 && dim % 2 == 0, "timestep_embedding: bad arguments");
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3((unsigned)n), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), t,
                     out, n, dim);
  AVSD_CHECK_LAUNCH("timestep_embedding launch");
  return AVSD_OK;
}

extern "C" int avsd_linear_small_m_x2(const float* x, const void* W, int64_t w_lo, const float* bias, float* out, int M, int N, int K,
                                      int ldw, int act_in, int act_out, void* stream) {
  AVSD_REQUIRE(x && W && out, "linear_small_m: null pointer");
  AVSD_REQUIRE(M > 0 && M <= 64 && N > 0 && K > 0 && K % 8 == 0 && ldw % 8 == 0 && ldw >= K && w_lo % 8 == 0,
               "linear_small_m: need 0 < M <= 64, K %% 8 == 0, ldw %% 8 == 0 (M=%d N=%d K=%d ldw=%d)", M, N, K, ldw);
  dim3 grid((unsigned)((N + 3) / 4), (unsigned)((M + 7) / 8));
  if (w_lo != 0)
    hipLaunchKernelGGL(linear_small_m_kernel<true>, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x,
                       (const h16_t*)W, w_lo, bias, out, M, N, K, ldw, act_in, act_out);
  else
    hipLaunchKernelGGL(linear_small_m_kernel<false>, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x,
                       (const h16_t*)W, w_lo, bias, out, M, N, K, ldw, act_in, act_out);
  AVSD_CHECK_LAUNCH("linear_small_m launch");
  return AVSD_OK;
}

extern "C" int avsd_linear_small_m(const float* x, const void* W, const float* bias, float* out, int M, int N, int K,
                                   int ldw, int act_in, int act_out, void* stream) {
  return avsd_linear_small_m_x2(x, W, 0, bias, out, M, N, K, ldw, act_in, act_out, stream);
}

extern "C" int avsd_guided_step(const float* noise_pred, int n_branch, float g, float g2, float* eps_hist, int store_slot,
                                float w_cur, const int32_t* hist_idx, const float* w, int n_hist, const float* x_in,
                                float* x_out, float ca, float cb, int B, int C, int F, int HW, void* stream) {
  GuidedArgs a;
  if (int rc = step_require("guided_step", a.s, noise_pred, n_branch, g, g2, eps_hist, store_slot, hist_idx, w != nullptr, n_hist, x_in,
                            x_out, B, C, F, HW))
    return rc;
  pad4(a.w, w, n_hist);
  a.w_cur = w_cur; a.ca = ca; a.cb = cb;
  const int64_t n = (int64_t)B * C * F * HW;
  hipLaunchKernelGGL(guided_step_kernel, dim3(grid_for(n, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  AVSD_CHECK_LAUNCH("guided_step launch");
  return AVSD_OK;
}

extern "C" int avsd_guided_multistep(const float* noise_pred, int n_branch, float g, float g2, float* hist, int store_slot,
                                     const int32_t* hist_idx, const float* w, int n_hist, const float* x_in, float* x_out,
                                     float ca, float c_cur, float s_x, float s_e, int B, int C, int F, int HW, void* stream) {
  MultistepArgs a;
  if (int rc = step_require("guided_multistep", a.s, noise_pred, n_branch, g, g2, hist, store_slot, hist_idx, w != nullptr, n_hist, x_in,
                            x_out, B, C, F, HW))
    return rc;
  pad4(a.w, w, n_hist);
  a.ca = ca; a.c_cur = c_cur; a.s_x = s_x; a.s_e = s_e;
  const int64_t n = (int64_t)B * C * F * HW;
  hipLaunchKernelGGL(guided_multistep_kernel, dim3(grid_for(n, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  AVSD_CHECK_LAUNCH("guided_multistep launch");
  return AVSD_OK;
}

extern "C" int avsd_guided_step_sde(const float* noise_pred, int n_branch, float g, float g2, float* eps_hist, int store_slot,
                                    float w_cur, const int32_t* hist_idx, const float* w, int n_hist, const float* x_in,
                                    float* x_out, float ca, float cb, int B, int C, int F, int HW, float c_noise, uint64_t seed,
                                    uint32_t stream, uint32_t step, void* hip_stream) {
  GuidedArgs a;
  NoiseArgs nz;
  if (int rc = step_require("guided_step_sde", a.s, noise_pred, n_branch, g, g2, eps_hist, store_slot, hist_idx, w != nullptr, n_hist,
                            x_in, x_out, B, C, F, HW))
    return rc;
  if (int rc = noise_require("guided_step_sde", nz, c_noise, seed, stream, step, B, C)) return rc;
  pad4(a.w, w, n_hist);
  a.w_cur = w_cur; a.ca = ca; a.cb = cb;
  const int64_t n = (int64_t)B * C * F * HW;
  if (step_vectorizes(a.s))
    hipLaunchKernelGGL(guided_step_sde_kernel<4>, dim3(grid_for(n / 4, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream), a,
                       nz);
  else
    hipLaunchKernelGGL(guided_step_sde_kernel<1>, dim3(grid_for(n, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream), a, nz);
  AVSD_CHECK_LAUNCH("guided_step_sde launch");
  return AVSD_OK;
}

extern "C" int avsd_guided_multistep_sde(const float* noise_pred, int n_branch, float g, float g2, float* hist, int store_slot,
                                         const int32_t* hist_idx, const float* w, int n_hist, const float* x_in, float* x_out,
                                         float ca, float c_cur, float s_x, float s_e, int B, int C, int F, int HW, float c_noise,
                                         uint64_t seed, uint32_t stream, uint32_t step, void* hip_stream) {
  MultistepArgs a;
  NoiseArgs nz;
  if (int rc = step_require("guided_multistep_sde", a.s, noise_pred, n_branch, g, g2, hist, store_slot, hist_idx, w != nullptr, n_hist,
                            x_in, x_out, B, C, F, HW))
    return rc;
  if (int rc = noise_require("guided_multistep_sde", nz, c_noise, seed, stream, step, B, C)) return rc;
  pad4(a.w, w, n_hist);
  a.ca = ca; a.c_cur = c_cur; a.s_x = s_x; a.s_e = s_e;
  const int64_t n = (int64_t)B * C * F * HW;
  if (step_vectorizes(a.s))
    hipLaunchKernelGGL(guided_multistep_sde_kernel<4>, dim3(grid_for(n / 4, 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(hip_stream), a, nz);
  else
    hipLaunchKernelGGL(guided_multistep_sde_kernel<1>, dim3(grid_for(n, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream),
                       a, nz);
  AVSD_CHECK_LAUNCH("guided_multistep_sde launch");
  return AVSD_OK;
}

extern "C" int avsd_guided_unipc(const float* noise_pred, int n_branch, float g, float g2, float* hist, int store_slot,
                                 const int32_t* hist_idx, const float* wc, const float* wp, int n_hist, const float* x_in,
                                 float* x_out, float* x_last, int use_corrector, float s_x, float s_e, float cc_last,
                                 float cc_cur, float cp_x, float cp_cur, int B, int C, int F, int HW, void* stream) {
  AVSD_REQUIRE(x_last, "guided_unipc: null pointer");
  UniPCArgs a;
  if (int rc = step_require("guided_unipc", a.s, noise_pred, n_branch, g, g2, hist, store_slot, hist_idx, wc && wp, n_hist, x_in, x_out,
                            B, C, F, HW))
    return rc;
  AVSD_REQUIRE(x_last != x_in && x_last != x_out, "guided_unipc: x_last must not alias x_in or x_out");
  for (int k = 0; k < n_hist; ++k) AVSD_REQUIRE(hist_idx[k] >= 0, "guided_unipc: negative history slot");
  a.x_last = x_last; a.use_corrector = use_corrector != 0;
  pad4(a.wc, wc, n_hist);
  pad4(a.wp, wp, n_hist);
  a.s_x = s_x; a.s_e = s_e; a.cc_last = cc_last; a.cc_cur = cc_cur; a.cp_x = cp_x; a.cp_cur = cp_cur;
  const int64_t n = (int64_t)B * C * F * HW;
  hipLaunchKernelGGL(guided_unipc_kernel, dim3(grid_for(n, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  AVSD_CHECK_LAUNCH("guided_unipc launch");
  return AVSD_OK;
}

extern "C" int avsd_vae_postprocess_x2(const void* src, int ld, int64_t src_lo, float* dst, int N, int HW, void* stream) {
  AVSD_REQUIRE(src && dst && N > 0 && HW > 0 && ld >= 3, "vae_postprocess: bad arguments");
  const int64_t n = (int64_t)N * 3 * HW;
  hipLaunchKernelGGL(vae_postprocess_kernel, dim3(grid_for(n, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     (const h16_t*)src, ld, src_lo, dst, N, HW);
  AVSD_CHECK_LAUNCH("vae_postprocess launch");
  return AVSD_OK;
}

extern "C" int avsd_vae_postprocess(const void* src, int ld, float* dst, int N, int HW, void* stream) {
  return avsd_vae_postprocess_x2(src, ld, 0, dst, N, HW, stream);
}

extern "C" int avsd_vae_postprocess_u8_x2(const void* src, int ld, int64_t src_lo, void* dst, int N, int HW, void* stream) {
  AVSD_REQUIRE(src && dst && N > 0 && HW > 0 && ld >= 3, "vae_postprocess_u8: bad arguments");
  const int64_t n = (int64_t)N * HW;
  hipLaunchKernelGGL(vae_postprocess_u8_kernel, dim3(grid_for(n, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     (const h16_t*)src, ld, src_lo, (uint8_t*)dst, n);
  AVSD_CHECK_LAUNCH("vae_postprocess_u8 launch");
  return AVSD_OK;
}

extern "C" int avsd_vae_postprocess_u8(const void* src, int ld, void* dst, int N, int HW, void* stream) {
  return avsd_vae_postprocess_u8_x2(src, ld, 0, dst, N, HW, stream);
}

extern "C" int avsd_copy(const void* src, void* dst, int64_t bytes, int rep, void* stream) {
  AVSD_REQUIRE(src && dst && bytes > 0 && bytes % 16 == 0 && rep >= 1, "copy: need non-null pointers, bytes %% 16 == 0, rep >= 1");
  AVSD_REQUIRE(((uintptr_t)src | (uintptr_t)dst) % 16 == 0, "copy: pointers must be 16-byte aligned");
  const int64_t nvec = bytes / 16;
  hipLaunchKernelGGL(copy_rep_kernel, dim3(grid_for(nvec, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     (const uint4*)src, (uint4*)dst, nvec, rep);
  AVSD_CHECK_LAUNCH("copy launch");
  return AVSD_OK;
}

extern "C" int avsd_window_turnover(const float* x_prev, const float* noise, float* x_next, float sigma, int B, int C, int F, int HW,
                                    void* stream) {
  AVSD_REQUIRE(x_prev && x_next, "window_turnover: null pointer");
  AVSD_REQUIRE(B > 0 && C > 0 && F > 0 && HW > 0, "window_turnover: bad shape");
  AVSD_REQUIRE(noise || F == 1, "window_turnover: frames 1.. need noise");
  AVSD_REQUIRE(((uintptr_t)x_prev | (uintptr_t)x_next | (uintptr_t)noise) % 4 == 0, "window_turnover: pointers must be 4-byte aligned");
  const int64_t xbytes = (int64_t)B * C * F * HW * 4, nbytes = (int64_t)B * C * (F - 1) * HW * 4;
  const uintptr_t xp = (uintptr_t)x_prev, xn = (uintptr_t)x_next, nz = (uintptr_t)noise;
  AVSD_REQUIRE(xp == xn || xp + xbytes <= xn || xn + xbytes <= xp, "window_turnover: x_next must equal x_prev or not overlap it");
  AVSD_REQUIRE(nbytes == 0 || nz + nbytes <= xn || xn + xbytes <= nz, "window_turnover: noise must not overlap x_next");
  const int units = F > 2 ? F - 1 : 1;
  const int per_row = (HW + 3) / 4;
  const int64_t total = (int64_t)B * C * units * per_row;
  hipLaunchKernelGGL(window_turnover_kernel, dim3(grid_for(total, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     x_prev, noise, x_next, sigma, F, HW, units, per_row, total);
  AVSD_CHECK_LAUNCH("window_turnover launch");
  return AVSD_OK;
}

extern "C" int avsd_xattn_pack_kv(const void* kv, int n_kv, int rows, int C, const int32_t* idx, int n_frames, int nk,
                                  void* k_out, void* vt_out, int lk_pad, void* stream) {
  AVSD_REQUIRE(kv && k_out && vt_out && n_kv > 0 && rows > 0 && C > 0 && C % 8 == 0, "xattn_pack_kv: bad arguments");
  AVSD_REQUIRE(!idx || (n_frames > 0 && nk > 0 && nk <= rows), "xattn_pack_kv: a gather list needs n_frames > 0 and 0 < nk <= rows");
  const int lk = idx ? nk : rows;
  AVSD_REQUIRE(lk_pad >= lk, "xattn_pack_kv: lk_pad (%d) < keys per block (%d)", lk_pad, lk);
  const int nb = idx ? n_kv * n_frames : n_kv;
  const int64_t total = (int64_t)nb * lk_pad * (C / 8);
  hipLaunchKernelGGL(xattn_pack_kv_kernel, dim3(grid_for(total, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     (const h16_t*)kv, rows, C, idx, n_frames, nk, lk, (h16_t*)k_out, (h16_t*)vt_out, lk_pad, total);
  AVSD_CHECK_LAUNCH("xattn_pack_kv launch");
  return AVSD_OK;
}
