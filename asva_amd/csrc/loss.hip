// The training objective's forward value (include/avsd.h; asva_amd/trainer.py): the noising step and the loss reduction of
// audio_cond_animation_trainer.py:119-148.  f32 and integers only: both libraries compile to the same arithmetic.  Both kernels
// stream through HBM once; the only LDS is the four-wave fold of the reduction.
#include "avsd_common.h"

namespace {

inline unsigned grid_for(int64_t n, int block) {
  int64_t g = (n + block - 1) / block;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (unsigned)g;
}

// four f32 with the alignment of one: rows start at multiples of HW floats behind a pointer that is only 4-byte aligned
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// One work item = up to 4 consecutive floats of one (b, c, f) row of HW floats; the last item of a row (v == nvec) is the scalar
// tail of HW % 4 floats.  The products are written as fma(a, x, s * n): one form whatever the compiler's contraction setting.
template <bool V>
__global__ void diffuse_clip_kernel(const float* x0, const float* noise, const int32_t* timesteps, const float* tab_a, const float* tab_s,
                                    int T, float* noisy, float* target, int keep_first, int CF, int F, int HW, int per_row, int64_t total) {
  const int nvec = HW / 4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int v = (int)(i % per_row);
    const int64_t row = i / per_row;                // (b * C + c) * F + f
    const int f = (int)(row % F);
    const int b = (int)(row / CF);
    const int t = timesteps[b];
    if (t < 0 || t >= T) continue;                  // refused by the wrapper; never index the tables with it
    const float a = tab_a[t], s = tab_s[t];
    const bool keep = keep_first && f == 0;
    const int64_t base = row * HW;
    if (v < nvec) {
      const int64_t o = base + v * 4;
      const f32x4_a4 x = *reinterpret_cast<const f32x4_a4*>(x0 + o);
      const f32x4_a4 n = *reinterpret_cast<const f32x4_a4*>(noise + o);
      f32x4_a4 y = x, w = n;
      if (!keep) {
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = fmaf(a, x[e], s * n[e]);
      }
      *reinterpret_cast<f32x4_a4*>(noisy + o) = y;
      if (target) {
        if constexpr (V) {
#pragma unroll
          for (int e = 0; e < 4; ++e) w[e] = fmaf(a, n[e], -(s * x[e]));
        }
        *reinterpret_cast<f32x4_a4*>(target + o) = w;
      }
    } else {
      for (int64_t o = base + nvec * 4; o < base + HW; ++o) {
        const float x = x0[o], n = noise[o];
        noisy[o] = keep ? x : fmaf(a, x, s * n);
        if (target) target[o] = V ? fmaf(a, n, -(s * x)) : n;
      }
    }
  }
}

// Stage 1 of the loss: grid (AVSD_FRAME_MSE_PARTS, B), 256 threads.  A sample is C rows of L = (F - f0) * HW contiguous floats;
// a row is ceil(L / 4) items (the last one the scalar tail of L % 4), and part p owns items [p * ipp, (p + 1) * ipp) of the
// sample's C * per_row: a partition fixed by (C, F - f0, HW) alone.  Thread k of the part takes items k, k + 256, ... in order
// into one f32 accumulator, the wave folds by xor-shuffles, wave 0 adds the four wave sums in index order.
__global__ void __launch_bounds__(256) frame_mse_partial_kernel(const float* pred, const float* target, float* scratch, int f0, int C, int F,
                                                                int HW, int L, int per_row, int ipp, int items) {
  __shared__ float wsum[4];
  const int p = blockIdx.x, b = blockIdx.y;
  const int nvec = L / 4;
  const int lo = p * ipp;
  const int hi = min(lo + ipp, items);
  float acc = 0.f;
  for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
    const int c = i / per_row, v = i - c * per_row;
    const int64_t base = (((int64_t)b * C + c) * F + f0) * HW;
    if (v < nvec) {
      const f32x4_a4 x = *reinterpret_cast<const f32x4_a4*>(pred + base + v * 4);
      const f32x4_a4 y = *reinterpret_cast<const f32x4_a4*>(target + base + v * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = x[e] - y[e];
        acc = fmaf(d, d, acc);
      }
    } else {
      for (int o = nvec * 4; o < L; ++o) {
        const float d = pred[base + o] - target[base + o];
        acc = fmaf(d, d, acc);
      }
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) scratch[(int64_t)b * AVSD_FRAME_MSE_PARTS + p] = ((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
}

// Stage 2: one wave.  Lane p holds partial p of sample b as a double; the xor-shuffle tree gives every lane the same sum; the
// samples are added in index order.
__global__ void __launch_bounds__(64) frame_mse_final_kernel(const float* scratch, float* per_sample, float* loss, int B, double inv_n) {
  static_assert(AVSD_FRAME_MSE_PARTS == 64, "one lane per partial");
  double total = 0.0;
  for (int b = 0; b < B; ++b) {
    double v = (double)scratch[(int64_t)b * AVSD_FRAME_MSE_PARTS + threadIdx.x];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const double m = v * inv_n;
    if (threadIdx.x == 0) per_sample[b] = (float)m;
    total += m;
  }
  if (threadIdx.x == 0) loss[0] = (float)(total / (double)B);
}

bool apart(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x + (uintptr_t)na <= y || y + (uintptr_t)nb <= x;
}

}  // namespace

extern "C" int avsd_diffuse_clip_f32(const float* x0, const float* noise, const int32_t* timesteps, const float* sqrt_acp,
                                     const float* sqrt_1m_acp, int T, float* noisy, float* target, int keep_first, int mode, int B, int C,
                                     int F, int HW, void* stream) {
  AVSD_REQUIRE(x0 && noise && timesteps && sqrt_acp && sqrt_1m_acp && noisy, "diffuse_clip_f32: null pointer");
  AVSD_REQUIRE(B > 0 && C > 0 && F > 0 && HW > 0, "diffuse_clip_f32: shapes must be positive");
  AVSD_REQUIRE(T > 0, "diffuse_clip_f32: the tables need T > 0 entries");
  AVSD_REQUIRE(mode == AVSD_DIFFUSE_EPSILON || mode == AVSD_DIFFUSE_V, "diffuse_clip_f32: mode must be 0 (epsilon) or 1 (v)");
  AVSD_REQUIRE(((uintptr_t)x0 | (uintptr_t)noise | (uintptr_t)timesteps | (uintptr_t)sqrt_acp | (uintptr_t)sqrt_1m_acp | (uintptr_t)noisy |
                (uintptr_t)target) % 4 == 0, "diffuse_clip_f32: pointers must be 4-byte aligned");
  const int64_t rows = (int64_t)B * C * F;
  AVSD_REQUIRE(rows <= INT32_MAX && (int64_t)C * F <= INT32_MAX, "diffuse_clip_f32: B * C * F exceeds 2^31 - 1");
  const int64_t bytes = rows * HW * 4;
  const struct { const void* p; int64_t n; } ins[5] = {{x0, bytes}, {noise, bytes}, {timesteps, (int64_t)B * 4}, {sqrt_acp, (int64_t)T * 4},
                                                       {sqrt_1m_acp, (int64_t)T * 4}};
  for (const auto& in : ins) {
    AVSD_REQUIRE(apart(noisy, bytes, in.p, in.n), "diffuse_clip_f32: noisy overlaps an input (noisy == x0 is not allowed)");
    AVSD_REQUIRE(!target || apart(target, bytes, in.p, in.n), "diffuse_clip_f32: target overlaps an input");
  }
  AVSD_REQUIRE(!target || apart(noisy, bytes, target, bytes), "diffuse_clip_f32: noisy and target overlap");
  const int per_row = (HW + 3) / 4;
  const int64_t total = rows * per_row;
  const dim3 grid(grid_for(total, 256)), block(256);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (mode == AVSD_DIFFUSE_V)
    hipLaunchKernelGGL(diffuse_clip_kernel<true>, grid, block, 0, st, x0, noise, timesteps, sqrt_acp, sqrt_1m_acp, T, noisy, target, keep_first,
                       C * F, F, HW, per_row, total);
  else
    hipLaunchKernelGGL(diffuse_clip_kernel<false>, grid, block, 0, st, x0, noise, timesteps, sqrt_acp, sqrt_1m_acp, T, noisy, target, keep_first,
                       C * F, F, HW, per_row, total);
  AVSD_CHECK_LAUNCH("diffuse_clip_f32 launch");
  return AVSD_OK;
}

extern "C" int avsd_frame_mse_f32(const float* pred, const float* target, int f0, float* scratch, float* per_sample, float* loss, int B, int C,
                                  int F, int HW, void* stream) {
  AVSD_REQUIRE(pred && target && scratch && per_sample && loss, "frame_mse_f32: null pointer");
  AVSD_REQUIRE(B > 0 && C > 0 && F > 0 && HW > 0, "frame_mse_f32: shapes must be positive");
  AVSD_REQUIRE(f0 >= 0 && f0 < F, "frame_mse_f32: no frames to score: need 0 <= f0 (%d) < F (%d)", f0, F);
  AVSD_REQUIRE(B <= 65535, "frame_mse_f32: B (%d) exceeds 65535", B);
  AVSD_REQUIRE(((uintptr_t)pred | (uintptr_t)target | (uintptr_t)scratch | (uintptr_t)per_sample | (uintptr_t)loss) % 4 == 0,
               "frame_mse_f32: pointers must be 4-byte aligned");
  const int64_t L = (int64_t)(F - f0) * HW;
  const int64_t per_row = (L + 3) / 4;
  const int64_t items = per_row * C;
  AVSD_REQUIRE(L <= INT32_MAX && items <= INT32_MAX - 256 * AVSD_FRAME_MSE_PARTS, "frame_mse_f32: a sample of %lld x %d floats is too large",
               (long long)L, C);
  const int64_t bytes = (int64_t)B * C * F * HW * 4, sbytes = (int64_t)B * AVSD_FRAME_MSE_PARTS * 4;
  const struct { const void* p; int64_t n; } outs[3] = {{scratch, sbytes}, {per_sample, (int64_t)B * 4}, {loss, 4}};
  for (int i = 0; i < 3; ++i) {
    AVSD_REQUIRE(apart(outs[i].p, outs[i].n, pred, bytes) && apart(outs[i].p, outs[i].n, target, bytes),
                 "frame_mse_f32: scratch / per_sample / loss overlaps an input");
    for (int j = i + 1; j < 3; ++j)
      AVSD_REQUIRE(apart(outs[i].p, outs[i].n, outs[j].p, outs[j].n), "frame_mse_f32: scratch, per_sample and loss overlap");
  }
  const int ipp = (int)((items + AVSD_FRAME_MSE_PARTS - 1) / AVSD_FRAME_MSE_PARTS);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(frame_mse_partial_kernel, dim3(AVSD_FRAME_MSE_PARTS, B), dim3(256), 0, st, pred, target, scratch, f0, C, F, HW, (int)L,
                     (int)per_row, ipp, (int)items);
  AVSD_CHECK_LAUNCH("frame_mse_f32 partial launch");
  hipLaunchKernelGGL(frame_mse_final_kernel, dim3(1), dim3(64), 0, st, (const float*)scratch, per_sample, loss, B,
                     1.0 / ((double)C * (double)L));
  AVSD_CHECK_LAUNCH("frame_mse_f32 final launch");
  return AVSD_OK;
}
