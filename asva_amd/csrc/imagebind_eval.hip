// ImageBind evaluation towers (asva_amd/imagebind_eval.py): the kernels CLIPSim and AlignSync need beyond csrc/avsync.hip (linear
// layers, patch embedding: avsd_convnd_f32) and csrc/clip_text.hip (LayerNorm, token embedding, causal attention) — bidirectional
// self-attention for the ViT-H/14 vision tower (257 tokens, heads of 80) and the audio trunk (230 keys, heads of 64), erf-GELU,
// cls + position rows, and the cosine of embedding rows.  A metric must not move with the storage mode of the clip it judges, so
// NOTHING here uses the 16-bit type of the build: tensors are f32, products run on v_mfma_f32_32x32x2_f32, and the bf16 and fp16
// libraries compile this file to the same arithmetic.
#include "avsd_common.h"

#include <math.h>

namespace {

// ---- avsd_attention_f32 ---------------------------------------------------------------------------------------------------------------
// Grid (query block, head, sequence); 256 threads = 4 waves; wave w owns queries 128 qb + 32 w .. + 31.  K and V of the head stream
// through LDS in tiles of 64 keys, flash style: a lane keeps the running maximum m and denominator l of ITS query, so any sequence
// length fits.
//
// Layout (the idea of attention_causal_f32_kernel, csrc/clip_text.hip, taken one step further).  The first product is transposed,
// S^T = K . Q^T: in the C/D layout of v_mfma_f32_32x32x2_f32 (column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) a lane
// holds, for its query lane & 31, the scores of 16 keys per 32-key subtile, and the softmax of a query is in-lane plus one exchange
// between the halves of the wave.  The second product is transposed too, O^T = V^T . P^T: the probabilities are its B operand
// (B[k = lane >> 5][j = lane & 31], the same lane map as an A operand) if step r takes the two keys (r & 3) + 8 (r >> 2) + {0, 4},
// and the accumulator column is again the lane's own query — the rescale by exp(m_old - m_new) and the final 1 / l are in-lane, with
// no exchange.  A lane ends with 4-channel runs of its query's output row and stores them as float4.
//
// Every output element is one chain: keys in ascending tiles, inside a subtile in the order above, the rescale between tiles.  The
// chain of a query depends on nothing but its own row, the keys of its sequence and L — not on the batch, the query block or the
// lane it lands in.  Keys >= L: K and V rows are zeros in LDS and the score is -inf, so the weight is expf(-inf) = 0 exactly.
// Query rows >= L repeat row L - 1 and are not stored.  d = 80: the 16 pad columns of the third 32-channel tile of V are zeros
// written into LDS once — global memory past the head's 80 columns is never read, and those accumulator rows are never stored.
constexpr int FA_KT = 64;                          // keys per tile

template <int D>
__global__ __launch_bounds__(256) void attention_f32_kernel(const float* __restrict__ Q, int ldq, const float* __restrict__ K, int ldk,
                                                            const float* __restrict__ V, int ldv, float* __restrict__ O, int ldo, int L,
                                                            float scale) {
  constexpr int KS = D + 1;                        // K row stride: odd, so the 32 rows a fragment column reads fall into 32 banks
  constexpr int NT = (D + 31) / 32;                // 32-channel tiles of V^T
  constexpr int DV = NT * 32;                      // V row stride
  __shared__ float sK[FA_KT * KS];
  __shared__ __attribute__((aligned(16))) float sV[FA_KT * DV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, half = lane >> 5;
  const int h = blockIdx.y;
  const int64_t row0 = (int64_t)blockIdx.z * L;
  const int q0 = blockIdx.x * 128 + wave * 32;
  const bool active = q0 < L;                      // wave-uniform; an idle wave still loads tiles and meets every barrier
  const int qi = min(q0 + li, L - 1);
  if constexpr (DV > D) {
    for (int idx = tid; idx < FA_KT * (DV - D); idx += 256) sV[(idx / (DV - D)) * DV + D + idx % (DV - D)] = 0.f;
  }
  float q[D / 2];                                  // B operand of S^T = K . Q^T: B[k = lane >> 5][j = lane & 31] = Q[j][k]
  {
    const float* qp = Q + (row0 + qi) * ldq + h * D + half;
#pragma unroll
    for (int t = 0; t < D / 2; ++t) q[t] = qp[2 * t];
  }
  f32x16 o[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[nt][r] = 0.f;
  float m = -INFINITY, l = 0.f;                    // running maximum of the query; this HALF's share of the denominator
  for (int k0 = 0; k0 < L; k0 += FA_KT) {
    __syncthreads();                               // the previous tile has been read by every wave
    for (int idx = tid; idx < FA_KT * (D / 4); idx += 256) {
      const int r = idx / (D / 4), c = (idx - r * (D / 4)) * 4;
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
      if (k0 + r < L) {
        kv = *reinterpret_cast<const float4*>(K + (row0 + k0 + r) * ldk + h * D + c);
        vv = *reinterpret_cast<const float4*>(V + (row0 + k0 + r) * ldv + h * D + c);
      }
      float* dk = sK + r * KS + c;
      dk[0] = kv.x; dk[1] = kv.y; dk[2] = kv.z; dk[3] = kv.w;
      *reinterpret_cast<float4*>(sV + r * DV + c) = vv;
    }
    __syncthreads();
    if (!active) continue;
    const int nsub = (L - k0 > 32) ? 2 : 1;        // 32-key subtiles that hold a key
    f32x16 s[FA_KT / 32];
#pragma unroll
    for (int kt = 0; kt < FA_KT / 32; ++kt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kt][r] = 0.f;
      if (kt < nsub) {
        const float* pk = sK + (kt * 32 + li) * KS + half;   // A[i = lane & 31][k = lane >> 5] = K[k0 + 32 kt + i][k]
#pragma unroll
        for (int t = 0; t < D / 2; ++t) s[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(pk[2 * t], q[t], s[kt], 0, 0, 0);
      }
    }
    float mx = m;
#pragma unroll
    for (int kt = 0; kt < FA_KT / 32; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = k0 + kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const float v = (kt < nsub && key < L) ? s[kt][r] * scale : -INFINITY;
        s[kt][r] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));        // key k0 takes part: the maximum is finite from the first tile on
    const float alpha = expf(m - mx);              // first tile: expf(-inf) = 0 on l = 0 and o = 0
    m = mx;
    float psum = 0.f;
#pragma unroll
    for (int kt = 0; kt < FA_KT / 32; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = expf(s[kt][r] - mx);       // a key >= L: expf(-inf) = 0 exactly
        s[kt][r] = p;
        psum += p;
      }
    l = fmaf(l, alpha, psum);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[nt][r] *= alpha;
#pragma unroll
    for (int kt = 0; kt < FA_KT / 32; ++kt)
      if (kt < nsub) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          // A[i = lane & 31][k = lane >> 5] = V[key][32 nt + i]; B[k = lane >> 5][j = lane & 31] = P[query j][key] = s[kt][r]
          const float* pv = sV + (kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * DV + li;
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) o[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(pv[nt * 32], s[kt][r], o[nt], 0, 0, 0);
        }
      }
  }
  if (!active || q0 + li >= L) return;             // no barrier below
  l += __shfl_xor(l, 32, 64);                      // (both halves of a query's lanes are live or gone together)
  const float inv = 1.0f / l;
  // C/D layout: column = lane & 31 (the query), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (channel of the 32-channel tile)
  float* op = O + (row0 + q0 + li) * ldo + h * D;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int ch = nt * 32 + 8 * g + 4 * half;
      if (ch < D)
        *reinterpret_cast<float4*>(op + ch) =
            make_float4(o[nt][4 * g] * inv, o[nt][4 * g + 1] * inv, o[nt][4 * g + 2] * inv, o[nt][4 * g + 3] * inv);
    }
}

// ---- avsd_gelu_f32 --------------------------------------------------------------------------------------------------------------------
// 0.5 x (1 + erf(x / sqrt 2)) with 1 + erf(z) formed as libm's erfc(-z): no cancellation for negative x, 2 for x -> inf and 0 for
// x -> -inf, so +-1e4 give 1e4 and -0
__global__ __launch_bounds__(256) void gelu_f32_kernel(const float* x, float* y, int64_t n) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const float v = x[idx];
  y[idx] = 0.5f * v * erfcf(-v * 0.70710678118654752440f);
}

// ---- avsd_vit_tokens_f32: one thread per output element --------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vit_tokens_f32_kernel(const float* __restrict__ patches, const float* __restrict__ cls,
                                                             const float* __restrict__ pos, float* __restrict__ out, int n, int C, int tail,
                                                             int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t row = idx / C;
  const int c = (int)(idx - row * C);
  const int rows = 1 + n + tail;
  const int64_t b = row / rows;
  const int t = (int)(row - b * rows);
  float v = 0.f;                                   // tail rows
  if (t == 0) v = cls[c] + pos[c];
  else if (t <= n) v = patches[(b * n + (t - 1)) * C + c] + pos[(int64_t)t * C + c];
  out[idx] = v;
}

// ---- avsd_cosine_rows_f32: one wave per row, four rows per block -------------------------------------------------------------------------
// lane j sums elements j, j + 64, .. in ascending order, then the butterfly of wave_sum: one fixed order whatever m and rep
__global__ __launch_bounds__(256) void cosine_rows_f32_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                              float* __restrict__ out, int m, int C, int rep) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= m) return;                              // whole waves leave; no barrier below
  const float* xr = x + (int64_t)i * C;
  const float* yr = y + (int64_t)(i / rep) * C;
  float xy = 0.f, xx = 0.f, yy = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float a = xr[c], b = yr[c];
    xy = fmaf(a, b, xy);
    xx = fmaf(a, a, xx);
    yy = fmaf(b, b, yy);
  }
  xy = wave_sum(xy);
  xx = wave_sum(xx);
  yy = wave_sum(yy);
  if (lane == 0) out[i] = xy / (fmaxf(sqrtf(xx), 1e-12f) * fmaxf(sqrtf(yy), 1e-12f));
}

// ---- avsd_normalize_rows_f32: one wave per row, four rows per block; the summation order of cosine_rows_f32_kernel -------------------
// (x and y may be the same buffer: a lane writes only the elements it has read)
__global__ __launch_bounds__(256) void normalize_rows_f32_kernel(const float* x, float* y, int m, int C) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= m) return;                              // whole waves leave; no barrier below
  const float* xr = x + (int64_t)i * C;
  float* yr = y + (int64_t)i * C;
  float xx = 0.f;
  for (int c = lane; c < C; c += 64) xx = fmaf(xr[c], xr[c], xx);
  const float nrm = fmaxf(sqrtf(wave_sum(xx)), 1e-12f);
  for (int c = lane; c < C; c += 64) yr[c] = xr[c] / nrm;
}

}  // namespace

extern "C" int avsd_attention_f32(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo, int B,
                                  int L, int heads, int d, float scale, void* stream) {
  AVSD_REQUIRE(Q && K && V && O, "attention_f32: null pointer");
  AVSD_REQUIRE(d == 64 || d == 80, "attention_f32: built for head dims 64 and 80, got %d", d);
  AVSD_REQUIRE(L >= 1 && B > 0 && B < 65536 && heads > 0 && heads < 65536 && (int64_t)B * L < (1ll << 24),
               "attention_f32: L >= 1, 0 < B < 65536, 0 < heads < 65536 and B * L < 2^24 are required");
  const int C = heads * d;
  AVSD_REQUIRE(ldq >= C && ldk >= C && ldv >= C && ldo >= C, "attention_f32: row strides must be at least heads * d = %d", C);
  AVSD_REQUIRE(ldk % 4 == 0 && ldv % 4 == 0 && ldo % 4 == 0 && ((uintptr_t)K | (uintptr_t)V | (uintptr_t)O) % 16 == 0,
               "attention_f32: K, V and O must be 16-byte aligned with row strides a multiple of 4");
  const dim3 grid((unsigned)((L + 127) / 128), (unsigned)heads, (unsigned)B);
  if (d == 64)
    hipLaunchKernelGGL(attention_f32_kernel<64>, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), Q, ldq, K, ldk, V, ldv, O, ldo,
                       L, scale);
  else
    hipLaunchKernelGGL(attention_f32_kernel<80>, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), Q, ldq, K, ldk, V, ldv, O, ldo,
                       L, scale);
  AVSD_CHECK_LAUNCH("attention_f32 launch");
  return AVSD_OK;
}

extern "C" int avsd_gelu_f32(const float* x, float* y, int64_t n, void* stream) {
  AVSD_REQUIRE(x && y, "gelu_f32: null pointer");
  AVSD_REQUIRE(n > 0 && (n + 255) / 256 < (1ll << 31), "gelu_f32: n must be positive and below 2^39");
  hipLaunchKernelGGL(gelu_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, y, n);
  AVSD_CHECK_LAUNCH("gelu_f32 launch");
  return AVSD_OK;
}

extern "C" int avsd_vit_tokens_f32(const float* patches, const float* cls, const float* pos, float* out, int B, int n_patches, int C,
                                   int tail_rows, void* stream) {
  AVSD_REQUIRE(patches && cls && pos && out, "vit_tokens_f32: null pointer");
  AVSD_REQUIRE(B > 0 && n_patches > 0 && C > 0 && tail_rows >= 0, "vit_tokens_f32: bad sizes");
  const int64_t total = (int64_t)B * (1 + (int64_t)n_patches + tail_rows) * C;
  AVSD_REQUIRE((total + 255) / 256 < (1ll << 31), "vit_tokens_f32: tensor too large");
  hipLaunchKernelGGL(vit_tokens_f32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     patches, cls, pos, out, n_patches, C, tail_rows, total);
  AVSD_CHECK_LAUNCH("vit_tokens_f32 launch");
  return AVSD_OK;
}

extern "C" int avsd_cosine_rows_f32(const float* x, const float* y, float* out, int m, int C, int rep, void* stream) {
  AVSD_REQUIRE(x && y && out, "cosine_rows_f32: null pointer");
  AVSD_REQUIRE(m > 0 && C > 0 && rep > 0, "cosine_rows_f32: sizes must be positive");
  AVSD_REQUIRE(m % rep == 0, "cosine_rows_f32: rep (%d) must divide m (%d)", rep, m);
  hipLaunchKernelGGL(cosine_rows_f32_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, y, out,
                     m, C, rep);
  AVSD_CHECK_LAUNCH("cosine_rows_f32 launch");
  return AVSD_OK;
}

extern "C" int avsd_normalize_rows_f32(const float* x, float* y, int m, int C, void* stream) {
  AVSD_REQUIRE(x && y, "normalize_rows_f32: null pointer");
  AVSD_REQUIRE(m > 0 && C > 0, "normalize_rows_f32: sizes must be positive");
  hipLaunchKernelGGL(normalize_rows_f32_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, y, m,
                     C);
  AVSD_CHECK_LAUNCH("normalize_rows_f32 launch");
  return AVSD_OK;
}
