// CLIP text encoder (asva_amd/text_encoder.py): the kernels of Stable Diffusion 1.5's text_encoder — token + position embedding,
// LayerNorm, causal self-attention and quick-GELU.  The linear layers are avsd_convnd_f32 (csrc/avsync.hip) with taps (1, 1, 1).
// The encoder runs once per clip (77 tokens, 12 layers, about 13 GFLOP) and the reference feeds its output as fp32, so NOTHING here
// uses the 16-bit type of the build: tensors are f32, products run on the f32-input matrix cores (v_mfma_f32_32x32x2_f32, as
// csrc/gemm_f32.hip and csrc/avsync.hip), and the bf16 and fp16 libraries compile this file to the same arithmetic.
#include "avsd_common.h"

#include <math.h>

namespace {

// ---- avsd_embed_tokens_f32: one thread per output element -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void embed_tokens_f32_kernel(const int* __restrict__ ids, const float* __restrict__ tok,
                                                               const float* __restrict__ pos, float* __restrict__ out, int L, int C, int V,
                                                               int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t row = idx / C;
  const int c = (int)(idx - row * C);
  const int id = min(max(ids[row], 0), V - 1);     // the host has checked the range: a corrupt id still cannot leave the table
  out[idx] = tok[(int64_t)id * C + c] + pos[(int64_t)(row % L) * C + c];
}

// ---- avsd_layernorm_f32: one wave per row, four rows per block ---------------------------------------------------------------------
// Two-pass statistics, with the mean kept as a pair: m0 = sum(x) / C rounded to f32, and the correction corr = sum(x - m0) / C that
// this rounding (and the rounding of the long sum) left.  Deviations are formed as (x - m0) - corr — x - m0 is exact for values near
// the mean — so rows with a mean a hundred times their spread lose nothing to cancellation.  Never E[x^2] - E[x]^2.
// (x and y may be the same buffer: a lane writes only the elements it has read)
__global__ __launch_bounds__(256) void layernorm_f32_kernel(const float* x, int ldx, float* y, int ldy, int M, int C,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, float eps) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;                              // whole waves leave; no barrier below
  const float* xr = x + (int64_t)m * ldx;
  float* yr = y + (int64_t)m * ldy;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += xr[c];
  const float m0 = wave_sum(s) / (float)C;
  s = 0.f;
  for (int c = lane; c < C; c += 64) s += xr[c] - m0;
  const float corr = wave_sum(s) / (float)C;
  float q = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float dlt = (xr[c] - m0) - corr;
    q = fmaf(dlt, dlt, q);
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
  for (int c = lane; c < C; c += 64) yr[c] = ((xr[c] - m0) - corr) * rstd * gamma[c] + beta[c];
}

// ---- avsd_quick_gelu_f32 ------------------------------------------------------------------------------------------------------------
// x * sigmoid(1.702 x) with libm's expf and an IEEE division: exp overflows to inf for x < -52 and the quotient is then 0, never NaN
__global__ __launch_bounds__(256) void quick_gelu_f32_kernel(const float* x, float* y, int64_t n) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const float v = x[idx];
  y[idx] = v * (1.0f / (1.0f + expf(-1.702f * v)));
}

// ---- avsd_attention_causal_f32 ------------------------------------------------------------------------------------------------------
// One workgroup per (sequence, head), 256 threads = 4 waves; wave w owns query rows 32 w .. 32 w + 31 and visits key tiles 0 .. w
// only (the tiles above the diagonal are skipped).  K and V of the head live in LDS ([128][64] each, 64 KB together); K is stored
// with its column index XOR (row & 31), so that the 32 rows a fragment column reads fall into 32 different banks without padding.
//
// The first product is computed TRANSPOSED, S^T = K . Q^T: in the C/D layout of v_mfma_f32_32x32x2_f32 (column = lane & 31, row =
// (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) a lane then holds, for ITS query lane & 31, the scores of 16 keys per tile.  The softmax of
// a query is therefore in-lane plus one exchange between the two halves of the wave, and the probabilities are already the A operand
// (A[i = lane & 31][k = lane >> 5]) of the second product if step r of that product takes the two keys (r & 3) + 8 (r >> 2) + {0, 4}:
// no transposition through LDS.  Every output element is one chain in that fixed key order.
constexpr int AD = 64, AL = 128;

__global__ __launch_bounds__(256) void attention_causal_f32_kernel(const float* __restrict__ Q, int ldq, const float* __restrict__ K,
                                                                   int ldk, const float* __restrict__ V, int ldv, float* __restrict__ O,
                                                                   int ldo, int L, int heads, float scale) {
  __shared__ float sK[AL * AD];
  __shared__ float sV[AL * AD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
  const int64_t row0 = (int64_t)b * L;
  const int Lp = (L + 31) & ~31;                   // <= AL (checked by the entry point); rows L .. Lp - 1 are zeros
  for (int idx = tid; idx < Lp * (AD / 4); idx += 256) {
    const int r = idx >> 4, c = (idx & 15) * 4;
    float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
    if (r < L) {
      kv = *reinterpret_cast<const float4*>(K + (row0 + r) * ldk + h * AD + c);
      vv = *reinterpret_cast<const float4*>(V + (row0 + r) * ldv + h * AD + c);
    }
    float* dk = sK + r * AD;
    const int sw = r & 31;
    dk[c ^ sw] = kv.x; dk[(c + 1) ^ sw] = kv.y; dk[(c + 2) ^ sw] = kv.z; dk[(c + 3) ^ sw] = kv.w;
    *reinterpret_cast<float4*>(sV + r * AD + c) = vv;
  }
  __syncthreads();
  const int q0 = wave * 32;
  if (q0 >= L) return;                             // whole waves leave; no barrier below
  const int li = lane & 31, half = lane >> 5;
  const int qi = q0 + li;                          // this lane's query; a row past L repeats row L - 1 and is not stored
  float q[AD / 2];                                 // B operand of S^T = K . Q^T: B[k = lane >> 5][j = lane & 31] = Q[j][k]
  {
    const float* qp = Q + (row0 + min(qi, L - 1)) * ldq + h * AD + half;
#pragma unroll
    for (int t = 0; t < AD / 2; ++t) q[t] = qp[2 * t];
  }
  f32x16 s[AL / 32];
#pragma unroll
  for (int kt = 0; kt < AL / 32; ++kt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) s[kt][r] = 0.f;
    if (kt <= wave) {
      const float* pk = sK + (kt * 32 + li) * AD;   // A[i = lane & 31][k = lane >> 5] = K[32 kt + i][k], column swizzled by i
#pragma unroll
      for (int t = 0; t < AD / 2; ++t) s[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(pk[(2 * t + half) ^ li], q[t], s[kt], 0, 0, 0);
    }
  }
  // softmax over the keys j <= qi, j < L of this lane's query (key 0 always takes part, so the maximum is finite)
  float mx = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < AL / 32; ++kt)
    if (kt <= wave) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const float v = (key <= qi && key < L) ? s[kt][r] * scale : -INFINITY;
        s[kt][r] = v;
        mx = fmaxf(mx, v);
      }
    }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int kt = 0; kt < AL / 32; ++kt)
    if (kt <= wave) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = expf(s[kt][r] - mx);       // a masked key: expf(-inf) = 0 exactly
        s[kt][r] = p;
        sum += p;
      }
    }
  sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.0f / sum;
  f32x16 o[AD / 32];
#pragma unroll
  for (int nt = 0; nt < AD / 32; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[nt][r] = 0.f;
#pragma unroll
  for (int kt = 0; kt < AL / 32; ++kt)
    if (kt <= wave) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = s[kt][r] * inv;
        const float* pv = sV + (kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * AD + li;   // B[k = lane >> 5][j = lane & 31] = V[key][j]
#pragma unroll
        for (int nt = 0; nt < AD / 32; ++nt) o[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(p, pv[nt * 32], o[nt], 0, 0, 0);
      }
    }
  // C/D layout: column = lane & 31 (channel of the head), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (query)
#pragma unroll
  for (int nt = 0; nt < AD / 32; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = q0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (row < L) O[(row0 + row) * ldo + h * AD + nt * 32 + li] = o[nt][r];
    }
}

}  // namespace

extern "C" int avsd_embed_tokens_f32(const int* ids, const float* tok, const float* pos, float* out, int B, int L, int C, int V,
                                     void* stream) {
  AVSD_REQUIRE(ids && tok && pos && out, "embed_tokens_f32: null pointer");
  AVSD_REQUIRE(B > 0 && L > 0 && C > 0 && V > 0, "embed_tokens_f32: sizes must be positive");
  const int64_t total = (int64_t)B * L * C;
  AVSD_REQUIRE((total + 255) / 256 < (1ll << 31) && (int64_t)B * L < (1ll << 31), "embed_tokens_f32: tensor too large");
  hipLaunchKernelGGL(embed_tokens_f32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     ids, tok, pos, out, L, C, V, total);
  AVSD_CHECK_LAUNCH("embed_tokens_f32 launch");
  return AVSD_OK;
}

extern "C" int avsd_layernorm_f32(const float* x, int ldx, float* y, int ldy, int M, int C, const float* gamma, const float* beta,
                                  float eps, void* stream) {
  AVSD_REQUIRE(x && y && gamma && beta, "layernorm_f32: null pointer");
  AVSD_REQUIRE(M > 0 && C > 0 && ldx >= C && ldy >= C, "layernorm_f32: sizes must be positive and row strides at least C");
  AVSD_REQUIRE(eps >= 0.f, "layernorm_f32: eps must not be negative");
  hipLaunchKernelGGL(layernorm_f32_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, ldx, y,
                     ldy, M, C, gamma, beta, eps);
  AVSD_CHECK_LAUNCH("layernorm_f32 launch");
  return AVSD_OK;
}

extern "C" int avsd_attention_causal_f32(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo,
                                         int B, int L, int heads, int d, float scale, void* stream) {
  AVSD_REQUIRE(Q && K && V && O, "attention_causal_f32: null pointer");
  AVSD_REQUIRE(d == AD, "attention_causal_f32: built for head dim 64, got %d", d);
  AVSD_REQUIRE(L >= 1 && L <= AL, "attention_causal_f32: built for 1 <= L <= 128, got %d", L);
  AVSD_REQUIRE(B > 0 && heads > 0 && (int64_t)B * heads < (1ll << 31) && (int64_t)B * L < (1ll << 24),
               "attention_causal_f32: batch and heads must be positive (B * L < 2^24)");
  const int C = heads * d;
  AVSD_REQUIRE(ldq >= C && ldk >= C && ldv >= C && ldo >= C, "attention_causal_f32: row strides must be at least heads * d = %d", C);
  AVSD_REQUIRE(ldk % 4 == 0 && ldv % 4 == 0 && ((uintptr_t)K | (uintptr_t)V) % 16 == 0,
               "attention_causal_f32: K and V must be 16-byte aligned with row strides a multiple of 4");
  hipLaunchKernelGGL(attention_causal_f32_kernel, dim3((unsigned)(B * heads)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), Q, ldq,
                     K, ldk, V, ldv, O, ldo, L, heads, scale);
  AVSD_CHECK_LAUNCH("attention_causal_f32 launch");
  return AVSD_OK;
}

extern "C" int avsd_quick_gelu_f32(const float* x, float* y, int64_t n, void* stream) {
  AVSD_REQUIRE(x && y, "quick_gelu_f32: null pointer");
  AVSD_REQUIRE(n > 0 && (n + 255) / 256 < (1ll << 31), "quick_gelu_f32: n must be positive and below 2^39");
  hipLaunchKernelGGL(quick_gelu_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, y, n);
  AVSD_CHECK_LAUNCH("quick_gelu_f32 launch");
  return AVSD_OK;
}
