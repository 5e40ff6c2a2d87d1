// AVSync classifier on a MATRIX of (audio, video) pairs (asva_amd/avsync.py pair_scores): what the reference does with the FC head
// beyond scoring aligned rows — scripts/avsync_eval.py:138-148 (one audio against k videos, k audios against one video) and
// avsync/models/sync_contrastive_trainer.py:35-53 (all k x k pairs of an example, two cross-entropies, two accuracies).
// The head's first layer is linear in cat(a, v): W1 . cat(a_p, v_q) + b1 = Wa . a_p + (Wv . v_q + b1) = U[p] + Vh[q], two
// avsd_convnd_f32 calls on the column halves of the packed W1.  avsd_pair_head_f32 does everything behind that in one launch and
// keeps neither the (pairs, 2 D) concatenation nor the (pairs, H1) hidden layer in memory; avsd_pair_xent_f32 reduces the score
// matrix to the contrastive objective.  f32 only, like csrc/avsync.hip: both libraries compile this file to the same arithmetic.
#include "avsd_common.h"

namespace {

// ---- avsd_pair_head_f32 ------------------------------------------------------------------------------------------------------------
// GEMM rows are pairs m = (g * P + p) * Q + q, columns the H2 units of the second layer, K = H1.  A block owns PR = 32 consecutive
// pairs and all H2 columns; its four waves split the columns, FW fragments of 32 each (wave w: fragments w * FW .. w * FW + FW - 1).
// Per K chunk of 32 the block stages, for each of its pairs, 32 floats of that pair's U row and of its Vh row, and H2 x 32 floats of
// W2 (LDS rows padded to 33 floats as in csrc/avsync.hip); the A operand relu(U + Vh) is formed from the two LDS tiles when the
// fragment is read and exists nowhere else.  The next chunk is fetched into registers while the matrix cores work on this one.
// Epilogue: lane (column j) folds w3[n] * relu(h2[n] + b2[n]) over its fragments in index order, the 32 lanes of a half wave fold by
// xor-shuffles 16, 8, 4, 2, 1, and the four wave sums are added as (s0 + s1) + (s2 + s3), then b3.  Every step is the same for every
// row of the tile and knows nothing of G, P, Q: a pair's score is one fixed chain of (U row, Vh row, weights).
constexpr int PK = 32, PP = PK + 1, PR = 32;

template <int FW>
__global__ __launch_bounds__(256) void pair_head_f32_kernel(const float* __restrict__ U, const float* __restrict__ Vh,
                                                            const float* __restrict__ W2, const float* __restrict__ b2,
                                                            const float* __restrict__ w3, const float* __restrict__ b3,
                                                            float* __restrict__ scores, int P, int Q, int H1, int H2, int ldw2, int M) {
  constexpr int NW = 4 * FW;                         // W2 row slabs of 32 the block stages
  __shared__ float sU[PR * PP];
  __shared__ float sV[PR * PP];
  __shared__ float sW[NW * 32 * PP];
  __shared__ float sPart[4][PR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * PR;
  const int nf = H2 >> 5;

  // loader: thread = (row lr of a 32-row slab, float4 at k offset lk)
  const int lr = tid >> 3, lk = (tid & 7) * 4;
  const int m = m0 + lr;
  const bool ok = m < M;                             // pairs past M: zeros, never read, never written
  const float* pu = U;
  const float* pv = Vh;
  if (ok) {
    const int pq = P * Q;
    const int g = m / pq, rem = m - g * pq;
    const int p = rem / Q, q = rem - p * Q;
    pu = U + ((int64_t)g * P + p) * H1 + lk;
    pv = Vh + ((int64_t)g * Q + q) * H1 + lk;
  }

  f32x16 acc[FW];
#pragma unroll
  for (int f = 0; f < FW; ++f)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[f][r] = 0.f;

  float4 ru, rv, rw[NW];
  auto fetch = [&](int k0) {
    ru = ok ? *reinterpret_cast<const float4*>(pu + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
    rv = ok ? *reinterpret_cast<const float4*>(pv + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int n = lr + 32 * i;
      rw[i] = n < H2 ? *reinterpret_cast<const float4*>(W2 + (int64_t)n * ldw2 + k0 + lk) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto stage = [&]() {
    float* d = sU + lr * PP + lk;
    d[0] = ru.x; d[1] = ru.y; d[2] = ru.z; d[3] = ru.w;
    d = sV + lr * PP + lk;
    d[0] = rv.x; d[1] = rv.y; d[2] = rv.z; d[3] = rv.w;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      d = sW + (lr + 32 * i) * PP + lk;
      d[0] = rw[i].x; d[1] = rw[i].y; d[2] = rw[i].z; d[3] = rw[i].w;
    }
  };

  fetch(0);
  for (int k0 = 0; k0 < H1; k0 += PK) {
    __syncthreads();                  // everybody is done reading the previous chunk
    stage();
    __syncthreads();
    if (k0 + PK < H1) fetch(k0 + PK);
    // operand layout of v_mfma_f32_32x32x2_f32: A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31]
    // No branch in here, so that the next operands are fetched while the matrix cores work: a fragment past H2 multiplies the zero
    // rows the loader staged and is never read by the epilogue.
    const int oa = (lane & 31) * PP + (lane >> 5);
    const float* pw = sW + wave * FW * 32 * PP + oa;
#pragma unroll
    for (int kk = 0; kk < PK; kk += 2) {
      const float a = fmaxf(sU[oa + kk] + sV[oa + kk], 0.f);
      float wv[FW];
#pragma unroll
      for (int f = 0; f < FW; ++f) wv[f] = pw[f * 32 * PP + kk];
#pragma unroll
      for (int f = 0; f < FW; ++f) acc[f] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wv[f], acc[f], 0, 0, 0);
    }
  }

  // C/D layout: column j = lane & 31 (n), row i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (pair)
  float t[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) t[r] = 0.f;
#pragma unroll
  for (int f = 0; f < FW; ++f) {
    const int frag = wave * FW + f;
    if (frag < nf) {
      const int n = frag * 32 + (lane & 31);
      const float bv = b2 ? b2[n] : 0.f, wv = w3[n];
#pragma unroll
      for (int r = 0; r < 16; ++r) t[r] = fmaf(wv, fmaxf(acc[f][r] + bv, 0.f), t[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r)
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) t[r] += __shfl_xor(t[r], o, 64);
  if ((lane & 31) == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) sPart[wave][(r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)] = t[r];
  }
  __syncthreads();
  if (tid < PR && m0 + tid < M)
    scores[m0 + tid] = ((sPart[0][tid] + sPart[1][tid]) + (sPart[2][tid] + sPart[3][tid])) + (b3 ? b3[0] : 0.f);
}

// ---- avsd_pair_xent_f32 ------------------------------------------------------------------------------------------------------------
// Stage 1, grid (G, 2), one wave.  Side 0 walks the P rows of example g (Q scores each, contiguous), side 1 its Q columns (P scores
// each, Q apart).  Per line: lane l takes elements l, l + 64, ... in order; maximum and its lowest index by an xor-shuffle tree on
// (value, index); x = s * inv_tau; sum of exp(x - max) in f32 in the same order and tree; loss = log(sum) + (max - x[label]).
// The products are not contracted into the subtraction: the maximum's own term is exp(0) = 1 exactly.
__global__ __launch_bounds__(64) void pair_xent_lines_kernel(const float* __restrict__ scores, float inv_tau, float* __restrict__ row_loss,
                                                             float* __restrict__ col_loss, int32_t* __restrict__ row_argmax,
                                                             int32_t* __restrict__ col_argmax, int P, int Q) {
#pragma clang fp contract(off)
  const int g = blockIdx.x, side = blockIdx.y, lane = threadIdx.x;
  const int lines = side ? Q : P, len = side ? P : Q;
  const int64_t lstride = side ? 1 : Q, estride = side ? Q : 1;
  float* loss = side ? col_loss : row_loss;
  int32_t* amax = side ? col_argmax : row_argmax;
  const bool want_loss = loss && lines <= len;       // the label of line i is element i
  const float* base = scores + (int64_t)g * P * Q;
  for (int line = 0; line < lines; ++line) {
    const float* src = base + line * lstride;
    float best = -INFINITY;
    int bi = INT32_MAX;
    for (int e = lane; e < len; e += 64) {
      const float v = src[e * estride];
      if (bi == INT32_MAX || v > best) { best = v; bi = e; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi != INT32_MAX && (bi == INT32_MAX || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
    }
    if (lane == 0) amax[(int64_t)g * lines + line] = bi;
    if (!want_loss) continue;
    const float mx = best * inv_tau;
    float sum = 0.f;
    for (int e = lane; e < len; e += 64) sum += expf(src[e * estride] * inv_tau - mx);
    sum = wave_sum(sum);
    if (lane == 0) loss[(int64_t)g * lines + line] = logf(sum) + (mx - src[line * estride] * inv_tau);
  }
}

// Stage 2 (P == Q only), one wave: the G * P line losses and hits, lane l taking entries l, l + 64, ... in order as doubles, an
// xor-shuffle tree in double, one division.
__global__ __launch_bounds__(64) void pair_xent_means_kernel(const float* __restrict__ row_loss, const float* __restrict__ col_loss,
                                                             const int32_t* __restrict__ row_argmax, const int32_t* __restrict__ col_argmax,
                                                             float* __restrict__ means, int n, int P) {
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < n; i += 64) {
    const int label = i % P;
    v[0] += (double)row_loss[i];
    v[1] += (double)col_loss[i];
    v[2] += row_argmax[i] == label ? 1.0 : 0.0;
    v[3] += col_argmax[i] == label ? 1.0 : 0.0;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[j] += __shfl_xor(v[j], o, 64);
    if (threadIdx.x == 0) means[j] = (float)(v[j] / (double)n);
  }
}

bool apart(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x + (uintptr_t)na <= y || y + (uintptr_t)nb <= x;
}

}  // namespace

extern "C" int avsd_pair_head_f32(const float* U, const float* Vh, const float* W2, int ldw2, const float* b2, const float* w3,
                                  const float* b3, float* scores, int G, int P, int Q, int H1, int H2, void* stream) {
  AVSD_REQUIRE(U && Vh && W2 && w3 && scores, "pair_head_f32: null pointer");
  AVSD_REQUIRE(G > 0 && P > 0 && Q > 0, "pair_head_f32: G, P, Q must be positive, got (%d, %d, %d)", G, P, Q);
  AVSD_REQUIRE(H1 > 0 && H1 % 32 == 0, "pair_head_f32: H1 must be a positive multiple of 32, got %d", H1);
  AVSD_REQUIRE(H2 > 0 && H2 % 32 == 0 && H2 <= 256, "pair_head_f32: H2 must be a multiple of 32 in 32 .. 256, got %d", H2);
  AVSD_REQUIRE(ldw2 >= H1 && ldw2 % 4 == 0, "pair_head_f32: ldw2 %d must be at least H1 = %d and a multiple of 4", ldw2, H1);
  AVSD_REQUIRE(((uintptr_t)U | (uintptr_t)Vh | (uintptr_t)W2) % 16 == 0, "pair_head_f32: U, Vh and W2 must be 16-byte aligned");
  AVSD_REQUIRE(((uintptr_t)b2 | (uintptr_t)w3 | (uintptr_t)b3 | (uintptr_t)scores) % 4 == 0, "pair_head_f32: pointers must be 4-byte aligned");
  const int64_t M = (int64_t)G * P * Q;
  AVSD_REQUIRE(M < (1ll << 31) - PR && (int64_t)G * P * H1 < (1ll << 31) && (int64_t)G * Q * H1 < (1ll << 31), "pair_head_f32: tensor too large");
  AVSD_REQUIRE(apart(scores, M * 4, U, (int64_t)G * P * H1 * 4) && apart(scores, M * 4, Vh, (int64_t)G * Q * H1 * 4),
               "pair_head_f32: scores overlaps U or Vh");
  const dim3 grid((unsigned)((M + PR - 1) / PR));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (H2 <= 128)
    hipLaunchKernelGGL(pair_head_f32_kernel<1>, grid, dim3(256), 0, s, U, Vh, W2, b2, w3, b3, scores, P, Q, H1, H2, ldw2, (int)M);
  else
    hipLaunchKernelGGL(pair_head_f32_kernel<2>, grid, dim3(256), 0, s, U, Vh, W2, b2, w3, b3, scores, P, Q, H1, H2, ldw2, (int)M);
  AVSD_CHECK_LAUNCH("pair_head_f32 launch");
  return AVSD_OK;
}

extern "C" int avsd_pair_xent_f32(const float* scores, float inv_tau, float* row_loss, float* col_loss, int32_t* row_argmax,
                                  int32_t* col_argmax, float* means, int G, int P, int Q, void* stream) {
  AVSD_REQUIRE(scores && row_argmax && col_argmax, "pair_xent_f32: null pointer");
  AVSD_REQUIRE(G > 0 && P > 0 && Q > 0, "pair_xent_f32: G, P, Q must be positive, got (%d, %d, %d)", G, P, Q);
  AVSD_REQUIRE((int64_t)G * P * Q < (1ll << 31), "pair_xent_f32: tensor too large");
  AVSD_REQUIRE(inv_tau > 0.f && inv_tau < INFINITY, "pair_xent_f32: 1 / tau must be positive and finite");
  AVSD_REQUIRE(P > Q || row_loss, "pair_xent_f32: row_loss is needed when P <= Q");
  AVSD_REQUIRE(Q > P || col_loss, "pair_xent_f32: col_loss is needed when Q <= P");
  AVSD_REQUIRE(P != Q || means, "pair_xent_f32: means is needed when P == Q");
  AVSD_REQUIRE(((uintptr_t)scores | (uintptr_t)row_loss | (uintptr_t)col_loss | (uintptr_t)row_argmax | (uintptr_t)col_argmax |
                (uintptr_t)means) % 4 == 0, "pair_xent_f32: pointers must be 4-byte aligned");
  const int64_t sbytes = (int64_t)G * P * Q * 4;
  const struct { const void* p; int64_t n; } outs[5] = {{P <= Q ? row_loss : nullptr, (int64_t)G * P * 4}, {Q <= P ? col_loss : nullptr, (int64_t)G * Q * 4},
                                                        {row_argmax, (int64_t)G * P * 4}, {col_argmax, (int64_t)G * Q * 4}, {P == Q ? means : nullptr, 16}};
  for (int i = 0; i < 5; ++i) {
    if (!outs[i].p) continue;
    AVSD_REQUIRE(apart(outs[i].p, outs[i].n, scores, sbytes), "pair_xent_f32: an output overlaps scores");
    for (int j = i + 1; j < 5; ++j)
      AVSD_REQUIRE(!outs[j].p || apart(outs[i].p, outs[i].n, outs[j].p, outs[j].n), "pair_xent_f32: outputs overlap");
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(pair_xent_lines_kernel, dim3((unsigned)G, 2), dim3(64), 0, s, scores, inv_tau, P <= Q ? row_loss : nullptr,
                     Q <= P ? col_loss : nullptr, row_argmax, col_argmax, P, Q);
  AVSD_CHECK_LAUNCH("pair_xent_f32 lines launch");
  if (P == Q) {
    hipLaunchKernelGGL(pair_xent_means_kernel, dim3(1), dim3(64), 0, s, (const float*)row_loss, (const float*)col_loss,
                       (const int32_t*)row_argmax, (const int32_t*)col_argmax, means, G * P, P);
    AVSD_CHECK_LAUNCH("pair_xent_f32 means launch");
  }
  return AVSD_OK;
}
