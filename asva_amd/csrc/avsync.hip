// AVSync scorer (asva_amd/avsync.py): the kernels of the reference's evaluation classifier — an R(2+1)D-18 video network, a 2-D
// convolutional audio network on the log-mel spectrogram and a 3-layer FC head (avsync/models/{video,audio,head}.py), and the video
// preprocessing of avgen/evaluations/avsync/compute_avsync.py:14-34.  A metric must not move with the storage mode of what it
// measures, so NOTHING here uses the 16-bit type of the build: tensors are f32, products run on the f32-input matrix cores
// (v_mfma_f32_32x32x2_f32, as csrc/gemm_f32.hip), and the bf16 and fp16 libraries compile this file to the same arithmetic.
// Also here, because they share the convolution body: the two kernels Inception-v3 adds for FID (asva_amd/fid.py) — the convolution
// on channel slices of wider buffers (avsd_convnd_ld_f32) and the 3 x 3 pools (avsd_pool3_hw_f32) — and the two kernels I3D adds for
// FVD (asva_amd/fvd.py): the same convolution with "same" padding (avsd_conv3d_same_f32) and the 3-D max pool (avsd_maxpool3d_same_f32).
//
// Layout: channels-last f32, video activations [n][t][h][w][c], audio activations the same with t = 1.
#include "avsd_common.h"

namespace {

// ---- avsd_convnd_f32 -------------------------------------------------------------------------------------------------------------
// Implicit GEMM: row m = (n, to, ho, wo), column = output channel, K = taps * cin (tap-major, cin-minor), gathered from the input
// inside the kernel.  Tile (64 FM) x (64 FN) x 32, 256 threads = 2 x 2 waves, each wave FM x FN accumulator fragments of 32 x 32;
// LDS rows padded to 33 floats as in gemm_f32.hip.  The next K tile is fetched into registers while the matrix cores work on the
// current one.  Every output element is one k-ordered chain 0 .. K-1 whatever the tile and whatever its row index: results do not
// depend on the tile choice or on the batch size.
constexpr int CK = 32, CP = CK + 1;

struct ConvGeom {
  int n, ti, hi, wi, cin, to, ho, wo, cout;
  int kt, kh, kw, st, sh, sw, pt, ph, pw;
  int ldw, relu, M, K;
};
// avsd_convnd_ld_f32: the strides between pixels of x (ldx >= cin) and of out / res (ldy >= cout), in elements; x and out may
// be channel slices of wider channels-last buffers.  The dense kernel does not carry them: its code stays what it was.
struct ConvLd {
  int ldx, ldy;
};

// four consecutive floats at an address that is only 4-byte aligned (the run loader): one global_load_dwordx4
struct __attribute__((packed, aligned(4))) F4U {
  float x, y, z, w;
};

// LD = false: pixels are cin / cout elements apart (avsd_convnd_f32); LD = true: ld.ldx / ld.ldy apart.  Only addresses differ:
// the chain of every output element is the same in both.
// RUN (avsd_conv3d_same_f32 with a small cin and ldx == cin): the kw * cin floats that one (dt, dh) row of the window reads are
// contiguous in memory and in k.  A thread owns four consecutive k as in the float4 loader; where they lie in one run and inside
// the image it fetches them with one 4-byte-aligned wide load, anywhere else (a run boundary, the w borders, the K tail) element by
// element as the scalar loader does.  For x a half wave holds ONE group of four k and 32 rows, so that whether the group straddles a
// run is uniform across it and most waves never enter the element-wise path; neighbouring rows read overlapping addresses (stride *
// cin floats apart).  The LDS tiles hold the same values in the same places for all three loaders.
template <int FM, int FN, bool VEC, bool LD, bool RUN = false>
__device__ __forceinline__ void convnd_f32_body(const float* __restrict__ x, const float* __restrict__ w,
                                                const float* __restrict__ bias, const float* __restrict__ res,
                                                const float* __restrict__ rscale, float* __restrict__ out, const ConvGeom& g,
                                                const ConvLd& ld) {
  const int ldx = LD ? ld.ldx : g.cin, ldy = LD ? ld.ldy : g.cout;
  constexpr int BM = 64 * FM, BN = 64 * FN;
  constexpr bool V4 = VEC || RUN;                 // four consecutive k per thread
  constexpr int NA = V4 ? BM / 32 : BM / 8;       // A elements (float4 / float) each thread fetches per K tile
  constexpr int NW = V4 ? BN / 32 : BN / 8;
  __shared__ float sA[BM * CP];
  __shared__ float sW[BN * CP];
  __shared__ int4 sRow[BM];                        // per tile row: (sample n, to*st - pt, ho*sh - ph, wo*sw - pw)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int M = g.M, K = g.K;

  for (int r = tid; r < BM; r += 256) {
    const int m = m0 + r;
    int4 v = make_int4(0, -(1 << 28), 0, 0);       // rows past M: every tap falls outside the input -> zeros
    if (m < M) {
      int q = m;
      const int wo = q % g.wo; q /= g.wo;
      const int ho = q % g.ho; q /= g.ho;
      const int to = q % g.to; q /= g.to;
      v = make_int4(q, to * g.st - g.pt, ho * g.sh - g.ph, wo * g.sw - g.pw);
    }
    sRow[r] = v;
  }
  __syncthreads();

  f32x16 acc[FM][FN];
#pragma unroll
  for (int a = 0; a < FM; ++a)
#pragma unroll
    for (int b = 0; b < FN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  // VEC (cin % 32 == 0, so a K tile lies inside one tap): thread = (row lr of a 32-row slab, float4 at channel lk)
  // else: thread = (k column tid & 31, row tid >> 5 of an 8-row slab), one float at a time, tap decoded per element
  const int lr = V4 ? tid >> 3 : tid >> 5;
  const int lk = V4 ? (tid & 7) * 4 : tid & 31;
  const int ar = RUN ? tid & 31 : lr;             // the x tile of the run loader: (row ar of a 32-row slab, four k at ak)
  const int ak = RUN ? (tid >> 5) * 4 : lk;
  float4 ra[V4 ? NA : 1], rw[V4 ? NW : 1];
  float fa[V4 ? 1 : NA], fw[V4 ? 1 : NW];

  auto fetch = [&](int k0) {
    if constexpr (RUN) {
      const int k = k0 + ak;
      int edt[4], edh[4], edw[4], ec[4];
      bool ek[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ek[e] = k + e < K;
        const int tap = (k + e) / g.cin;
        ec[e] = k + e - tap * g.cin;
        edw[e] = tap % g.kw;
        edh[e] = (tap / g.kw) % g.kh;
        edt[e] = tap / (g.kw * g.kh);
      }
      // the four k lie in one (dt, dh) row of the window: consecutive floats of x (pixels are cin apart here)
      const bool whole = ek[3] && edt[3] == edt[0] && edh[3] == edh[0];
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int4 rv = sRow[ar + 32 * i];
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        const int t0 = rv.y + edt[0], h0 = rv.z + edh[0];
        if (whole && (unsigned)t0 < (unsigned)g.ti && (unsigned)h0 < (unsigned)g.hi && rv.w + edw[0] >= 0 && rv.w + edw[3] < g.wi) {
          const F4U q = *reinterpret_cast<const F4U*>(x + ((((int64_t)rv.x * g.ti + t0) * g.hi + h0) * g.wi + rv.w + edw[0]) * g.cin + ec[0]);
          v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int t = rv.y + edt[e], h = rv.z + edh[e], ww = rv.w + edw[e];
            if (ek[e] && (unsigned)t < (unsigned)g.ti && (unsigned)h < (unsigned)g.hi && (unsigned)ww < (unsigned)g.wi)
              v[e] = x[((((int64_t)rv.x * g.ti + t) * g.hi + h) * g.wi + ww) * g.cin + ec[e]];
          }
        }
        ra[i] = make_float4(v[0], v[1], v[2], v[3]);
      }
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        const int nn = n0 + lr + 32 * i;
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (nn < g.cout) {
          const int kw0 = k0 + lk;
          const float* pw = w + (int64_t)nn * g.ldw + kw0;
          if (kw0 + 3 < K) {
            q = *reinterpret_cast<const float4*>(pw);
          } else {                    // the K tail: columns >= K of a weight row are never read
            if (kw0 < K) q.x = pw[0];
            if (kw0 + 1 < K) q.y = pw[1];
            if (kw0 + 2 < K) q.z = pw[2];
          }
        }
        rw[i] = q;
      }
    } else if constexpr (VEC) {
      const int tap = k0 / g.cin, c = k0 - tap * g.cin + lk;
      const int dw = tap % g.kw, dh = (tap / g.kw) % g.kh, dt = tap / (g.kw * g.kh);
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int4 rv = sRow[lr + 32 * i];
        const int t = rv.y + dt, h = rv.z + dh, ww = rv.w + dw;
        const bool ok = (unsigned)t < (unsigned)g.ti && (unsigned)h < (unsigned)g.hi && (unsigned)ww < (unsigned)g.wi;
        ra[i] = ok ? *reinterpret_cast<const float4*>(x + ((((int64_t)rv.x * g.ti + t) * g.hi + h) * g.wi + ww) * ldx + c)
                   : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        const int nn = n0 + lr + 32 * i;
        rw[i] = nn < g.cout ? *reinterpret_cast<const float4*>(w + (int64_t)nn * g.ldw + k0 + lk) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    } else {
      const int k = k0 + lk;
      const bool kok = k < K;
      const int tap = k / g.cin, c = k - tap * g.cin;
      const int dw = tap % g.kw, dh = (tap / g.kw) % g.kh, dt = tap / (g.kw * g.kh);
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int4 rv = sRow[lr + 8 * i];
        const int t = rv.y + dt, h = rv.z + dh, ww = rv.w + dw;
        const bool ok = kok && (unsigned)t < (unsigned)g.ti && (unsigned)h < (unsigned)g.hi && (unsigned)ww < (unsigned)g.wi;
        fa[i] = ok ? x[((((int64_t)rv.x * g.ti + t) * g.hi + h) * g.wi + ww) * ldx + c] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        const int nn = n0 + lr + 8 * i;
        fw[i] = (kok && nn < g.cout) ? w[(int64_t)nn * g.ldw + k] : 0.f;
      }
    }
  };
  auto stage = [&]() {
    if constexpr (V4) {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        float* d = sA + (ar + 32 * i) * CP + ak;
        d[0] = ra[i].x; d[1] = ra[i].y; d[2] = ra[i].z; d[3] = ra[i].w;
      }
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        float* d = sW + (lr + 32 * i) * CP + lk;
        d[0] = rw[i].x; d[1] = rw[i].y; d[2] = rw[i].z; d[3] = rw[i].w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < NA; ++i) sA[(lr + 8 * i) * CP + lk] = fa[i];
#pragma unroll
      for (int i = 0; i < NW; ++i) sW[(lr + 8 * i) * CP + lk] = fw[i];
    }
  };

  fetch(0);
  for (int k0 = 0; k0 < K; k0 += CK) {
    __syncthreads();                  // everybody is done reading the previous tile
    stage();
    __syncthreads();
    if (k0 + CK < K) fetch(k0 + CK);
    // operand layout of v_mfma_f32_32x32x2_f32: A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31]
    const float* pa = sA + (wm * 32 * FM + (lane & 31)) * CP + (lane >> 5);
    const float* pw = sW + (wn * 32 * FN + (lane & 31)) * CP + (lane >> 5);
#pragma unroll
    for (int kk = 0; kk < CK; kk += 2) {
      float av[FM], wv[FN];
#pragma unroll
      for (int a = 0; a < FM; ++a) av[a] = pa[a * 32 * CP + kk];
#pragma unroll
      for (int b = 0; b < FN; ++b) wv[b] = pw[b * 32 * CP + kk];
#pragma unroll
      for (int a = 0; a < FM; ++a)
#pragma unroll
        for (int b = 0; b < FN; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], wv[b], acc[a][b], 0, 0, 0);
    }
  }
  // C/D layout: column j = lane & 31 (n), row i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (m)
#pragma unroll
  for (int a = 0; a < FM; ++a)
#pragma unroll
    for (int b = 0; b < FN; ++b) {
      const int nn = n0 + wn * 32 * FN + b * 32 + (lane & 31);
      if (nn >= g.cout) continue;
      const float bv = bias ? bias[nn] : 0.f;
      const float rs = rscale ? rscale[nn] : 1.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 * FM + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= M) continue;
        float v = acc[a][b][r] + bv;
        if (res) v += rs * res[(int64_t)m * ldy + nn];
        if (g.relu) v = fmaxf(v, 0.f);
        out[(int64_t)m * ldy + nn] = v;
      }
    }
}

template <int FM, int FN, bool VEC>
__global__ __launch_bounds__(256) void convnd_f32_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, const float* __restrict__ res,
                                                         const float* __restrict__ rscale, float* __restrict__ out, ConvGeom g) {
  convnd_f32_body<FM, FN, VEC, false>(x, w, bias, res, rscale, out, g, ConvLd{0, 0});
}
template <int FM, int FN, bool VEC>
__global__ __launch_bounds__(256) void convnd_ld_f32_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, const float* __restrict__ res,
                                                            const float* __restrict__ rscale, float* __restrict__ out, ConvGeom g,
                                                            ConvLd ld) {
  convnd_f32_body<FM, FN, VEC, true>(x, w, bias, res, rscale, out, g, ld);
}

template <int FM, int FN>
void launch_conv(bool vec, dim3 grid, hipStream_t s, const float* x, const float* w, const float* bias, const float* res,
                 const float* rscale, float* out, const ConvGeom& g, const ConvLd* ld) {
  if (ld) {
    if (vec) hipLaunchKernelGGL((convnd_ld_f32_kernel<FM, FN, true>), grid, dim3(256), 0, s, x, w, bias, res, rscale, out, g, *ld);
    else hipLaunchKernelGGL((convnd_ld_f32_kernel<FM, FN, false>), grid, dim3(256), 0, s, x, w, bias, res, rscale, out, g, *ld);
  } else {
    if (vec) hipLaunchKernelGGL((convnd_f32_kernel<FM, FN, true>), grid, dim3(256), 0, s, x, w, bias, res, rscale, out, g);
    else hipLaunchKernelGGL((convnd_f32_kernel<FM, FN, false>), grid, dim3(256), 0, s, x, w, bias, res, rscale, out, g);
  }
}

// checks and tile choice shared by avsd_convnd_f32 (ld == nullptr) and avsd_convnd_ld_f32
int convnd_dispatch(const char* who, const float* x, const float* w, const float* bias, const float* res, const float* rscale, float* out,
                    int n, int ti, int hi, int wi, int cin, int to, int ho, int wo, int cout, int kt, int kh, int kw, int st, int sh,
                    int sw, int pt, int ph, int pw, int ldw, int relu, const ConvLd* ld, void* stream) {
  AVSD_REQUIRE(x && w && out, "%s: null pointer", who);
  AVSD_REQUIRE(n > 0 && ti > 0 && hi > 0 && wi > 0 && cin > 0 && cout > 0, "%s: sizes must be positive", who);
  AVSD_REQUIRE(kt > 0 && kh > 0 && kw > 0 && kt <= 16 && kh <= 16 && kw <= 16 && st > 0 && sh > 0 && sw > 0,
               "%s: taps must be 1 .. 16 and strides positive", who);
  AVSD_REQUIRE(pt >= 0 && ph >= 0 && pw >= 0 && pt < kt && ph < kh && pw < kw, "%s: padding must be smaller than the window", who);
  AVSD_REQUIRE(ti + 2 * pt >= kt && hi + 2 * ph >= kh && wi + 2 * pw >= kw, "%s: the window does not fit the padded input", who);
  AVSD_REQUIRE(to == (ti + 2 * pt - kt) / st + 1 && ho == (hi + 2 * ph - kh) / sh + 1 && wo == (wi + 2 * pw - kw) / sw + 1,
               "%s: output size (%d, %d, %d) does not follow from input (%d, %d, %d), window, stride and padding", who, to, ho, wo,
               ti, hi, wi);
  const int64_t K64 = (int64_t)kt * kh * kw * cin, M64 = (int64_t)n * to * ho * wo;
  AVSD_REQUIRE(ldw >= K64, "%s: ldw %d is smaller than K = taps * cin = %lld", who, ldw, (long long)K64);
  AVSD_REQUIRE(M64 < (1ll << 31) && K64 < (1ll << 24) && (int64_t)n * ti * hi * wi < (1ll << 31), "%s: tensor too large", who);
  AVSD_REQUIRE(!rscale || res, "%s: rscale without a residual", who);
  if (ld) {
    AVSD_REQUIRE(ld->ldx >= cin, "%s: ldx %d is smaller than cin %d", who, ld->ldx, cin);
    AVSD_REQUIRE(ld->ldy >= cout, "%s: ldy %d is smaller than cout %d", who, ld->ldy, cout);
  }
  const bool vec = cin % CK == 0 && ldw % 4 == 0 && ((uintptr_t)x | (uintptr_t)w) % 16 == 0 && (!ld || ld->ldx % 4 == 0);
  ConvGeom g{n, ti, hi, wi, cin, to, ho, wo, cout, kt, kh, kw, st, sh, sw, pt, ph, pw, ldw, relu ? 1 : 0, (int)M64, (int)K64};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // tile by shape alone (the result does not depend on it): 64 output channels get a 64-wide tile; a layer too small to give
  // every CU a 128-row tile runs on 64 x 64 tiles
  const int fn = cout <= 64 ? 1 : 2;
  const int64_t big = ((M64 + 127) / 128) * ((cout + 64 * fn - 1) / (64 * fn));
  if (big < 256) {
    dim3 grid((unsigned)((cout + 63) / 64), (unsigned)((M64 + 63) / 64));
    launch_conv<1, 1>(vec, grid, s, x, w, bias, res, rscale, out, g, ld);
  } else if (fn == 1) {
    dim3 grid((unsigned)((cout + 63) / 64), (unsigned)((M64 + 127) / 128));
    launch_conv<2, 1>(vec, grid, s, x, w, bias, res, rscale, out, g, ld);
  } else {
    dim3 grid((unsigned)((cout + 127) / 128), (unsigned)((M64 + 127) / 128));
    launch_conv<2, 2>(vec, grid, s, x, w, bias, res, rscale, out, g, ld);
  }
  AVSD_CHECK_LAUNCH(ld ? "convnd_ld_f32 launch" : "convnd_f32 launch");
  return AVSD_OK;
}

// ---- avsd_conv3d_same_f32 (asva_amd/fvd.py): the body above with TensorFlow "same" zero padding worked out here from input size,
// window and stride.  Only the padding in front enters the geometry: every tap is bounds-checked, and the padding behind is those
// checks.  LOADER 1 scalar, 2 float4, 3 run; the chain of every output element is the same for all of them. ---------------------------
template <int FM, int FN, int LOADER>
__global__ __launch_bounds__(256) void conv3d_same_f32_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, float* __restrict__ out, ConvGeom g,
                                                              ConvLd ld) {
  convnd_f32_body<FM, FN, LOADER == 2, true, LOADER == 3>(x, w, bias, nullptr, nullptr, out, g, ld);
}

template <int FM, int FN>
void launch_conv_same(int loader, dim3 grid, hipStream_t s, const float* x, const float* w, const float* bias, float* out,
                      const ConvGeom& g, const ConvLd& ld) {
  if (loader == 3) hipLaunchKernelGGL((conv3d_same_f32_kernel<FM, FN, 3>), grid, dim3(256), 0, s, x, w, bias, out, g, ld);
  else if (loader == 2) hipLaunchKernelGGL((conv3d_same_f32_kernel<FM, FN, 2>), grid, dim3(256), 0, s, x, w, bias, out, g, ld);
  else hipLaunchKernelGGL((conv3d_same_f32_kernel<FM, FN, 1>), grid, dim3(256), 0, s, x, w, bias, out, g, ld);
}

// TensorFlow "same": the total padding of one axis; pad / 2 of it goes in front, the rest behind; the output is ceil(size / stride)
inline int same_pad_total(int size, int k, int s) {
  const int r = size % s;
  const int p = k - (r == 0 ? s : r);
  return p > 0 ? p : 0;
}

// ---- avsd_maxpool3d_same_f32: window 1 .. 3 and stride 1 .. 2 per axis, "same" padding; one thread per output position and 4
// channels.  A padded position takes part in the maximum as 0.0f (the reference pads with F.pad, then pools unpadded). ------------------
struct PoolGeom {
  int ti, hi, wi, c4, to, ho, wo, ldx, ldy;
  int kt, kh, kw, st, sh, sw, pt, ph, pw;
};
__global__ __launch_bounds__(256) void maxpool3d_same_f32_kernel(const float* __restrict__ x, float* __restrict__ out, PoolGeom g,
                                                                 int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % g.c4);
  int64_t q = idx / g.c4;
  const int ox = (int)(q % g.wo); q /= g.wo;
  const int oy = (int)(q % g.ho); q /= g.ho;
  const int ot = (int)(q % g.to);
  const int64_t n = q / g.to;
  const float* src = x + n * g.ti * g.hi * g.wi * g.ldx + 4 * c;
  float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  for (int dt = 0; dt < g.kt; ++dt) {
    const int t = ot * g.st - g.pt + dt;
    for (int dy = 0; dy < g.kh; ++dy) {
      const int y = oy * g.sh - g.ph + dy;
      for (int dx = 0; dx < g.kw; ++dx) {
        const int xx = ox * g.sw - g.pw + dx;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((unsigned)t < (unsigned)g.ti && (unsigned)y < (unsigned)g.hi && (unsigned)xx < (unsigned)g.wi)
          v = *reinterpret_cast<const float4*>(src + (((int64_t)t * g.hi + y) * g.wi + xx) * g.ldx);
        m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
      }
    }
  }
  *reinterpret_cast<float4*>(out + (((n * g.to + ot) * g.ho + oy) * g.wo + ox) * g.ldy + 4 * c) = m;
}

// ---- avsd_maxpool_hw_f32: (1, 3, 3) window, stride (1, 2, 2), padding (0, 1, 1); one thread per output pixel and 4 channels ---------
__global__ __launch_bounds__(256) void maxpool_hw_f32_kernel(const float* __restrict__ x, float* __restrict__ out, int hi, int wi,
                                                             int c4, int ho, int wo, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % c4);
  int64_t q = idx / c4;
  const int ox = (int)(q % wo); q /= wo;
  const int oy = (int)(q % ho);
  const int64_t img = q / ho;
  const float4* src = reinterpret_cast<const float4*>(x) + img * hi * wi * c4 + c;
  float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);   // padded positions do not take part
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    const int y = 2 * oy - 1 + dy;
    if ((unsigned)y >= (unsigned)hi) continue;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int xx = 2 * ox - 1 + dx;
      if ((unsigned)xx >= (unsigned)wi) continue;
      const float4 v = src[((int64_t)y * wi + xx) * c4];
      m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
    }
  }
  reinterpret_cast<float4*>(out)[idx] = m;
}

// ---- avsd_pool3_hw_f32: 3 x 3 window of Inception-v3 (asva_amd/fid.py), stride S and padding P in {(2, 0), (1, 1)}; one thread per
// output pixel and 4 channels.  Pixels of x are ldx elements apart and pixels of out ldy: either may be a channel slice of a wider
// buffer.  AVG: the taps inside the image are summed in (dy, dx) order and divided by their number (count_include_pad=False);
// otherwise the maximum over them.  Padded positions never take part. -----------------------------------------------------------------
template <bool AVG>
__global__ __launch_bounds__(256) void pool3_hw_f32_kernel(const float* __restrict__ x, float* __restrict__ out, int hi, int wi, int c4,
                                                           int ldx, int ldy, int ho, int wo, int S, int P, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % c4);
  int64_t q = idx / c4;
  const int ox = (int)(q % wo); q /= wo;
  const int oy = (int)(q % ho);
  const int64_t img = q / ho;
  const float* src = x + img * hi * wi * ldx + 4 * c;
  float4 m = AVG ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  int cnt = 0;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    const int y = S * oy - P + dy;
    if ((unsigned)y >= (unsigned)hi) continue;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int xx = S * ox - P + dx;
      if ((unsigned)xx >= (unsigned)wi) continue;
      const float4 v = *reinterpret_cast<const float4*>(src + ((int64_t)y * wi + xx) * ldx);
      if constexpr (AVG) {
        m.x += v.x; m.y += v.y; m.z += v.z; m.w += v.w;
      } else {
        m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
      }
      ++cnt;
    }
  }
  if constexpr (AVG) {
    const float d = (float)cnt;      // >= 1: the entry point admits only windows that meet the image
    m.x /= d; m.y /= d; m.z /= d; m.w /= d;
  }
  *reinterpret_cast<float4*>(out + ((img * ho + oy) * wo + ox) * ldy + 4 * c) = m;
}

// ---- avsd_mean_rows_f32: x [n][rows][c] -> out [n][c].  Thread (channel, quarter q): rows q, q + 4, ... in order, accumulated in
// double so that a long column costs no accuracy; the four partial sums are combined in a fixed order.  No atomics. --------------------
__global__ __launch_bounds__(256) void mean_rows_f32_kernel(const float* __restrict__ x, float* __restrict__ out, int rows, int c) {
  __shared__ double part[4][64];
  const int cl = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int ch = blockIdx.x * 64 + cl;
  const float* src = x + (int64_t)blockIdx.y * rows * c;
  double s = 0.0;
  if (ch < c)
    for (int r = q; r < rows; r += 4) s += (double)src[(int64_t)r * c + ch];
  part[q][cl] = s;
  __syncthreads();
  if (q == 0 && ch < c)
    out[(int64_t)blockIdx.y * c + ch] = (float)(((part[0][cl] + part[1][cl]) + (part[2][cl] + part[3][cl])) / (double)rows);
}

// ---- avsd_resize_aa_normalize_f32: separable antialiased resampling with host-built taps, horizontal pass then vertical ------------
// pass 1: x [img*3][hi][wi] -> tmp [img*3][hi][wo]
__global__ __launch_bounds__(256) void resize_h_f32_kernel(const float* __restrict__ x, float* __restrict__ tmp,
                                                           const int* __restrict__ xs, const int* __restrict__ xn,
                                                           const float* __restrict__ xw, int taps, int wi, int wo, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int ox = (int)(idx % wo);
  const int64_t row = idx / wo;
  const int n = min(max(xn[ox], 0), taps);                     // taps <= wi (checked): a corrupt table cannot leave the row
  const float* src = x + row * wi + min(max(xs[ox], 0), wi - n);
  const float* wt = xw + (int64_t)ox * taps;
  float s = 0.f;
  for (int j = 0; j < n; ++j) s += src[j] * wt[j];
  tmp[idx] = s;
}
// pass 2: tmp -> out [img][ho][wo][3] = (value - mean[c]) / std[c]
__global__ __launch_bounds__(256) void resize_v_norm_f32_kernel(const float* __restrict__ tmp, float* __restrict__ out,
                                                                const int* __restrict__ ys, const int* __restrict__ yn,
                                                                const float* __restrict__ yw, int taps, int hi, int ho, int wo,
                                                                float m0, float m1, float m2, float s0, float s1, float s2,
                                                                int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int ox = (int)(idx % wo);
  int64_t q = idx / wo;
  const int oy = (int)(q % ho); q /= ho;
  const int c = (int)(q % 3);
  const int64_t img = q / 3;
  const int n = min(max(yn[oy], 0), taps);
  const float* src = tmp + ((img * 3 + c) * hi + min(max(ys[oy], 0), hi - n)) * wo + ox;
  const float* wt = yw + (int64_t)oy * taps;
  float s = 0.f;
  for (int j = 0; j < n; ++j) s += src[(int64_t)j * wo] * wt[j];
  const float mean = c == 0 ? m0 : c == 1 ? m1 : m2, sd = c == 0 ? s0 : c == 1 ? s1 : s2;
  out[((img * ho + oy) * wo + ox) * 3 + c] = (s - mean) / sd;
}

}  // namespace

extern "C" int avsd_convnd_f32(const float* x, const float* w, const float* bias, const float* res, const float* rscale, float* out,
                               int n, int ti, int hi, int wi, int cin, int to, int ho, int wo, int cout, int kt, int kh, int kw,
                               int st, int sh, int sw, int pt, int ph, int pw, int ldw, int relu, void* stream) {
  return convnd_dispatch("convnd_f32", x, w, bias, res, rscale, out, n, ti, hi, wi, cin, to, ho, wo, cout, kt, kh, kw, st, sh, sw, pt, ph,
                         pw, ldw, relu, nullptr, stream);
}

extern "C" int avsd_convnd_ld_f32(const float* x, int ldx, const float* w, const float* bias, const float* res, const float* rscale,
                                  float* out, int ldy, int n, int ti, int hi, int wi, int cin, int to, int ho, int wo, int cout, int kt,
                                  int kh, int kw, int st, int sh, int sw, int pt, int ph, int pw, int ldw, int relu, void* stream) {
  const ConvLd ld{ldx, ldy};
  return convnd_dispatch("convnd_ld_f32", x, w, bias, res, rscale, out, n, ti, hi, wi, cin, to, ho, wo, cout, kt, kh, kw, st, sh, sw, pt,
                         ph, pw, ldw, relu, &ld, stream);
}

extern "C" int avsd_conv3d_same_f32(const float* x, int ldx, const float* w, const float* bias, float* out, int ldy, int n, int ti, int hi,
                                    int wi, int cin, int to, int ho, int wo, int cout, int kt, int kh, int kw, int st, int sh, int sw,
                                    int ldw, int relu, int loader, void* stream) {
  AVSD_REQUIRE(x && w && out, "conv3d_same_f32: null pointer");
  AVSD_REQUIRE(n > 0 && ti > 0 && hi > 0 && wi > 0 && cin > 0 && cout > 0, "conv3d_same_f32: sizes must be positive");
  AVSD_REQUIRE(kt > 0 && kh > 0 && kw > 0 && kt <= 16 && kh <= 16 && kw <= 16 && st > 0 && sh > 0 && sw > 0,
               "conv3d_same_f32: taps must be 1 .. 16 and strides positive");
  AVSD_REQUIRE(to == (ti + st - 1) / st && ho == (hi + sh - 1) / sh && wo == (wi + sw - 1) / sw,
               "conv3d_same_f32: output size (%d, %d, %d) is not ceil(input / stride) of input (%d, %d, %d) and stride (%d, %d, %d)", to, ho,
               wo, ti, hi, wi, st, sh, sw);
  const int64_t K64 = (int64_t)kt * kh * kw * cin, M64 = (int64_t)n * to * ho * wo;
  AVSD_REQUIRE(ldw >= K64, "conv3d_same_f32: ldw %d is smaller than K = taps * cin = %lld", ldw, (long long)K64);
  AVSD_REQUIRE(M64 < (1ll << 31) && K64 < (1ll << 24) && (int64_t)n * ti * hi * wi < (1ll << 31), "conv3d_same_f32: tensor too large");
  AVSD_REQUIRE(ldx >= cin, "conv3d_same_f32: ldx %d is smaller than cin %d", ldx, cin);
  AVSD_REQUIRE(ldy >= cout, "conv3d_same_f32: ldy %d is smaller than cout %d", ldy, cout);
  const bool w4 = ldw % 4 == 0 && (uintptr_t)w % 16 == 0;
  const bool can_vec = w4 && cin % CK == 0 && ldx % 4 == 0 && (uintptr_t)x % 16 == 0;
  const bool can_run = w4 && ldx == cin;       // pixels side by side: a (dt, dh) row of the window is one run of kw * cin floats
  AVSD_REQUIRE(loader >= 0 && loader <= 3, "conv3d_same_f32: loader must be 0 (automatic), 1 (scalar), 2 (float4) or 3 (run), got %d", loader);
  AVSD_REQUIRE(loader != 2 || can_vec,
               "conv3d_same_f32: loader 2 (float4) needs cin %% 32 == 0, ldx %% 4 == 0, ldw %% 4 == 0 and 16-byte aligned x and w");
  AVSD_REQUIRE(loader != 3 || can_run, "conv3d_same_f32: loader 3 (run) needs ldx == cin, ldw %% 4 == 0 and a 16-byte aligned w");
  // measured on the stem (cin 3, K 1029, 8 clips of 12 x 224 x 224): scalar 1.26 ms, run 1.29 ms — the layer is bound by its 128 x 64
  // tile, not by its loads (profiles/fvd.md), so the run loader is never picked; it stays selectable for A/Bs
  if (loader == 0) loader = can_vec ? 2 : 1;
  ConvGeom g{n, ti, hi, wi, cin, to, ho, wo, cout, kt, kh, kw, st, sh, sw, same_pad_total(ti, kt, st) / 2, same_pad_total(hi, kh, sh) / 2,
             same_pad_total(wi, kw, sw) / 2, ldw, relu ? 1 : 0, (int)M64, (int)K64};
  const ConvLd ld{ldx, ldy};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // the tile rule of avsd_convnd_f32 (the result does not depend on it)
  const int fn = cout <= 64 ? 1 : 2;
  const int64_t big = ((M64 + 127) / 128) * ((cout + 64 * fn - 1) / (64 * fn));
  if (big < 256) {
    dim3 grid((unsigned)((cout + 63) / 64), (unsigned)((M64 + 63) / 64));
    launch_conv_same<1, 1>(loader, grid, s, x, w, bias, out, g, ld);
  } else if (fn == 1) {
    dim3 grid((unsigned)((cout + 63) / 64), (unsigned)((M64 + 127) / 128));
    launch_conv_same<2, 1>(loader, grid, s, x, w, bias, out, g, ld);
  } else {
    dim3 grid((unsigned)((cout + 127) / 128), (unsigned)((M64 + 127) / 128));
    launch_conv_same<2, 2>(loader, grid, s, x, w, bias, out, g, ld);
  }
  AVSD_CHECK_LAUNCH("conv3d_same_f32 launch");
  return AVSD_OK;
}

extern "C" int avsd_maxpool3d_same_f32(const float* x, int ldx, float* out, int ldy, int n, int ti, int hi, int wi, int c, int to, int ho,
                                       int wo, int kt, int kh, int kw, int st, int sh, int sw, void* stream) {
  AVSD_REQUIRE(x && out, "maxpool3d_same_f32: null pointer");
  AVSD_REQUIRE(n > 0 && ti > 0 && hi > 0 && wi > 0 && c > 0 && c % 4 == 0, "maxpool3d_same_f32: sizes must be positive, channels a multiple of 4");
  AVSD_REQUIRE(kt >= 1 && kh >= 1 && kw >= 1 && kt <= 3 && kh <= 3 && kw <= 3, "maxpool3d_same_f32: windows must be 1 .. 3, got (%d, %d, %d)", kt,
               kh, kw);
  AVSD_REQUIRE(st >= 1 && sh >= 1 && sw >= 1 && st <= 2 && sh <= 2 && sw <= 2, "maxpool3d_same_f32: strides must be 1 .. 2, got (%d, %d, %d)", st,
               sh, sw);
  AVSD_REQUIRE(to == (ti + st - 1) / st && ho == (hi + sh - 1) / sh && wo == (wi + sw - 1) / sw,
               "maxpool3d_same_f32: output size (%d, %d, %d) is not ceil(input / stride) of input (%d, %d, %d) and stride (%d, %d, %d)", to,
               ho, wo, ti, hi, wi, st, sh, sw);
  AVSD_REQUIRE(ldx >= c && ldy >= c && ldx % 4 == 0 && ldy % 4 == 0,
               "maxpool3d_same_f32: ldx %d and ldy %d must be at least c = %d and multiples of 4", ldx, ldy, c);
  AVSD_REQUIRE(((uintptr_t)x | (uintptr_t)out) % 16 == 0, "maxpool3d_same_f32: pointers must be 16-byte aligned");
  const int64_t total = (int64_t)n * to * ho * wo * (c / 4);
  AVSD_REQUIRE((total + 255) / 256 < (1ll << 31) && (int64_t)n * ti * hi * wi < (1ll << 31), "maxpool3d_same_f32: tensor too large");
  const PoolGeom g{ti, hi, wi, c / 4, to, ho, wo, ldx, ldy, kt, kh, kw, st, sh, sw, same_pad_total(ti, kt, st) / 2,
                   same_pad_total(hi, kh, sh) / 2, same_pad_total(wi, kw, sw) / 2};
  hipLaunchKernelGGL(maxpool3d_same_f32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x,
                     out, g, total);
  AVSD_CHECK_LAUNCH("maxpool3d_same_f32 launch");
  return AVSD_OK;
}

extern "C" int avsd_maxpool_hw_f32(const float* x, float* out, int n_img, int hi, int wi, int c, int ho, int wo, void* stream) {
  AVSD_REQUIRE(x && out, "maxpool_hw_f32: null pointer");
  AVSD_REQUIRE(n_img > 0 && hi > 0 && wi > 0 && c > 0 && c % 4 == 0, "maxpool_hw_f32: sizes must be positive, channels a multiple of 4");
  AVSD_REQUIRE(ho == (hi - 1) / 2 + 1 && wo == (wi - 1) / 2 + 1, "maxpool_hw_f32: output size (%d, %d) does not follow from input (%d, %d)", ho,
               wo, hi, wi);
  AVSD_REQUIRE(((uintptr_t)x | (uintptr_t)out) % 16 == 0, "maxpool_hw_f32: pointers must be 16-byte aligned");
  const int64_t total = (int64_t)n_img * ho * wo * (c / 4);
  AVSD_REQUIRE((total + 255) / 256 < (1ll << 31), "maxpool_hw_f32: tensor too large");
  hipLaunchKernelGGL(maxpool_hw_f32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x,
                     out, hi, wi, c / 4, ho, wo, total);
  AVSD_CHECK_LAUNCH("maxpool_hw_f32 launch");
  return AVSD_OK;
}

extern "C" int avsd_pool3_hw_f32(const float* x, int ldx, float* out, int ldy, int n_img, int hi, int wi, int c, int ho, int wo,
                                 int stride, int pad, int avg, void* stream) {
  AVSD_REQUIRE(x && out, "pool3_hw_f32: null pointer");
  AVSD_REQUIRE(n_img > 0 && hi > 0 && wi > 0 && c > 0 && c % 4 == 0, "pool3_hw_f32: sizes must be positive, channels a multiple of 4");
  AVSD_REQUIRE((stride == 2 && pad == 0) || (stride == 1 && pad == 1), "pool3_hw_f32: (stride, padding) must be (2, 0) or (1, 1), got (%d, %d)",
               stride, pad);
  AVSD_REQUIRE(hi + 2 * pad >= 3 && wi + 2 * pad >= 3, "pool3_hw_f32: the window does not fit the padded input (%d, %d)", hi, wi);
  AVSD_REQUIRE(ho == (hi + 2 * pad - 3) / stride + 1 && wo == (wi + 2 * pad - 3) / stride + 1,
               "pool3_hw_f32: output size (%d, %d) does not follow from input (%d, %d), stride %d and padding %d", ho, wo, hi, wi, stride, pad);
  AVSD_REQUIRE(ldx >= c && ldy >= c && ldx % 4 == 0 && ldy % 4 == 0, "pool3_hw_f32: ldx %d and ldy %d must be at least c = %d and multiples of 4",
               ldx, ldy, c);
  AVSD_REQUIRE(((uintptr_t)x | (uintptr_t)out) % 16 == 0, "pool3_hw_f32: pointers must be 16-byte aligned");
  const int64_t total = (int64_t)n_img * ho * wo * (c / 4);
  AVSD_REQUIRE((total + 255) / 256 < (1ll << 31) && (int64_t)n_img * hi * wi < (1ll << 31), "pool3_hw_f32: tensor too large");
  const dim3 grid((unsigned)((total + 255) / 256));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (avg) hipLaunchKernelGGL(pool3_hw_f32_kernel<true>, grid, dim3(256), 0, s, x, out, hi, wi, c / 4, ldx, ldy, ho, wo, stride, pad, total);
  else hipLaunchKernelGGL(pool3_hw_f32_kernel<false>, grid, dim3(256), 0, s, x, out, hi, wi, c / 4, ldx, ldy, ho, wo, stride, pad, total);
  AVSD_CHECK_LAUNCH("pool3_hw_f32 launch");
  return AVSD_OK;
}

extern "C" int avsd_mean_rows_f32(const float* x, float* out, int n, int rows, int c, void* stream) {
  AVSD_REQUIRE(x && out, "mean_rows_f32: null pointer");
  AVSD_REQUIRE(n > 0 && rows > 0 && c > 0 && n < 65536, "mean_rows_f32: sizes must be positive (n < 65536)");
  hipLaunchKernelGGL(mean_rows_f32_kernel, dim3((unsigned)((c + 63) / 64), (unsigned)n), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     x, out, rows, c);
  AVSD_CHECK_LAUNCH("mean_rows_f32 launch");
  return AVSD_OK;
}

extern "C" int avsd_resize_aa_normalize_f32(const float* x, float* tmp, float* out, int n_img, int hi, int wi, int ho, int wo,
                                            const int* y_start, const int* y_count, const float* y_weight, int y_taps,
                                            const int* x_start, const int* x_count, const float* x_weight, int x_taps, int crop,
                                            float mean0, float mean1, float mean2, float std0, float std1, float std2, void* stream) {
  AVSD_REQUIRE(x && tmp && out && y_start && y_count && y_weight && x_start && x_count && x_weight, "resize_aa_normalize_f32: null pointer");
  AVSD_REQUIRE(n_img > 0 && hi > 0 && wi > 0 && ho > 0 && wo > 0 && y_taps > 0 && x_taps > 0 && y_taps <= hi && x_taps <= wi,
               "resize_aa_normalize_f32: sizes must be positive, taps no more than the input size");
  AVSD_REQUIRE(crop == ho && crop == wo, "resize_aa_normalize_f32: the centre crop (%d) must equal the resized size (%d, %d)", crop, ho, wo);
  AVSD_REQUIRE(std0 != 0.f && std1 != 0.f && std2 != 0.f, "resize_aa_normalize_f32: std must not be zero");
  const int64_t t1 = (int64_t)n_img * 3 * hi * wo, t2 = (int64_t)n_img * 3 * ho * wo;
  AVSD_REQUIRE((t1 + 255) / 256 < (1ll << 31) && (t2 + 255) / 256 < (1ll << 31), "resize_aa_normalize_f32: tensor too large");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(resize_h_f32_kernel, dim3((unsigned)((t1 + 255) / 256)), dim3(256), 0, s, x, tmp, x_start, x_count, x_weight, x_taps, wi,
                     wo, t1);
  hipLaunchKernelGGL(resize_v_norm_f32_kernel, dim3((unsigned)((t2 + 255) / 256)), dim3(256), 0, s, tmp, out, y_start, y_count, y_weight,
                     y_taps, hi, ho, wo, mean0, mean1, mean2, std0, std1, std2, t2);
  AVSD_CHECK_LAUNCH("resize_aa_normalize_f32 launch");
  return AVSD_OK;
}
