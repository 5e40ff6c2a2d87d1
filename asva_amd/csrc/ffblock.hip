// The tail of a 320-channel transformer block as ONE launch (gfx950): avsd_ff_block.
//
//     g   = GEGLU(LayerNorm(h) . W1'^T + b1)          24576 x 2560 x 320   (ff_spatio_audio_temp_transformer_3d.py:361-371)
//     h'  = g . W2^T + b2 + h                         24576 x  320 x 1280
//     out = h' . Wp^T + bp + x                        24576 x  320 x 320   (proj_out + the block input, :151-158)
//
// As three launches g (63 MB at the 32 x 32 level) is written and read back, and so is h' (16 MB); neither is needed by anything
// else.  Here a workgroup owns a band of 96 rows, exactly as nstream_kernel<320, 3, true> (nstream.hip) does — the band of h resident in
// LDS, the LayerNorm statistics of its rows folded once, W1' streamed in MFMA-fragment order straight into registers — and keeps going:
//   * stage 1 runs in 10 rounds of 8 GEGLU fragments = 128 hidden channels; wave w takes fragment 8 t + w: nstream's K loop and its
//     written-out epilogue, unchanged.  What that epilogue used to store — per row fragment b one 16-byte piece per lane: row
//     32 b + (l & 31), hidden channels 16 f + 8 (l >> 5) .. + 7, rounded to 16 bits — IS the B operand of the 32x32x16 MFMA whose
//     k-step is the 16 hidden channels of fragment f.  The wave parks its three pieces in an LDS chunk ([8 k-steps][3][64 lanes] x 16 B
//     = 24 KB: written and read by the same lane index, so conflict-free without padding; two chunks, alternating);
//   * after ONE barrier per round the FF-out units accumulate over the chunk's 8 k-steps, in ascending order.  A unit is one
//     (32-column fragment c of the 10, row fragment b of the 3) accumulator; wave w owns (c = w, b = 0..2) and, for w < 6, also
//     (c = 8 + w / 3, b = w % 3): 4 + 4 or 4 + 3 units on each SIMD, and 14 instead of 30 W2 fragment loads per k-step.  W2 streams
//     in fragment order [10][80][64][8] like W1';
//   * waves 0-3 run the FF-out units of round t - 1 BEFORE the K loop of round t, waves 4-7 AFTER its epilogue: one barrier per round
//     locks the two waves of a SIMD in step, and this way one's GEGLU epilogue (VALU) lies beside the other's matrix work instead of
//     beside the other's epilogue;
//   * stage 2 (template flag): h' = acc + b2 + h with h read from the band, rounded to 16 bits and written OVER the band (dead after
//     the last K loop; every element is read and rewritten by the lane that owns it), one barrier, then the same units over
//     K = 320 with Wp [10][20][64][8]; + bp + x, 16-bit stores.  With the flag off h' is stored and proj_out stays a GEMM.
// Arithmetic: every product accumulates in f32 over K in ascending 16-wide steps and g, h' are rounded to 16 bits where the three
// launches round them; the epilogue terms are added in the shared epilogue's order (gemm_common.h: fold, bias, residual).  The
// results are bit-identical to the three launches on LDS-direct tiles with the unrotated K walk.  No atomics, nothing crosses
// workgroups.  Rows past M are loaded clamped to row M - 1 and never stored.
// LDS: 96 x 656 B band + 2 x 24 KB = 109.5 KB.  C = 320, hidden 1280 only: at C = 640 the 64 bands would need an N split and with it
// a cross-workgroup sum.
#include "avsd_common.h"
#include "band_units.h"

namespace {

typedef unsigned u32x4f __attribute__((ext_vector_type(4)));

struct ffb_args {
  const h16_t* h; int ldh;
  const float* ln_stats; int ln_nblk; float ln_eps;
  const u32x4f* w1; const float* colsum; const float* b1;
  const u32x4f* w2; const float* b2;
  const u32x4f* wp; const float* bp;
  const h16_t* x; int ldx;
  h16_t* out; int ldo;
  int M;
};

constexpr int FB_C = 320, FB_HID = 1280, FB_RF = 3, FB_BM = 32 * FB_RF;
constexpr int FB_KS1 = FB_C / 16;            // k-steps of the GEGLU projection and of proj_out
constexpr int FB_KS2 = FB_HID / 16;          // k-steps of FF-out = GEGLU fragments
constexpr int FB_ROUNDS = FB_KS2 / 8;
constexpr int FB_PITCH = FB_C * 2 + 16;      // 164 dwords = 36 mod 64: ds_read_b128 conflict-free (nstream.hip)
constexpr int FB_BAND = FB_BM * FB_PITCH;
constexpr int FB_CHUNK = 8 * FB_RF * 64 * 16;
constexpr size_t FB_LDS = (size_t)FB_BAND + 2 * FB_CHUNK;
static_assert(FB_BAND % 16 == 0 && FB_LDS <= 160 * 1024, "LDS carve");

template <bool PROJ>
__global__ __launch_bounds__(512, 1) void ffblock_kernel(const ffb_args p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smf[];
  constexpr int KS = FB_KS1, PITCH = FB_PITCH, RF = FB_RF;
  constexpr int D = 10;                      // k-steps of W1' in flight per wave (nstream.hip)
  constexpr int AD = 2;                      // band fragments are read AD k-steps ahead
  constexpr int D2 = 4;                      // k-steps of W2 / Wp in flight per wave and unit column
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = blockIdx.x * FB_BM;
  const int hsel = (lane >> 5) * 4;
  unsigned char* const chunk = smf + FB_BAND;
  // FF-out / proj_out units of this wave: (c0, 0..2) and, below wave 6, (c1, b1)
  const int c0 = wave;
  const bool extra = wave < 6;
  const int c1 = extra ? 8 + wave / 3 : 8, b1 = extra ? wave % 3 : 0;
  const bool late = wave >= 4;

  // LayerNorm fold, first half (nstream.hip): the partial pairs of this lane's rows are requested together, ahead of the band
  constexpr int NPAIR = FB_C / 32;
  float4 lnq[RF][NPAIR / 2];
  const bool ln1 = p.ln_nblk == 1;
#pragma unroll
  for (int b = 0; b < RF; ++b) {
    const float2* st = reinterpret_cast<const float2*>(p.ln_stats) + (int64_t)min(m0 + 32 * b + (lane & 31), p.M - 1) * p.ln_nblk;
    if (ln1) {
      const float2 t = st[0];
      lnq[b][0] = make_float4(t.x, t.y, 0.f, 0.f);
    } else {
#pragma unroll
      for (int j = 0; j < NPAIR / 2; ++j) lnq[b][j] = reinterpret_cast<const float4*>(st)[j];
    }
  }
  const u32x4f* w1base = p.w1 + lane;
  const u32x4f* w2base = p.w2 + lane;
  const unsigned char* arow = smf + (lane & 31) * PITCH + (lane >> 5) * 16;
  // the first D k-steps of W1' are requested before the band: they land while it is staged
  u32x4f wq[D];
#pragma unroll
  for (int d = 0; d < D; ++d) wq[d] = __builtin_nontemporal_load(w1base + ((int64_t)wave * KS + d) * 64);
  // ---- band of h -> LDS, once ---------------------------------------------------------------------------------------------------
  {
    constexpr int V = FB_C / 8;              // 16-byte vectors per row
    constexpr int NV = (FB_BM * V + 511) / 512;
    uint4 xv[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = min(tid + i * 512, FB_BM * V - 1), r = v / V, c = v - r * V;
      xv[i] = *reinterpret_cast<const uint4*>(p.h + (int64_t)min(m0 + r, p.M - 1) * p.ldh + c * 8);      // (rows past M: a copy of the last row, never stored)
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = tid + i * 512, r = v / V, c = v - r * V;
      if (v < FB_BM * V) *reinterpret_cast<uint4*>(smf + r * PITCH + c * 16) = xv[i];
    }
  }
  // ... second half: (rstd, mean * rstd), the arithmetic of ln_row_stats (gemm_common.h) in the same order
  float pre_ln[2 * RF];
#pragma unroll
  for (int b = 0; b < RF; ++b) {
    float sm = 0.f, sq = 0.f;
    if (ln1) { sm += lnq[b][0].x; sq += lnq[b][0].y; }
    else {
#pragma unroll
      for (int j = 0; j < NPAIR / 2; ++j) { sm += lnq[b][j].x; sq += lnq[b][j].y; sm += lnq[b][j].z; sq += lnq[b][j].w; }
    }
    const float inv_k = 1.0f / (float)FB_C;
    const float mean = sm * inv_k;
    const float var = fmaxf(sq * inv_k - mean * mean, 0.f);
    pre_ln[2 * b] = rsqrtf(var + p.ln_eps);
    pre_ln[2 * b + 1] = mean * pre_ln[2 * b];
  }
  f32x16 acc_out[4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc_out[u][r] = 0.f;
  __syncthreads();

  // FF-out over the chunk of round t: k-steps 8 t .. 8 t + 7 of this wave's units, ascending
  auto ffout = [&](int t) {
    const unsigned char* ck = chunk + (t & 1) * FB_CHUNK + lane * 16;
    const u32x4f* wa = w2base + (int64_t)(c0 * FB_KS2 + 8 * t) * 64;
    const u32x4f* wb = w2base + (int64_t)(c1 * FB_KS2 + 8 * t) * 64;
    u32x4f qa[D2], qb[D2];
#pragma unroll
    for (int d = 0; d < D2; ++d) {
      qa[d] = __builtin_nontemporal_load(wa + d * 64);
      if (extra) qb[d] = __builtin_nontemporal_load(wb + d * 64);
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      __builtin_amdgcn_sched_barrier(0);
      h16x8 pc[RF];
#pragma unroll
      for (int b = 0; b < RF; ++b) pc[b] = *reinterpret_cast<const h16x8*>(ck + (s * RF + b) * 1024);
      const h16x8 wf = __builtin_bit_cast(h16x8, qa[s % D2]);
#pragma unroll
      for (int b = 0; b < RF; ++b) acc_out[b] = mfma32x32x16(wf, pc[b], acc_out[b], 0, 0, 0);
      if (s + D2 < 8) qa[s % D2] = __builtin_nontemporal_load(wa + (s + D2) * 64);
      if (extra) {
        const h16x8 px = *reinterpret_cast<const h16x8*>(ck + (s * RF + b1) * 1024);
        acc_out[3] = mfma32x32x16(__builtin_bit_cast(h16x8, qb[s % D2]), px, acc_out[3], 0, 0, 0);
        if (s + D2 < 8) qb[s % D2] = __builtin_nontemporal_load(wb + (s + D2) * 64);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  // ---- stage 1: 10 rounds of (GEGLU fragment 8 t + wave -> chunk, barrier, FF-out units over the chunk) -------------------------
  for (int t = 0; t < FB_ROUNDS; ++t) {
    const int f = 8 * t + wave;
    const int fnext = t + 1 < FB_ROUNDS ? f + 8 : f;          // past the end: re-read this fragment (never consumed)
    const u32x4f* wcur = w1base + (int64_t)f * KS * 64;
    const u32x4f* wnxt = w1base + (int64_t)fnext * KS * 64;
    if (!late && t > 0) ffout(t - 1);
    f32x16 acc[RF];
#pragma unroll
    for (int b = 0; b < RF; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
    float4 cs4[4], bi4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      cs4[q] = *reinterpret_cast<const float4*>(p.colsum + f * 32 + 8 * q + hsel);
      bi4[q] = *reinterpret_cast<const float4*>(p.b1 + f * 32 + 8 * q + hsel);
    }
    // (the scheduling barriers keep hipcc from hoisting every fragment read of the unrolled loop to its top: nstream.hip)
    h16x8 af[AD + 1][RF];
#pragma unroll
    for (int j = 0; j < AD; ++j)
#pragma unroll
      for (int b = 0; b < RF; ++b) af[j][b] = *reinterpret_cast<const h16x8*>(arow + b * 32 * PITCH + j * 32);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      __builtin_amdgcn_sched_barrier(0);
      const h16x8 wf = __builtin_bit_cast(h16x8, wq[ks % D]);
      if (ks + AD < KS) {
#pragma unroll
        for (int b = 0; b < RF; ++b) af[(ks + AD) % (AD + 1)][b] = *reinterpret_cast<const h16x8*>(arow + b * 32 * PITCH + (ks + AD) * 32);
      }
#pragma unroll
      for (int b = 0; b < RF; ++b) acc[b] = mfma32x32x16(wf, af[ks % (AD + 1)][b], acc[b], 0, 0, 0);
      wq[ks % D] = __builtin_nontemporal_load(ks + D < KS ? wcur + (ks + D) * 64 : wnxt + (ks + D - KS) * 64);
    }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(0);
    // nstream's GEGLU epilogue; the piece goes to the chunk instead of to memory
    unsigned char* cw = chunk + (t & 1) * FB_CHUNK + (wave * RF * 64 + lane) * 16;
#pragma unroll
    for (int b = 0; b < RF; ++b) {
      const float rstd = pre_ln[2 * b], mr = pre_ln[2 * b + 1];
      float v[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float c4[4] = {cs4[q].x, cs4[q].y, cs4[q].z, cs4[q].w}, b4[4] = {bi4[q].x, bi4[q].y, bi4[q].z, bi4[q].w};
#pragma unroll
        for (int i = 0; i < 4; ++i) v[4 * q + i] = fmaf(acc[b][4 * q + i] + 0.f, rstd, -mr * c4[i]) + b4[i];
      }
      unsigned e0[2], e1[2];
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const float g00 = v[2 * d] * gelu_erf_f(v[8 + 2 * d]), g01 = v[2 * d + 1] * gelu_erf_f(v[8 + 2 * d + 1]);
        const float g10 = v[4 + 2 * d] * gelu_erf_f(v[12 + 2 * d]), g11 = v[4 + 2 * d + 1] * gelu_erf_f(v[12 + 2 * d + 1]);
        const auto e = __builtin_amdgcn_permlane32_swap(pack2h(g00, g01), pack2h(g10, g11), false, false);
        e0[d] = e[0]; e1[d] = e[1];
      }
      *reinterpret_cast<uint4*>(cw + b * 1024) = make_uint4(e0[0], e0[1], e1[0], e1[1]);     // hidden channels 16 f + 2 hsel .. + 7 of row 32 b + (lane & 31)
    }
    if (late && t > 0) ffout(t - 1);
    __syncthreads();
  }
  ffout(FB_ROUNDS - 1);

  // ---- h' = acc + b2 + h, rounded: over the band (stage 2) or to memory ----------------------------------------------------------
  const int frow = lane & 31;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (u == 3 && !extra) break;
    const int c = u < 3 ? c0 : c1, b = u < 3 ? u : b1;
    unsigned char* rp = smf + (32 * b + frow) * PITCH + (32 * c + 4 * hsel) * 2;
    const uint4 rlo = *reinterpret_cast<const uint4*>(rp), rhi = *reinterpret_cast<const uint4*>(rp + 16);
    uint4 lo, hi;
    unit_finish(acc_out[u], p.b2 + 32 * c, hsel, rlo, rhi, lo, hi);
    if constexpr (PROJ) {
      *reinterpret_cast<uint4*>(rp) = lo;
      *reinterpret_cast<uint4*>(rp + 16) = hi;
    } else {
      const int m = m0 + 32 * b + frow;
      if (m < p.M) {
        h16_t* op = p.out + (int64_t)m * p.ldo + 32 * c + 4 * hsel;
        *reinterpret_cast<uint4*>(op) = lo;
        *reinterpret_cast<uint4*>(op + 8) = hi;
      }
    }
  }
  if constexpr (PROJ) {
    __syncthreads();
    // ---- stage 2: out = h' . Wp^T + bp + x, the same units over K = 320 -------------------------------------------------------------
    // (opaque copies: everything below that is derived from the lane and the band is loop-invariant, and hipcc hoists it over the
    //  whole of stage 1, where the registers are spoken for — 5 spilled; nstream.hip has the same note)
    int lanev = lane, m0v = m0;
    asm volatile("" : "+v"(lanev), "+s"(m0v));
    const int frow = lanev & 31, hsel = (lanev >> 5) * 4;
    const unsigned char* arow = smf + frow * PITCH + (lanev >> 5) * 16;
    const u32x4f* wa = p.wp + lanev + (int64_t)c0 * KS * 64;
    const u32x4f* wb = p.wp + lanev + (int64_t)c1 * KS * 64;
    const unsigned char* arow1 = arow + b1 * 32 * PITCH;
    u32x4f qa[D2], qb[D2];
#pragma unroll
    for (int d = 0; d < D2; ++d) {
      qa[d] = __builtin_nontemporal_load(wa + d * 64);
      if (extra) qb[d] = __builtin_nontemporal_load(wb + d * 64);
    }
    // the block input's rows of this wave's units: requested ahead of the K loop
    uint4 xr[4][2];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = u < 3 ? c0 : c1, b = u < 3 ? u : b1;
      const h16_t* xp = p.x + (int64_t)min(m0v + 32 * b + frow, p.M - 1) * p.ldx + 32 * c + 4 * hsel;
      xr[u][0] = xr[u][1] = make_uint4(0u, 0u, 0u, 0u);
      if (u < 3 || extra) {
        xr[u][0] = *reinterpret_cast<const uint4*>(xp);
        xr[u][1] = *reinterpret_cast<const uint4*>(xp + 8);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc_out[u][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      __builtin_amdgcn_sched_barrier(0);
      h16x8 hf[RF];
#pragma unroll
      for (int b = 0; b < RF; ++b) hf[b] = *reinterpret_cast<const h16x8*>(arow + b * 32 * PITCH + ks * 32);
      const h16x8 wf = __builtin_bit_cast(h16x8, qa[ks % D2]);
#pragma unroll
      for (int b = 0; b < RF; ++b) acc_out[b] = mfma32x32x16(wf, hf[b], acc_out[b], 0, 0, 0);
      if (ks + D2 < KS) qa[ks % D2] = __builtin_nontemporal_load(wa + (ks + D2) * 64);
      if (extra) {
        const h16x8 hx = *reinterpret_cast<const h16x8*>(arow1 + ks * 32);
        acc_out[3] = mfma32x32x16(__builtin_bit_cast(h16x8, qb[ks % D2]), hx, acc_out[3], 0, 0, 0);
        if (ks + D2 < KS) qb[ks % D2] = __builtin_nontemporal_load(wb + (ks + D2) * 64);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (u == 3 && !extra) break;
      const int c = u < 3 ? c0 : c1, b = u < 3 ? u : b1;
      uint4 lo, hi;
      unit_finish(acc_out[u], p.bp + 32 * c, hsel, xr[u][0], xr[u][1], lo, hi);
      const int m = m0v + 32 * b + frow;
      if (m < p.M) {
        h16_t* op = p.out + (int64_t)m * p.ldo + 32 * c + 4 * hsel;
        *reinterpret_cast<uint4*>(op) = lo;
        *reinterpret_cast<uint4*>(op + 8) = hi;
      }
    }
  }
}

// the lower bound on M: at M = 24576 (256 bands, one per CU) the fused launch measured 94 us against 121 us for the three launches, at
// M = 12288 (128 bands: half the CUs idle, where the tiled GEMMs still fill the chip) 82 us against 69 us (profiles/ffblock_kernel_trace.md)
constexpr int FB_MIN_M = 24576;

template <bool PROJ>
int launch_ffblock(const ffb_args& a, hipStream_t s) {
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ffblock_kernel<PROJ>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FB_LDS);
    if (e != hipSuccess) {
      avsd_set_error("ff_block: hipFuncSetAttribute(%zu B LDS): %s", FB_LDS, hipGetErrorString(e));
      return AVSD_ELAUNCH;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL((ffblock_kernel<PROJ>), dim3((unsigned)((a.M + FB_BM - 1) / FB_BM)), dim3(512), FB_LDS, s, a);
  AVSD_CHECK_LAUNCH("ff_block launch");
  return AVSD_OK;
}

}  // namespace

extern "C" int avsd_ff_block_supported(int M, int C, int with_proj_out) {
  (void)with_proj_out;          // both forms are built and both measured faster than what they replace
  return C == FB_C && M >= FB_MIN_M ? 1 : 0;
}

extern "C" int avsd_ff_block(const void* h, int ldh, const float* ln_stats, int ln_nblk, float ln_eps, const void* w1_frag,
                             const float* w1_colsum, const float* b1, const void* w2_frag, const float* b2, const void* wp_frag,
                             const float* bp, const void* x, int ldx, void* out, int ldo, int M, int C, void* stream) {
  AVSD_REQUIRE(C == FB_C, "ff_block: unsupported shape: built for C = 320 (hidden 1280) only, got C = %d", C);
  AVSD_REQUIRE(M > 0, "ff_block: unsupported shape: M = %d", M);
  AVSD_REQUIRE(h && ln_stats && w1_frag && w1_colsum && b1 && w2_frag && b2 && out, "ff_block: null operand");
  AVSD_REQUIRE(ln_nblk == FB_C / 32 || ln_nblk == 1, "ff_block: ln_nblk must be C / 32 or 1 (pre-folded), got %d", ln_nblk);
  AVSD_REQUIRE(ldh >= C && ldo >= C && ldh % 8 == 0 && ldo % 8 == 0, "ff_block: unsupported strides: ldh %d and ldo %d must be multiples of 8, at least C", ldh, ldo);
  AVSD_REQUIRE(((uintptr_t)h | (uintptr_t)out | (uintptr_t)x | (uintptr_t)w1_frag | (uintptr_t)w2_frag | (uintptr_t)wp_frag | (uintptr_t)w1_colsum |
                (uintptr_t)b1 | (uintptr_t)b2 | (uintptr_t)bp | (uintptr_t)ln_stats) % 16 == 0, "ff_block: operands must be 16-byte aligned");
  if (wp_frag) {
    AVSD_REQUIRE(bp && x, "ff_block: proj_out needs its bias and the block input");
    AVSD_REQUIRE(ldx >= C && ldx % 8 == 0, "ff_block: unsupported strides: ldx %d must be a multiple of 8, at least C", ldx);
  }
  ffb_args a;
  a.h = reinterpret_cast<const h16_t*>(h); a.ldh = ldh;
  a.ln_stats = ln_stats; a.ln_nblk = ln_nblk; a.ln_eps = ln_eps;
  a.w1 = reinterpret_cast<const u32x4f*>(w1_frag); a.colsum = w1_colsum; a.b1 = b1;
  a.w2 = reinterpret_cast<const u32x4f*>(w2_frag); a.b2 = b2;
  a.wp = reinterpret_cast<const u32x4f*>(wp_frag); a.bp = bp;
  a.x = reinterpret_cast<const h16_t*>(x); a.ldx = ldx;
  a.out = reinterpret_cast<h16_t*>(out); a.ldo = ldo;
  a.M = M;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return wp_frag ? launch_ffblock<true>(a, s) : launch_ffblock<false>(a, s);
}
