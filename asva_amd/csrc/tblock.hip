// The temporal attention of a 320-channel transformer block as ONE launch (gfx950): avsd_temporal_block.
//
//     qkv = LayerNorm(h + pos[frame]) . Wqkv'^T + b       M x 960 x 320   (ff_spatio_audio_temp_transformer_3d.py:346-358)
//     o   = softmax(q k^T / sqrt d) v                      over the 12 frames of a pixel, per head (8 heads of d = 40)
//     h'  = o . Wo^T + bo + h                              M x 320 x 320, + the LayerNorm row statistics of h'
//
// As three launches qkv (47 MB at the 32 x 32 level) and o (16 MB) are written and read back, and nothing else reads them.  The 12
// frames of a pixel attend only to each other, so a band of 8 pixel columns x 12 frames = 96 rows is self-contained: one workgroup
// owns it, with the machinery of ffblock.hip — the band of h resident in LDS, the LayerNorm statistics of its rows folded once, the
// weights streamed in MFMA-fragment order straight into registers, stage-2 units that accumulate over LDS chunks.
//   * band: column c of the B hw columns is (batch c / hw, pixel c % hw); band row r = 8 f + j is frame f of column 8 blockIdx.x + j,
//     global row (batch 12 + f) hw + pixel, as tattn_kernel (attention.hip) addresses it.  Row fragment b holds frames 4 b .. 4 b + 3.
//     Columns past B hw are loaded clamped and never stored; a band may straddle a batch boundary (every row has its own address);
//   * stage 1 walks the q|k|v columns in 4 groups of 2 heads.  The column order of Wqkv' is free, q|k|v never leaves the chip: the
//     host packs, per group, [q | k | v] of its two heads = 240 columns padded with zeros to 256 = 8 fragments (weights.group_qkv),
//     and wave w runs fragment 8 g + w — nstream's K loop.  The epilogue is the shared LayerNorm fold with ln_rowvec
//     (gemm_common.h): fmaf(acc + posw[frame][n], rstd, -mean rstd colsum[n]), + bias, rounded to 16 bits, into an LDS chunk
//     [96 rows][256 columns] (pitch 528 B = 4 banks mod 64);
//   * attention of the group, after one barrier: 192 (row, head) items on 2 lanes each (waves 0-5).  An item computes what a
//     tattn_kernel<40, 12, false, true> thread computes: per key two dot2h chains over the 5 vectors in its order, the max over the
//     scaled scores, __expf of fma(dot, scale, -max) (the form hipcc gives that instantiation), the sum in key order, o = sum_j p_j v_j
//     by fmaf in key order, . 1 / sum, rounded.  The two lanes of an item compute the even / the odd keys' scores (whole chains) and
//     trade them, then each runs P.V for 20 of the 40 channels (every output channel is a sum of its own).  The rounded o goes to an
//     LDS chunk in the layout of the B operand of the 32x32x16 MFMA: it IS k-steps 5 g .. 5 g + 4 of the output projection
//     ([5][3][64 lanes] x 16 B = 15 KB; one chunk: its readers finish before the barrier ahead of the next attention);
//   * stage 2: ffblock's units — wave w owns column fragment w for the three row fragments and, below wave 6, one unit of fragments
//     8-9 — accumulate the k-steps of group g - 1 while group g is projected (waves 0-3 before their K loop, waves 4-7 after their
//     epilogue), Wo streamed in fragment order [10][20][64][8]: K ascending over heads 0..7;
//   * h' = acc + bo + h with h from the band, rounded, 16-bit stores, and per 32-column block the (sum, sum of squares) of the
//     rounded values as AVSD_GEMM_ROWSTATS writes them.
// Every value is rounded where the three launches round it and every sum runs in their order: bit-identical to them on LDS-direct
// tiles with the unrotated K walk.  No atomics, nothing crosses workgroups, two barriers per group.
// LDS: 96 x 656 B band + 96 x 528 B q|k|v chunk + 15 KB = 126 KB.  C = 320, 8 heads, 12 frames only: at C = 640 / 1280 the 64 / 16
// bands cannot fill the chip.
#include "gemm_common.h"
#include "band_units.h"

namespace {

typedef unsigned u32x4t __attribute__((ext_vector_type(4)));

struct tb_args {
  const h16_t* h; int ldh;
  const float* ln_stats; int ln_nblk; float ln_eps;
  const u32x4t* wqkv; const float* colsum; const float* bias; const float* posw;      // grouped column order: [1024], posw [12][1024]
  const u32x4t* wo; const float* bo;
  h16_t* out; int ldo;
  float* rowstats;
  int ncol, hw;              // ncol = B hw pixel columns
  float scale;
};

constexpr int TB_C = 320, TB_HEADS = 8, TB_D = 40, TB_F = 12, TB_PIX = 8, TB_RF = 3, TB_BM = TB_PIX * TB_F;
constexpr int TB_KS = TB_C / 16;                 // k-steps of both projections
constexpr int TB_GROUPS = 4;                     // of 2 heads
constexpr int TB_GN = 256;                       // q|k|v columns of a group: 3 x 80 = 240, padded to 8 fragments
constexpr int TB_NQKV = TB_GROUPS * TB_GN;
constexpr int TB_OKS = 2 * TB_D / 16;            // k-steps of Wo a group's o covers
constexpr int TB_PITCH = TB_C * 2 + 16;          // band rows: 164 dwords = 36 mod 64 (nstream.hip)
constexpr int TB_BAND = TB_BM * TB_PITCH;
constexpr int TB_CPITCH = TB_GN * 2 + 16;        // q|k|v chunk rows: 132 dwords = 4 mod 64
constexpr int TB_CHUNK = TB_BM * TB_CPITCH;
constexpr int TB_OCHUNK = TB_OKS * TB_RF * 64 * 16;
constexpr size_t TB_LDS = (size_t)TB_BAND + TB_CHUNK + TB_OCHUNK;
static_assert(TB_BM == 32 * TB_RF && TB_BAND % 16 == 0 && TB_CHUNK % 16 == 0 && TB_LDS <= 160 * 1024, "LDS carve");
static_assert(TB_GROUPS * TB_OKS == TB_KS && TB_GROUPS * 2 == TB_HEADS, "groups of 2 heads");

__global__ __launch_bounds__(512, 1) void tblock_kernel(const tb_args p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smt[];
  constexpr int KS = TB_KS, PITCH = TB_PITCH, CPITCH = TB_CPITCH, RF = TB_RF;
  constexpr int D = 10;                      // k-steps of Wqkv' in flight per wave (nstream.hip)
  constexpr int AD = 2;                      // band fragments are read AD k-steps ahead
  constexpr int D2 = 4;                      // k-steps of Wo in flight per wave and unit column
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col0 = blockIdx.x * TB_PIX;
  const int hsel = (lane >> 5) * 4;
  const int frow = lane & 31;
  unsigned char* const chunk = smt + TB_BAND;
  unsigned char* const ochunk = chunk + TB_CHUNK;
  // output-projection units of this wave: (c0, 0..2) and, below wave 6, (c1, b1)
  const int c0 = wave;
  const bool extra = wave < 6;
  const int c1 = extra ? 8 + wave / 3 : 8, b1 = extra ? wave % 3 : 0;
  const bool late = wave >= 4;

  // global rows of this lane's three band rows 32 b + frow: frame 4 b + (frow >> 3) of column col0 + (frow & 7)
  auto rows_of = [&](int fr, int (&grow)[RF]) {
    const int cc = min(col0 + (fr & 7), p.ncol - 1), bb = cc / p.hw, pix = cc - bb * p.hw;
#pragma unroll
    for (int b = 0; b < RF; ++b) grow[b] = (bb * TB_F + 4 * b + (fr >> 3)) * p.hw + pix;
  };
  // LayerNorm fold, first half (nstream.hip): the partial pairs of this lane's rows are requested together, ahead of the band
  constexpr int NPAIR = TB_C / 32;
  float4 lnq[RF][NPAIR / 2];
  const bool ln1 = p.ln_nblk == 1;
#pragma unroll
  for (int b = 0; b < RF; ++b) {
    int grow[RF];
    rows_of(frow, grow);
    const float2* st = reinterpret_cast<const float2*>(p.ln_stats) + (int64_t)grow[b] * p.ln_nblk;
    if (ln1) {
      const float2 t = st[0];
      lnq[b][0] = make_float4(t.x, t.y, 0.f, 0.f);
    } else {
#pragma unroll
      for (int j = 0; j < NPAIR / 2; ++j) lnq[b][j] = reinterpret_cast<const float4*>(st)[j];
    }
  }
  const u32x4t* w1base = p.wqkv + lane;
  const unsigned char* arow = smt + frow * PITCH + (lane >> 5) * 16;
  // the first D k-steps of Wqkv' are requested before the band: they land while it is staged
  u32x4t wq[D];
#pragma unroll
  for (int d = 0; d < D; ++d) wq[d] = __builtin_nontemporal_load(w1base + ((int64_t)wave * KS + d) * 64);
  // ---- band of h -> LDS, once ---------------------------------------------------------------------------------------------------
  {
    constexpr int V = TB_C / 8;              // 16-byte vectors per row
    constexpr int NV = (TB_BM * V + 511) / 512;
    uint4 xv[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = min(tid + i * 512, TB_BM * V - 1), r = v / V, c = v - r * V;
      const int cc = min(col0 + (r & 7), p.ncol - 1), bb = cc / p.hw, pix = cc - bb * p.hw;      // (columns past B hw: a copy of the last one, never stored)
      xv[i] = *reinterpret_cast<const uint4*>(p.h + (int64_t)((bb * TB_F + (r >> 3)) * p.hw + pix) * p.ldh + c * 8);
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = tid + i * 512, r = v / V, c = v - r * V;
      if (v < TB_BM * V) *reinterpret_cast<uint4*>(smt + r * PITCH + c * 16) = xv[i];
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
    const float inv_k = 1.0f / (float)TB_C;
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

  // output projection over the o chunk of group g: k-steps 5 g .. 5 g + 4 of this wave's units, ascending
  auto oproj = [&](int g) {
    int laneo = lane;
    asm volatile("" : "+v"(laneo));          // (opaque: or the addresses below live through the K loop, where the registers are spoken for)
    const unsigned char* ck = ochunk + laneo * 16;
    const u32x4t* wa = p.wo + laneo + (int64_t)(c0 * KS + TB_OKS * g) * 64;
    const u32x4t* wb = p.wo + laneo + (int64_t)(c1 * KS + TB_OKS * g) * 64;
    u32x4t qa[D2], qb[D2];
#pragma unroll
    for (int d = 0; d < D2; ++d) {
      qa[d] = __builtin_nontemporal_load(wa + d * 64);
      if (extra) qb[d] = __builtin_nontemporal_load(wb + d * 64);
    }
#pragma unroll
    for (int s = 0; s < TB_OKS; ++s) {
      __builtin_amdgcn_sched_barrier(0);
      h16x8 pc[RF];
#pragma unroll
      for (int b = 0; b < RF; ++b) pc[b] = *reinterpret_cast<const h16x8*>(ck + (s * RF + b) * 1024);
      const h16x8 wf = __builtin_bit_cast(h16x8, qa[s % D2]);
#pragma unroll
      for (int b = 0; b < RF; ++b) acc_out[b] = mfma32x32x16(wf, pc[b], acc_out[b], 0, 0, 0);
      if (s + D2 < TB_OKS) qa[s % D2] = __builtin_nontemporal_load(wa + (s + D2) * 64);
      if (extra) {
        const h16x8 px = *reinterpret_cast<const h16x8*>(ck + (s * RF + b1) * 1024);
        acc_out[3] = mfma32x32x16(__builtin_bit_cast(h16x8, qb[s % D2]), px, acc_out[3], 0, 0, 0);
        if (s + D2 < TB_OKS) qb[s % D2] = __builtin_nontemporal_load(wb + (s + D2) * 64);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  // ---- 4 groups of (q|k|v fragment 8 g + wave -> chunk, barrier, attention -> o chunk, barrier); the units of group g - 1 ride along ----
  for (int g = 0; g < TB_GROUPS; ++g) {
    const int f = 8 * g + wave;
    const int fnext = g + 1 < TB_GROUPS ? f + 8 : f;           // past the end: re-read this fragment (never consumed)
    const u32x4t* wcur = w1base + (int64_t)f * KS * 64;
    const u32x4t* wnxt = w1base + (int64_t)fnext * KS * 64;
    if (!late && g > 0) oproj(g - 1);
    f32x16 acc[RF];
#pragma unroll
    for (int b = 0; b < RF; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
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
    // the shared epilogue's LayerNorm fold with ln_rowvec, bias, rounding; the values go to the chunk instead of to memory
    // (opaque copy: what the epilogue derives from the lane is loop-invariant, and hipcc hoists it over the K loop, where the registers
    //  are spoken for: ffblock.hip)
    int lanee = lane;
    asm volatile("" : "+v"(lanee));
    const int frowe = lanee & 31, hsele = (lanee >> 5) * 4;
    // (the per-column operands are requested here, with the first position rows, not ahead of the K loop as in ffblock.hip: the
    //  position rows cost this round trip anyway, and the K loop has no 32 registers to spare beside the output accumulators)
    float4 cs4[4], bi4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      cs4[q] = *reinterpret_cast<const float4*>(p.colsum + f * 32 + 8 * q + hsele);
      bi4[q] = *reinterpret_cast<const float4*>(p.bias + f * 32 + 8 * q + hsele);
    }
#pragma unroll
    for (int b = 0; b < RF; ++b) {
      const float rstd = pre_ln[2 * b], mr = pre_ln[2 * b + 1];
      const float* pw = p.posw + (4 * b + (frowe >> 3)) * TB_NQKV + f * 32 + hsele;
      unsigned char* cw = chunk + (32 * b + frowe) * CPITCH + (32 * wave + hsele) * 2;
      float4 pw4[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) pw4[q] = *reinterpret_cast<const float4*>(pw + 8 * q);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float c4[4] = {cs4[q].x, cs4[q].y, cs4[q].z, cs4[q].w}, b4[4] = {bi4[q].x, bi4[q].y, bi4[q].z, bi4[q].w};
        const float p4[4] = {pw4[q].x, pw4[q].y, pw4[q].z, pw4[q].w};
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = fmaf(acc[b][4 * q + i] + p4[i], rstd, -mr * c4[i]) + b4[i];
        *reinterpret_cast<uint2*>(cw + 16 * q) = make_uint2(pack2h(v[0], v[1]), pack2h(v[2], v[3]));     // columns 32 wave + 8 q + hsel .. + 3 of the group
      }
    }
    if (late && g > 0) oproj(g - 1);
    __syncthreads();
    // ---- attention of heads 2 g, 2 g + 1: item = (band row r, head hh) on the lanes 2 item, 2 item + 1 -----------------------------
    if (wave < 6) {
      // (opaque copy: everything below that is derived from the thread index is loop-invariant, and hipcc hoists it over the K loop,
      //  where the registers are spoken for; the scheduling barriers keep it from requesting every key's vectors at once: ffblock.hip)
      int tidv = tid;
      asm volatile("" : "+v"(tidv));
      const int item = tidv >> 1, half = tidv & 1;
      const int hh = item >= TB_BM ? 1 : 0, r = item - TB_BM * hh;
      const unsigned char* kcol = chunk + (r & 7) * CPITCH + hh * 80;        // the item's pixel column: frame j is 8 rows further
      uint4 qv[5];
#pragma unroll
      for (int d = 0; d < 5; ++d) qv[d] = *reinterpret_cast<const uint4*>(chunk + r * CPITCH + hh * 80 + d * 16);
      float own[TB_F / 2];
#pragma unroll
      for (int i = 0; i < TB_F / 2; ++i) {
        __builtin_amdgcn_sched_barrier(0);
        const unsigned char* krow = kcol + (2 * i + half) * 8 * CPITCH + 160;
        float d0 = 0.f, d1 = 0.f;                                             // two chains, as tattn_kernel
#pragma unroll
        for (int d = 0; d < 5; ++d) {
          const uint4 kv = *reinterpret_cast<const uint4*>(krow + d * 16);
          d0 = dot2h(qv[d].x, kv.x, d0); d1 = dot2h(qv[d].y, kv.y, d1);
          d0 = dot2h(qv[d].z, kv.z, d0); d1 = dot2h(qv[d].w, kv.w, d1);
        }
        own[i] = d0 + d1;
      }
      __builtin_amdgcn_sched_barrier(0);
      float sc[TB_F];
      float mx = -1e30f;
#pragma unroll
      for (int i = 0; i < TB_F / 2; ++i) {
        const float oth = __shfl_xor(own[i], 1, 64);
        sc[2 * i] = half ? oth : own[i];
        sc[2 * i + 1] = half ? own[i] : oth;
      }
#pragma unroll
      for (int j = 0; j < TB_F; ++j) mx = fmaxf(mx, sc[j] * p.scale);
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < TB_F; ++j) {
        // tattn_kernel's `dot * scale - mx` is compiled as ONE fused multiply-add (hipcc contracts it, all 12 scores being the thread's
        // own); written out here, where half of the scores arrive from the partner lane and would otherwise be rounded first
        const float e = __expf(fmaf(sc[j], p.scale, -mx));
        sc[j] = e;
        sum += e;
      }
      const float inv = 1.0f / sum;
      // P.V for channels 20 half .. + 19 of the head, 4 at a time (keys ascending per channel)
      // -> the B operand of k-step ch / 16: lane (r & 31) + 32 ((ch / 8) & 1) of row fragment r / 32 holds channels 8 (ch / 8) .. + 7
      const unsigned char* vcol = kcol + 320 + half * 40;
      unsigned char* ow = ochunk + ((r >> 5) * 64 + (r & 31)) * 16;
#pragma unroll
      for (int t = 0; t < 5; ++t) {
        __builtin_amdgcn_sched_barrier(0);
        float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < TB_F; ++j) {
          const uint2 w = *reinterpret_cast<const uint2*>(vcol + j * 8 * CPITCH + 8 * t);
          o[0] = fmaf(sc[j], lo2f(w.x), o[0]); o[1] = fmaf(sc[j], hi2f(w.x), o[1]);
          o[2] = fmaf(sc[j], lo2f(w.y), o[2]); o[3] = fmaf(sc[j], hi2f(w.y), o[3]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] *= inv;
        const int ch = 40 * hh + 20 * half + 4 * t;
        *reinterpret_cast<uint2*>(ow + ((ch >> 4) * RF * 64 + 32 * ((ch >> 3) & 1)) * 16 + ((ch >> 2) & 1) * 8) =
            make_uint2(pack2h(o[0], o[1]), pack2h(o[2], o[3]));
      }
    }
    __syncthreads();
  }
  oproj(TB_GROUPS - 1);

  // ---- h' = acc + bo + h, rounded, and its row statistics per 32-column block ------------------------------------------------------
  int lanev = lane;
  asm volatile("" : "+v"(lanev));          // (opaque, as above)
  const int frowv = lanev & 31, hselv = (lanev >> 5) * 4;
  int grow[RF];
  rows_of(frowv, grow);
  const bool live = col0 + (frowv & 7) < p.ncol;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (u == 3 && !extra) break;
    const int c = u < 3 ? c0 : c1, b = u < 3 ? u : b1;
    const unsigned char* rp = smt + (32 * b + frowv) * PITCH + (32 * c + 4 * hselv) * 2;
    const uint4 rlo = *reinterpret_cast<const uint4*>(rp), rhi = *reinterpret_cast<const uint4*>(rp + 16);
    uint4 lo, hi;
    unit_finish(acc_out[u], p.bo + 32 * c, hselv, rlo, rhi, lo, hi);
    const int m = u < 3 ? grow[u] : (b1 == 0 ? grow[0] : b1 == 1 ? grow[1] : grow[2]);
    if (live) {
      h16_t* op = p.out + (int64_t)m * p.ldo + 32 * c + 4 * hselv;
      *reinterpret_cast<uint4*>(op) = lo;
      *reinterpret_cast<uint4*>(op + 8) = hi;
    }
    if (p.rowstats) {
      // as AVSD_GEMM_ROWSTATS (gemm_common.h): the 16 rounded values this lane stored plus the partner lane's 16, low half first
      float sm, sq;
      const unsigned w8[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
      rowstats16(w8, nullptr, sm, sq);
      const auto t = __builtin_amdgcn_permlane32_swap(__float_as_uint(sm), __float_as_uint(sm), false, false);
      const auto q = __builtin_amdgcn_permlane32_swap(__float_as_uint(sq), __float_as_uint(sq), false, false);
      if (live && hselv == 0)
        reinterpret_cast<float2*>(p.rowstats)[(int64_t)m * (TB_C / 32) + c] =
            make_float2(__uint_as_float(t[0]) + __uint_as_float(t[1]), __uint_as_float(q[0]) + __uint_as_float(q[1]));
    }
  }
}

// the lower bound on M (the break-even itself was not measured): at M = 24576 (256 bands, one per CU) the fused launch measured
// 54 us against 84 us for the three launches in the traced step (profiles/tblock_kernel_trace.md), the only size the step runs it
// at; with fewer bands CUs idle where the tiled GEMMs still fill the chip (event-timed from Python at M = 12288: 40 against 49 us,
// a loop the host paces, so not taken as a measurement)
constexpr int TB_MIN_M = 24576;

}  // namespace

extern "C" int avsd_temporal_block_supported(int M, int C, int heads, int frames) {
  return C == TB_C && heads == TB_HEADS && frames == TB_F && M >= TB_MIN_M ? 1 : 0;
}

extern "C" int avsd_temporal_block(const void* h, int ldh, const float* ln_stats, int ln_nblk, float ln_eps, const void* wqkv_frag,
                                   const float* qkv_colsum, const float* qkv_bias, const float* posw, const void* wo_frag, const float* bo,
                                   void* out, int ldo, float* rowstats, int B, int frames, int hw, int C, int heads, float scale,
                                   void* stream) {
  AVSD_REQUIRE(C == TB_C && heads == TB_HEADS && frames == TB_F,
               "temporal_block: unsupported shape: built for C = 320, 8 heads, 12 frames only, got C = %d, %d heads, %d frames", C, heads, frames);
  AVSD_REQUIRE(B > 0 && hw > 0 && (int64_t)B * hw * TB_F <= 0x7fffffff, "temporal_block: unsupported shape: B = %d, hw = %d", B, hw);
  AVSD_REQUIRE(h && ln_stats && wqkv_frag && qkv_colsum && qkv_bias && posw && wo_frag && bo && out, "temporal_block: null operand");
  AVSD_REQUIRE(ln_nblk == TB_C / 32 || ln_nblk == 1, "temporal_block: ln_nblk must be C / 32 or 1 (pre-folded), got %d", ln_nblk);
  AVSD_REQUIRE(ldh >= C && ldo >= C && ldh % 8 == 0 && ldo % 8 == 0,
               "temporal_block: unsupported strides: ldh %d and ldo %d must be multiples of 8, at least C", ldh, ldo);
  AVSD_REQUIRE(((uintptr_t)h | (uintptr_t)out | (uintptr_t)wqkv_frag | (uintptr_t)wo_frag | (uintptr_t)qkv_colsum | (uintptr_t)qkv_bias |
                (uintptr_t)posw | (uintptr_t)bo | (uintptr_t)ln_stats | (uintptr_t)rowstats) % 16 == 0, "temporal_block: operands must be 16-byte aligned");
  AVSD_REQUIRE(scale > 0.f, "temporal_block: scale must be positive");
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&tblock_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TB_LDS);
    if (e != hipSuccess) {
      avsd_set_error("temporal_block: hipFuncSetAttribute(%zu B LDS): %s", TB_LDS, hipGetErrorString(e));
      return AVSD_ELAUNCH;
    }
    attr_set = true;
  }
  tb_args a;
  a.h = reinterpret_cast<const h16_t*>(h); a.ldh = ldh;
  a.ln_stats = ln_stats; a.ln_nblk = ln_nblk; a.ln_eps = ln_eps;
  a.wqkv = reinterpret_cast<const u32x4t*>(wqkv_frag); a.colsum = qkv_colsum; a.bias = qkv_bias; a.posw = posw;
  a.wo = reinterpret_cast<const u32x4t*>(wo_frag); a.bo = bo;
  a.out = reinterpret_cast<h16_t*>(out); a.ldo = ldo;
  a.rowstats = rowstats;
  a.ncol = B * hw; a.hw = hw;
  a.scale = scale;
  hipLaunchKernelGGL(tblock_kernel, dim3((unsigned)((a.ncol + TB_PIX - 1) / TB_PIX)), dim3(512), TB_LDS, reinterpret_cast<hipStream_t>(stream), a);
  AVSD_CHECK_LAUNCH("temporal_block launch");
  return AVSD_OK;
}
