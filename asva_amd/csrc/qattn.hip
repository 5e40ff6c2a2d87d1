// Q projection + cross-attention in one launch for the transformer blocks below 32 x 32 (C = 640 / 1280, 8 heads):
//
//     O = softmax( (LN(h) Wq^T) K^T / sqrt(d) ) V
//
// Stages 1 and 2 of xattn_kernel (xattn.hip), split by head instead of holding every head of a row in one workgroup: the
// output projection, which needs all of them, stays the GEMM it was (DESIGN.md 10.5 — 24 workgroups at C = 1280 and
// 246 KB of K + V^T at C = 640 are objections to stage 3 only).  It replaces two launches (LayerNorm-folded Q projection,
// attention) and the M x C round trip of q between them; q never leaves the accumulators.
//
// One workgroup = BM rows of h x 160 channels (one head of 160, or two heads of 80): BM / 32 matrix waves of 32 rows each + 4 loader waves
//   stage 1  Q_g = LN-fold(h) . Wq'[160 g : 160 (g + 1), :]^T     LDS-direct K tiles over C in the tile image of xattn_kernel.  A 1-KiB
//            LDS-direct piece costs its wave ~90 cycles of issue, in order with its MFMAs: with the (BM + 160) / 8 pieces of a K tile
//            issued by the matrix waves themselves the loop ran at 1900 cycles per K tile for 640 cycles of MFMA.  The loader waves
//            issue them instead (7 or 9 each per K tile) into a ring of 5 (BM = 64) / 4 (BM = 128) stages, wait on their own counted
//            vmcnt, and the one s_barrier per K tile hands the landed tile to the matrix waves.
//   stage 2  per head: S^T = K_h . Q_h^T -> f32 softmax in registers (all keys resident: Lk <= 96) -> O^T = V_h^T . P^T
//            heads start on 16-channel k-blocks; the one 32-channel output fragment that two heads of 80 share takes
//            the row mask of xattn_kernel.  (matrix waves only; the loader waves have left)
//   store    O / l, rounded, 16 bytes per lane.
// LDS: stage 1 ring <= 144 KB | stage 2 K_g [LKP][168] + V_g^T [160][LKP + 4] <= 64 KB — the phases alias; + 1.25 KB colsum | bias.
// The grid is (row tiles x channel groups) in XCD-contiguous order with the group as the minor index: the workgroups of a
// row tile, and the row tiles of a K/V block, share one L2.  No atomics, fixed summation order.
#include "avsd_common.h"
#include "gemm_common.h"

namespace {

struct QAttnArgs {
  const h16_t* H; int ldh;
  const h16_t* Wq; int ldwq;
  const float* q_colsum; const float* q_bias;
  const float* ln_stats; int ln_nblk; float ln_eps;
  const h16_t* Kc; const h16_t* Vt;       // K [nkv][LKP][C], V^T [nkv][C][LKP]
  int lk, L, q_per_kv;
  float sl2;                              // softmax scale * log2(e)
  h16_t* O; int ldo;
  int nwg;
};

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int QA_NCH = 160;                // channels of a workgroup

// stages of the stage-1 ring: three to four K tiles in flight; one workgroup per CU (the grids are 192 workgroups on 256 CUs)
constexpr int qattn_stages(int BM) { return BM == 64 ? 5 : 4; }
constexpr int QA_NLW = 4;                  // loader waves
constexpr int QA_CB_BYTES = 2 * QA_NCH * 4;   // colsum | bias of the group's channels, f32
constexpr int qattn_threads(int BM) { return (BM / 32 + QA_NLW) * 64; }
constexpr int qattn_ln_bytes(int BM) { return BM * 8; }       // (rstd, mean * rstd) per row

template <int NT>
constexpr int qattn_lds_bytes(int BM) {
  const int ring = qattn_stages(BM) * (BM + QA_NCH) * 128;
  const int kv = NT * 32 * (QA_NCH + 8) * 2 + QA_NCH * (NT * 32 + 4) * 2;
  return (ring > kv ? ring : kv) + QA_CB_BYTES + qattn_ln_bytes(BM);
}

template <int C, int D, int BM, int NT>
__global__ __launch_bounds__(qattn_threads(BM)) void qattn_kernel(const QAttnArgs p) {
  constexpr int NCW = BM / 32, NLW = QA_NLW, NTHR = (NCW + NLW) * 64;      // matrix waves, loader waves
  constexpr int NCOL = QA_NCH;             // channels per matrix wave = per workgroup
  constexpr int NG = C / NCOL;             // channel groups
  constexpr int FN = NCOL / 32;            // 32-channel fragments per wave
  constexpr int HPW = NCOL / D;            // heads per workgroup
  constexpr int LKP = NT * 32;
  constexpr int NKT = C / BK;
  constexpr int A_BYTES = BM * 128, W_BYTES = NCOL * 128, STAGE_BYTES = A_BYTES + W_BYTES;
  constexpr int PAL = (BM / 8) / NLW, PPL = (STAGE_BYTES / 1024) / NLW;     // 1-KiB pieces of the A image / of a whole stage per loader wave
  constexpr int NS = qattn_stages(BM);     // ring stages
  constexpr int RING_BYTES = NS * STAGE_BYTES;
  constexpr int KS = NCOL + 8;             // sK row stride (elements): 16-byte aligned rows, ds_read_b128 spread over the banks
  constexpr int VS = LKP + 4;              // sVt row stride (elements): conflict-free ds_read_b64
  constexpr int SK_BYTES = LKP * KS * 2;
  static_assert(C % NCOL == 0 && NCOL % D == 0 && D % 16 == 0 && C % BK == 0 && BM % 32 == 0, "shape");
  static_assert(PAL * NLW * 8 == BM && PPL * NLW * 1024 == STAGE_BYTES && PPL <= 9, "a stage must split evenly into 1-KiB pieces per loader wave");
  static_assert(SK_BYTES + NCOL * VS * 2 <= RING_BYTES && RING_BYTES + QA_CB_BYTES + qattn_ln_bytes(BM) == qattn_lds_bytes<NT>(BM), "LDS");
  static_assert(qattn_lds_bytes<NT>(BM) <= 160 * 1024 && NKT >= NS && (NS - 2) * PPL < 64, "ring");
  extern __shared__ __attribute__((aligned(1024))) unsigned char smq[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool loader = wave >= NCW;         // wave-uniform
  const int lw = wave - NCW;               // loader index
  const int half = lane >> 5, l31 = lane & 31, hsel = half * 4;
  // XCD-aware order: the 8 XCDs each get a contiguous range of work items (row tile major, channel group minor)
  int tm, grp;
  {
    const int nwg = p.nwg, bid = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    const int w = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    tm = w / NG;
    grp = w - tm * NG;
  }
  const int row0 = tm * BM;
  const int ch0 = grp * NCOL;              // first channel of the group
  const int kvb = (row0 / p.L) / p.q_per_kv;

  const __amdgpu_buffer_rsrc_t rsH = __builtin_amdgcn_make_buffer_rsrc((void*)p.H, 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsWq = __builtin_amdgcn_make_buffer_rsrc((void*)p.Wq, 0, 0x7fffffff, 0x00020000);

  // loader wave lw issues pieces lw + 4 j of a stage (A image, then W image): j < PAL are rows of h, the others rows of Wq'.
  // This lane's element offset in each (literal bound: see xattn.hip)
  int poff[9];
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    int r, kc;
    if (j < PAL) {
      piece_row_chunk(lw + j * NLW, lane, r, kc);
      poff[j] = (row0 + r) * p.ldh + kc;
    } else {
      piece_row_chunk(lw + (j - PAL) * NLW, lane, r, kc);
      poff[j] = (ch0 + r) * p.ldwq + kc;
    }
  }
  // fragment read offsets inside a tile image (16-byte chunk c = 2 * ks + half is XOR-ed in per k-step)
  const int a_row = (loader ? 0 : wave) * 32 + l31;
  int w_row[FN];
#pragma unroll
  for (int a = 0; a < FN; ++a) w_row[a] = a * 32 + l31;

  f32x16 acc[FN];
#pragma unroll
  for (int a = 0; a < FN; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

  // ================= stage 1: Q_g = h . Wq'_g^T ===================================================================
#define QATTN_ISSUE1(kt_)                                                                                                                  \
  do {                                                                                                                                    \
    unsigned char* sb_ = smq + ((kt_) % NS) * STAGE_BYTES + lw * 1024;                                                                    \
    _Pragma("unroll") for (int j_ = 0; j_ < PPL; ++j_)                                                                                    \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(j_ < PAL ? rsH : rsWq, (lds_ptr_t)(sb_ + j_ * NLW * 1024), 16, (poff[j_] + (kt_) * BK) * 2, 0, 0, 0); \
  } while (0)
  // K_g and V_g^T of this tile's conditioning block (L2-resident, shared by every row tile of the block) go out first, a few vectors per
  // thread of all waves, and ride through stage 1 in registers: nothing of stage 2 waits on memory after the last K tile
  constexpr int KV8 = NCOL / 8, VV8 = LKP / 8;              // 16-byte vectors per K_g row / per V^T row
  constexpr int NKV = (LKP * KV8 + NTHR - 1) / NTHR, NVV = (NCOL * VV8 + NTHR - 1) / NTHR;
  u32x4 kreg[NKV], vreg[NVV];      // (a native vector: a uint4 array copied whole to LDS stays in scratch memory)
  {
    const h16_t* gk = p.Kc + (int64_t)kvb * LKP * C + ch0;
#pragma unroll
    for (int u = 0; u < NKV; ++u) {
      const int v = min(tid + u * NTHR, LKP * KV8 - 1);
      const int r = v / KV8, c8 = v - r * KV8;
      kreg[u] = *reinterpret_cast<const u32x4*>(gk + r * C + c8 * 8);
    }
    const u32x4* gv = reinterpret_cast<const u32x4*>(p.Vt + ((int64_t)kvb * C + ch0) * LKP);     // rows ch0 .. ch0 + 160 of V^T are contiguous
#pragma unroll
    for (int u = 0; u < NVV; ++u) vreg[u] = gv[min(tid + u * NTHR, NCOL * VV8 - 1)];
  }
  float* sCB = reinterpret_cast<float*>(smq + RING_BYTES);      // colsum[160] | bias[160] of the group
  float2* sLN = reinterpret_cast<float2*>(smq + RING_BYTES + QA_CB_BYTES);      // (rstd, mean * rstd) of the BM rows
  if (loader) {
    const int lt = tid - NCW * 64;
    // the loader waves also fold the LayerNorm statistics — LPR lanes per row, NB / LPR (sum, sumsq) pairs each, needed after the last K tile
    // only — so the matrix waves carry no statistics loads to the first barrier (fixed order: NBL partials per lane, then a two-level tree)
    constexpr int NB = C / 32, LPR = NLW * 64 / BM, NBL = NB / LPR;
    static_assert(LPR * BM == NLW * 64 && NBL * LPR == NB && (LPR == 2 || LPR == 4), "statistics split");
    const float2* st = reinterpret_cast<const float2*>(p.ln_stats) + (int64_t)(row0 + lt / LPR) * p.ln_nblk + (lt % LPR) * NBL;
    float2 st2[NBL];
#pragma unroll
    for (int j = 0; j < NBL; ++j) st2[j] = st[j];
    const int lc = min(lt, 2 * NCOL / 4 - 1);                    // 80 threads fetch one float4 of colsum | bias each (the others repeat the last)
    const float4 cb = *reinterpret_cast<const float4*>((lc < NCOL / 4 ? p.q_colsum : p.q_bias) + ch0 + 4 * (lc % (NCOL / 4)));
#pragma unroll
    for (int t = 0; t < NS - 1; ++t) QATTN_ISSUE1(t);
    *reinterpret_cast<float4*>(sCB + 4 * lc) = cb;
    float sm = 0.f, sq = 0.f;
#pragma unroll
    for (int j = 0; j < NBL; ++j) { sm += st2[j].x; sq += st2[j].y; }
#pragma unroll
    for (int o = 1; o < LPR; o *= 2) { sm += __shfl_xor(sm, o, 64); sq += __shfl_xor(sq, o, 64); }
    const float inv_k = 1.0f / (float)C;
    const float mean = sm * inv_k;
    const float rstd = rsqrtf(fmaxf(sq * inv_k - mean * mean, 0.f) + p.ln_eps);
    if (lt % LPR == 0) sLN[lt / LPR] = make_float2(rstd, mean * rstd);
  }
  for (int kt = 0; kt < NKT; ++kt) {
    // loader waves: tile kt has landed when at most the tiles issued after it are in flight (NS - 2 of them, fewer at the tail; loads
    // return in order, and any other load of the wave in between only makes the wait stricter).  The barrier hands tile kt to the matrix
    // waves and says that they are done with tile kt - 1, whose slot tile kt + NS - 1 takes.
    if (loader) {
      wait_tiles_ahead<NS - 2, PPL>(min(NKT - 1, kt + NS - 2) - kt);
      __builtin_amdgcn_s_waitcnt(0xc07f);     // lgkmcnt(0): (first pass) the colsum | bias and statistics writes have landed before the barrier
    }
    __builtin_amdgcn_s_barrier();
    if (loader) {
      if (kt + NS - 1 < NKT) QATTN_ISSUE1(kt + NS - 1);
    } else {
      const unsigned char* sA = smq + (kt % NS) * STAGE_BYTES;
      const unsigned char* sW = sA + A_BYTES;
#pragma unroll
      for (int ks = 0; ks < BK / 16; ++ks) {
        const int c = ks * 2 + half;
        const h16x8 xf = *reinterpret_cast<const h16x8*>(sA + frag_offset(a_row, c));
        h16x8 wf[FN];
#pragma unroll
        for (int a = 0; a < FN; ++a) wf[a] = *reinterpret_cast<const h16x8*>(sW + frag_offset(w_row[a], c));
#pragma unroll
        for (int a = 0; a < FN; ++a) acc[a] = mfma32x32x16(wf[a], xf, acc[a], 0, 0, 0);
      }
    }
  }
  // ---- q = rstd * acc - mean * rstd * colsum + bias, rounded, as MFMA B operands: k-block kb = 16 channels of the group ----
  h16x8 qf[2 * FN];
  const float2 lnv = sLN[a_row];
  const float ln_rstd = lnv.x, ln_mr = lnv.y;
#pragma unroll
  for (int a = 0; a < (loader ? 0 : FN); ++a) {
    float v[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = a * 32 + 8 * q + hsel;
      const float4 cs = *reinterpret_cast<const float4*>(sCB + n);
      const float4 bb = *reinterpret_cast<const float4*>(sCB + NCOL + n);
      v[q][0] = fmaf(acc[a][4 * q + 0], ln_rstd, -ln_mr * cs.x) + bb.x;
      v[q][1] = fmaf(acc[a][4 * q + 1], ln_rstd, -ln_mr * cs.y) + bb.y;
      v[q][2] = fmaf(acc[a][4 * q + 2], ln_rstd, -ln_mr * cs.z) + bb.z;
      v[q][3] = fmaf(acc[a][4 * q + 3], ln_rstd, -ln_mr * cs.w) + bb.w;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      unsigned e0[2], e1[2];
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const auto e = __builtin_amdgcn_permlane32_swap(pack2h(v[2 * j][2 * d], v[2 * j][2 * d + 1]),
                                                        pack2h(v[2 * j + 1][2 * d], v[2 * j + 1][2 * d + 1]), false, false);
        e0[d] = e[0]; e1[d] = e[1];
      }
      qf[2 * a + j] = __builtin_bit_cast(h16x8, make_uint4(e0[0], e0[1], e1[0], e1[1]));
    }
  }
  __syncthreads();   // every wave is done with the stage-1 ring: K_g / V_g^T take its place
  unsigned char* sK = smq;
  unsigned char* sVt = smq + SK_BYTES;
#pragma unroll
  for (int u = 0; u < NKV; ++u) {
    const int v = tid + u * NTHR;
    if (v < LKP * KV8) {
      const int r = v / KV8, c8 = v - r * KV8;
      *reinterpret_cast<u32x4*>(sK + r * (KS * 2) + c8 * 16) = kreg[u];
    }
  }
#pragma unroll
  for (int u = 0; u < NVV; ++u) {
    const int v = tid + u * NTHR;
    if (v < NCOL * VV8) {
      const int r = v / VV8, k8 = v - r * VV8;
      uint2* dst = reinterpret_cast<uint2*>(sVt + r * (VS * 2) + k8 * 16);
      dst[0] = make_uint2(vreg[u].x, vreg[u].y);
      dst[1] = make_uint2(vreg[u].z, vreg[u].w);
    }
  }
  __syncthreads();   // K_g / V_g^T staged
  if (loader) return;   // (no barrier below)

  // ================= stage 2: attention, head by head ==============================================================
  f32x16 acc_o[FN];
#pragma unroll
  for (int f = 0; f < FN; ++f)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc_o[f][r] = 0.f;
  float inv_l[HPW];
  const h16x8 zero8 = __builtin_bit_cast(h16x8, make_uint4(0, 0, 0, 0));
#pragma unroll
  for (int hh = 0; hh < HPW; ++hh) {
    constexpr int KBH = D / 16;                     // 16-channel k-blocks per head: a head starts on one
    // ---- S^T[key][query] = K . Q^T over the head's channels ----
    f32x16 s[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
#pragma unroll
    for (int kb = hh * KBH; kb < (hh + 1) * KBH; ++kb) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const h16x8 kf = *reinterpret_cast<const h16x8*>(sK + (32 * t + l31) * (KS * 2) + (16 * kb + 8 * half) * 2);
        s[t] = mfma32x32x16(kf, qf[kb], s[t], 0, 0, 0);
      }
    }
    // ---- softmax over all keys: lane owns query l31 and keys (r&3) + 8*(r>>2) + 4*half of each tile ----
    float mx = -1e30f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (key >= p.lk) s[t][r] = -1e30f;
        mx = fmaxf(mx, s[t][r]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float nm = -mx * p.sl2;
    float psum = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[t][r] = __builtin_amdgcn_exp2f(fmaf(s[t][r], p.sl2, nm));
        psum += s[t][r];
      }
    psum += __shfl_xor(psum, 32, 64);
    inv_l[hh] = 1.0f / psum;
    // ---- O^T[channel][query] += V^T . P^T ; k-slot e of MFMA (t, cc) <-> register 8*cc + e (key permutation matched on V) ----
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        uint4 pv;
        pv.x = pack2h(s[t][8 * cc + 0], s[t][8 * cc + 1]);
        pv.y = pack2h(s[t][8 * cc + 2], s[t][8 * cc + 3]);
        pv.z = pack2h(s[t][8 * cc + 4], s[t][8 * cc + 5]);
        pv.w = pack2h(s[t][8 * cc + 6], s[t][8 * cc + 7]);
        const h16x8 pf = __builtin_bit_cast(h16x8, pv);
#pragma unroll
        for (int f = 0; f < FN; ++f) {
          if (32 * f >= D * (hh + 1) || 32 * f + 32 <= D * hh) continue;      // fragment holds no channel of this head
          const int ch = 32 * f + l31;                                        // group-local output channel of this lane's V^T row
          const unsigned char* vr = sVt + ch * (VS * 2) + (32 * t + 16 * cc + 4 * half) * 2;
          const uint2 lo = *reinterpret_cast<const uint2*>(vr);
          const uint2 hi = *reinterpret_cast<const uint2*>(vr + 16);
          h16x8 vv = __builtin_bit_cast(h16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
          const bool whole = 32 * f >= D * hh && 32 * f + 32 <= D * (hh + 1);  // compile-time: every row belongs to the head
          if (!whole && (ch < D * hh || ch >= D * (hh + 1))) vv = zero8;
          acc_o[f] = mfma32x32x16(vv, pf, acc_o[f], 0, 0, 0);
        }
      }
  }

  // ================= store: O / l, rounded; lanes l / l ^ 32 trade quads -> 8 consecutive channels per lane =========
  h16_t* orow = p.O + (int64_t)(row0 + a_row) * p.ldo + ch0;
#pragma unroll
  for (int f = 0; f < FN; ++f) {
    float v[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c0 = 32 * f + 8 * q + i;          // channel of register 4q+i on the low half; +4 on the high half
        v[q][i] = acc_o[f][4 * q + i] * (half ? inv_l[(c0 + 4) / D] : inv_l[c0 / D]);
      }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      unsigned e0[2], e1[2];
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const auto e = __builtin_amdgcn_permlane32_swap(pack2h(v[2 * j][2 * d], v[2 * j][2 * d + 1]),
                                                        pack2h(v[2 * j + 1][2 * d], v[2 * j + 1][2 * d + 1]), false, false);
        e0[d] = e[0]; e1[d] = e[1];
      }
      *reinterpret_cast<uint4*>(orow + 32 * f + 16 * j + 8 * half) = make_uint4(e0[0], e0[1], e1[0], e1[1]);
    }
  }
#undef QATTN_ISSUE1
}

template <int C, int D, int BM, int NT>
int launch_qattn(QAttnArgs& a, int M, hipStream_t s) {
  constexpr int lds = qattn_lds_bytes<NT>(BM);
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&qattn_kernel<C, D, BM, NT>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) {
      avsd_set_error("qproj_attention: hipFuncSetAttribute(%d B LDS): %s", lds, hipGetErrorString(e));
      return AVSD_ELAUNCH;
    }
    attr_set = true;
  }
  a.nwg = (M / BM) * (C / QA_NCH);
  hipLaunchKernelGGL((qattn_kernel<C, D, BM, NT>), dim3((unsigned)a.nwg), dim3(qattn_threads(BM)), (size_t)lds, s, a);
  AVSD_CHECK_LAUNCH("qproj_attention launch");
  return AVSD_OK;
}

template <int C, int D, int BM>
int launch_qattn_nt(QAttnArgs& a, int M, int lk_pad, hipStream_t s) {
  switch (lk_pad) {
    case 32: return launch_qattn<C, D, BM, 1>(a, M, s);
    case 64: return launch_qattn<C, D, BM, 2>(a, M, s);
    default: return launch_qattn<C, D, BM, 3>(a, M, s);
  }
}

// rows of a workgroup for a shape, 0 = not built.  A row tile never spans two K/V blocks: rows_per_kv_block % BM == 0.
int qattn_bm(int C, int heads, int lk_pad, int rows_per_kv_block) {
  if (heads != 8 || (lk_pad != 32 && lk_pad != 64 && lk_pad != 96) || rows_per_kv_block <= 0) return 0;
  if (C == 640) return rows_per_kv_block % 128 == 0 ? 128 : rows_per_kv_block % 64 == 0 ? 64 : 0;
  if (C == 1280) return rows_per_kv_block % 64 == 0 ? 64 : 0;
  return 0;
}

}  // namespace

extern "C" int avsd_qproj_attention_supported(int C, int heads, int lk_pad, int rows_per_kv_block) {
  return qattn_bm(C, heads, lk_pad, rows_per_kv_block) ? 1 : 0;
}

extern "C" int avsd_qproj_attention(const avsd_xattn_desc* dp, void* stream) {
  AVSD_REQUIRE(dp != nullptr, "qproj_attention: null descriptor");
  const avsd_xattn_desc& d = *dp;
  AVSD_REQUIRE(d.h && d.ln_stats && d.wq && d.q_colsum && d.q_bias && d.k && d.vt && d.out, "qproj_attention: null pointer");
  AVSD_REQUIRE(!d.wo && !d.o_bias && !d.res && !d.rowstats && !d.out_master && !d.stats_pos,
               "qproj_attention: wo, o_bias, res, rowstats, out_master and stats_pos must be null (the output projection is a launch of its own)");
  AVSD_REQUIRE(d.L > 0 && d.q_per_kv > 0 && d.M > 0 && d.M % d.L == 0 && (d.M / d.L) % d.q_per_kv == 0,
               "qproj_attention: M (%d) must be whole K/V blocks of L (%d) x q_per_kv (%d) rows", d.M, d.L, d.q_per_kv);
  const int64_t rows_per_kv = (int64_t)d.L * d.q_per_kv;
  const int bm = rows_per_kv <= d.M ? qattn_bm(d.C, d.heads, d.lk_pad, (int)rows_per_kv) : 0;
  AVSD_REQUIRE(bm != 0,
               "qproj_attention: unsupported shape C=%d heads=%d lk_pad=%d rows per K/V block=%lld (built: C=640 / 1280, 8 heads, lk_pad 32/64/96, "
               "K/V blocks of whole 64-row tiles)", d.C, d.heads, d.lk_pad, (long long)rows_per_kv);
  AVSD_REQUIRE(d.lk > 0 && d.lk <= d.lk_pad, "qproj_attention: bad key count");
  AVSD_REQUIRE(d.ldh % 8 == 0 && d.ldwq % 8 == 0 && d.ldo % 8 == 0 && d.ldh >= d.C && d.ldwq >= d.C && d.ldo >= d.C,
               "qproj_attention: row strides must be multiples of 8 and >= C");
  AVSD_REQUIRE((double)d.M * d.ldh * 2.0 < 2147483648.0 && (double)d.C * d.ldwq * 2.0 < 2147483648.0, "qproj_attention: h and wq must be < 2 GiB");
  AVSD_REQUIRE(d.scale > 0.f, "qproj_attention: scale must be positive");
  QAttnArgs a;
  a.H = (const h16_t*)d.h; a.ldh = d.ldh;
  a.Wq = (const h16_t*)d.wq; a.ldwq = d.ldwq;
  a.q_colsum = d.q_colsum; a.q_bias = d.q_bias;
  a.ln_stats = d.ln_stats; a.ln_nblk = d.C / 32; a.ln_eps = d.ln_eps;
  a.Kc = (const h16_t*)d.k; a.Vt = (const h16_t*)d.vt;
  a.lk = d.lk; a.L = d.L; a.q_per_kv = d.q_per_kv;
  a.sl2 = d.scale * 1.4426950408889634f;
  a.O = (h16_t*)d.out; a.ldo = d.ldo;
  a.nwg = 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (d.C == 640) return bm == 128 ? launch_qattn_nt<640, 80, 128>(a, d.M, d.lk_pad, s) : launch_qattn_nt<640, 80, 64>(a, d.M, d.lk_pad, s);
  return launch_qattn_nt<1280, 160, 64>(a, d.M, d.lk_pad, s);
}
