/*
 * avsd.h — C ABI of libavsd_hip.so: the MI355X (gfx950) kernels behind the AVSyncD
 * denoising path (per-step AudioUNet3D forward, CFG + scheduler update, VAE decode), the audio
 * front end, the AVSync scorer, the CLIP text encoder and the ImageBind evaluation towers (f32 in both builds).
 *
 * The reference (lzhangbj/ASVA) has no FFI layer: its hot path is PyTorch module calls.
 * Each entry point below names the reference call site (file:line under /root/reference)
 * whose arithmetic it replaces.  The host side (the asva_amd Python package) binds these with ctypes;
 * INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every function returns 0 on success, a negative AVSD_E* code otherwise;
 *     avsd_last_error() returns a thread-local message for the last failure.
 *   - all pointers are DEVICE pointers owned by the caller (torch tensors) unless the
 *     parameter name ends in _host.  Nothing here allocates or frees device memory, and
 *     nothing synchronises: every launch goes to `stream` (a hipStream_t), so the whole
 *     step is capturable in a hipGraph.
 *   - "bf16" buffers are raw uint16 bfloat16; statistics / biases / norm parameters are f32.
 *   - activations are channels-last: a (B, F, H, W, C) tensor is the row-major matrix
 *     [M = B*F*H*W, C]; "ld*" arguments are row strides in ELEMENTS.
 */
#ifndef AVSD_H
#define AVSD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVSD_OK 0
#define AVSD_EINVAL (-1)   /* bad argument (shape / alignment / null pointer)   */
#define AVSD_ELAUNCH (-2)  /* hipLaunch / runtime error                          */
#define AVSD_ENODEV (-3)   /* no gfx950 device / wrong architecture              */

#define AVSD_ABI_VERSION 10  /* v10: AVSD_GEMM_OUT_REST, AVSD_GEMM_X2 with out_master; v9: tile ids 67 (128 x 320 asm tile) and 70 (A-resident N-streaming tile), AVSD_GEMM_W_FRAG */

/* ---- library ------------------------------------------------------------------------ */
int avsd_abi_version(void);
/* "bf16" or "fp16": the 16-bit storage type this build of the library computes in. */
const char* avsd_precision(void);
const char* avsd_last_error(void);
/* Fills name[<=len] with the device arch string (e.g. "gfx950:sramecc+:xnack-"), and the
 * CU count.  AVSD_ENODEV when no device is visible. */
int avsd_device_info(char* name_host, int len, int* num_cu_host);

/* ---- GEMM family ---------------------------------------------------------------------
 * out[M, N] = epilogue( alpha * A'[M, K] . W[N, K]^T )
 * W is always [N][ldw] (K contiguous) — torch nn.Linear / packed conv weight layout.
 * A' is produced by the A-loader selected by `mode`:
 *
 *   AVSD_GEMM_PLAIN  A'[m, k] = k < k_split ? A[m*lda + k] : A2[m*lda2 + (k - k_split)]
 *                    (k_split == K, A2 == NULL for a single source).  Replaces nn.Linear /
 *                    1x1 nn.Conv2d: utils.py:123-131,159 (q/k/v/out), proj_in/proj_out
 *                    ff_spatio_audio_temp_transformer_3d.py:66,92, GEGLU FeedForward :276,
 *                    conv_shortcut ff_spatio_temp_resnet_3d.py:159 on a torch.cat input
 *                    (unet_3d_blocks.py:358,1038).
 *   AVSD_GEMM_TMIX   the temporal mixing linear of FFInflatedConv3d (utils.py:43-53):
 *                    K = 3*cseg; for row m = (b, f, p) (p in [0,hw)) segment s of K reads
 *                    row (b, g_s(f), p) of A with g = {0, max(f-1,0), f}.
 *   AVSD_GEMM_CONV3  implicit-GEMM 3x3 pad-1 convolution over channels-last images
 *                    (utils.py:37-38 -> nn.Conv2d): K = 9*cin (tap-major, cin-minor),
 *                    row m = (n, ho, wo); stride 1 or 2; `ups`=1 reads the input through a
 *                    nearest x2 upsample (ff_spatio_temp_resnet_3d.py:48); `pad` = top/left padding.
 *                    `ups`=2 (v10) is the SUB-PIXEL form of the same upsample + convolution: output pixel (2y + dy, 2x + dx) of the
 *                    upsampled 3x3 convolution only sees input rows y + dy - 1, y + dy and columns x + dx - 1, x + dx, so it is a 2x2
 *                    convolution on the ORIGINAL image with the kernel rows / columns that land on the same input pixel summed
 *                    (asva_amd/weights.py subpixel_conv3x3): the same function with 4/9 of the multiplies.  Descriptor: rows
 *                    m = (img, y, x) over the INPUT image (ho = hs, wo = ws), K = 4*cin (tap (i, j)-major: input pixel
 *                    (y + dy - 1 + i, x + dx - 1 + j)), N = 4*cout with column n = (2 dy + dx) * cout + co and W [4*cout][4*cin] likewise
 *                    (bias [4*cout] = the layer's bias four times); the epilogue stores element (m, n) to channel co of OUTPUT pixel
 *                    (img, 2y + dy, 2x + dx) of out [n_img*2hs*2ws][ldc] (out_master / the rest plane likewise).  stride 1, pad 1,
 *                    cin % 64 == 0, cout % 64 == 0 and cout a multiple of the tile's column width; bias only (no residual, row vector,
 *                    activation, statistics); LDS-direct tiles (4..38), AVSD_GEMM_X2 included.
 *
 * epilogue, in f32:  v = act(alpha*acc + bias[n] + rowvec[(m / rows_per_vec)*ldv + n])
 *                                   + res1[m*ldr1 + n] + res2[m*ldr2 + n]
 *   AVSD_GEMM_GELU:  act = gelu_erf (the MLP of the audio front-end's ViT blocks); identity otherwise.
 *   AVSD_GEMM_GEGLU: W rows are packed per 32-row block as [16 value rows | 16 gate rows];
 *                    out[M, N/2] = value * gelu_erf(gate)   (diffusers GEGLU)
 *   AVSD_GEMM_OUT_F32: out is f32 instead of 16-bit.
 *   AVSD_GEMM_RES1_F32 / RES2_F32: res1 / res2 are f32 [M][ldr] instead of 16-bit.  With `out_master` != NULL the epilogue
 *                    also stores the UN-ROUNDED f32 result to out_master[m*ldm + n]: together they keep a residual
 *                    stream (h = h + f(h), ff_spatio_audio_temp_transformer_3d.py:300-371; x + h, ff_spatio_temp_resnet_3d.py:189)
 *                    in f32 while the 16-bit copy in `out` feeds the next matrix multiply.
 * "16-bit" = bfloat16 in libavsd_hip.so, IEEE half in libavsd_hip_f16.so (the same sources built with -DAVSD_F16=1;
 *   avsd_precision() tells which); accumulation and the epilogue are f32 in both.
 *   AVSD_GEMM_KROT:  scheduling hint for the asm tiles (gemm4.hip): row bands start their K walk at different tiles and wrap (the weights of
 *                    the low-resolution layers stream from HBM: a lockstep walk is one chain of round trips).  Deterministic; the f32
 *                    summation order of a band then starts mid-K, so results differ from the unrotated walk in the last bits.
 *   AVSD_GEMM_XCD_N: scheduling hint, no effect on the result — tiles are dealt to the 8 XCDs in bands of N instead of
 *                    bands of M, so the weights (not the activations) are the operand each L2 fetches only once.
 *   AVSD_GEMM_W_FRAG: W is stored in MFMA-fragment order instead of [N][ldw]: [N / 32][K / 16][64][8] 16-bit values with element
 *                    (f, s, l, e) = W[32 f + (l & 31)][16 s + 8 (l >> 5) + e] (asva_amd/weights.py pack_frag) — one k-step of one 32-column
 *                    fragment is 1 KB, contiguous.  Only tile AVSD_GEMM_TILE_NSTREAM reads it (and refuses anything else); ldw is ignored.
 *   AVSD_GEMM_OUT_REST: a ONE-pass product whose 16-bit output also gets its rest plane: besides main = round16(v) at `out`, the epilogue
 *                    stores rest = round16(v - main) at `out + out_lo` elements (same strides) — the (main, rest) pair a three-pass product
 *                    (AVSD_GEMM_X2) reads as its A operand, written by the producer of the tensor instead of by a separate avsd_split_f32 pass
 *                    over its f32 master (per-layer precision plan: the ResBlock / transformer outputs that feed the three-pass shortcut and
 *                    sampler convolutions, ff_spatio_temp_resnet_3d.py:30-62,88-96,159).  16-bit output only, not with GEGLU; LayerNorm row
 *                    statistics (ROWSTATS) stay those of the main plane, which is what the one-pass consumers read.
 * blockIdx.z batches: pointers advance by batch_stride_* elements (0 = shared).
 */
enum { AVSD_GEMM_PLAIN = 0, AVSD_GEMM_TMIX = 1, AVSD_GEMM_CONV3 = 2 };
enum { AVSD_GEMM_GEGLU = 1, AVSD_GEMM_OUT_F32 = 2, AVSD_GEMM_GELU = 4, AVSD_GEMM_XCD_N = 8, AVSD_GEMM_ROWSTATS = 16,
       AVSD_GEMM_LNFUSE = 32, AVSD_GEMM_RES1_F32 = 64, AVSD_GEMM_RES2_F32 = 128, AVSD_GEMM_X2 = 256, AVSD_GEMM_KROT = 512, AVSD_GEMM_W_FRAG = 1024,
       AVSD_GEMM_OUT_REST = 2048 };
#define AVSD_GEMM_MAX_TILE 33
#define AVSD_GEMM_MAX_TILE_X2 36   /* AVSD_GEMM_X2 also has tiles 34..36 (gemm.hip dispatch_tile_x2) */
/* 256 x 160 LDS-direct tile, 8 MFMA + 4 loader waves (gemm.hip dispatch_tile; not with AVSD_GEMM_X2) */
#define AVSD_GEMM_TILE_256x160_8W 38
/* 3x3 stride-1 pad-1 convolution tiles with the input tile resident in LDS (conv3r.hip): K is walked chunk-major (64 input
 * channels at a time), the BM output rows plus one image row of halo on either side are staged once per chunk and read by all
 * nine taps; only the weight tile streams per K tile.  CONV3 descriptors with stride 1, ups 0, pad 1, one source,
 * cin % 64 == 0, image width <= 32 and a tile of whole image rows / whole images (avsd_gemm_conv3r_supported); split_k cuts
 * the channel chunks (split_k <= cin / 64).  No AVSD_GEMM_X2 / GEGLU / LNFUSE.  Other descriptors are refused with these ids. */
/* 4-wave tiles with a hand-scheduled (inline-asm) main loop, register-staged operands (gemm4.hip): 60 = 256 x 256, 61 = 256 x 128,
 * 62 = 128 x 256, 63 = 128 x 128, 64 = 128 x 64, 65 = 64 x 128, 66 = 64 x 64, 67 = 128 x 320 (PLAIN / TMIX, no AVSD_GEMM_X2).  PLAIN single-source descriptors with K % 64 == 0, no AVSD_GEMM_X2; every epilogue flag; split_k. */
#define AVSD_GEMM_TILE_ASM_FIRST 60
#define AVSD_GEMM_TILE_ASM_LAST 67
/* A-resident, N-streaming tile (nstream.hip): the workgroup keeps its 96-row band of A (all of K) in LDS and its 8 independent waves
 * stream W fragments straight from memory into MFMA operands — for the wide short-K projections (the GEGLU projection of a transformer
 * block: K = 320 / 640, N = 8 K).  PLAIN single-source descriptors with AVSD_GEMM_W_FRAG, K = 320 or 640, N % 32 == 0 (built for N % 256 == 0: 8 waves x whole fragments); every epilogue
 * flag except the position tables; no split_k, no AVSD_GEMM_X2. */
#define AVSD_GEMM_TILE_NSTREAM 70
#define AVSD_GEMM_TILE_CONV3R_FIRST 40
#define AVSD_GEMM_TILE_CONV3R_LAST 49
/* the same convolution with RECTANGULAR resident tiles (TH image rows x 32 pixels + a one-pixel halo, positions outside the image
 * zero-filled at load time) for images wider than 32 pixels: width % 32 == 0, height % TH == 0 (avsd_gemm_conv3r2d_supported);
 * otherwise as the ids above. */
#define AVSD_GEMM_TILE_CONV3R2D_FIRST 51
#define AVSD_GEMM_TILE_CONV3R2D_LAST 54
typedef struct avsd_gemm_desc {
  const void* A;        /* bf16 */
  const void* A2;       /* bf16 or NULL */
  const void* W;        /* bf16 [N][ldw] */
  void* out;            /* bf16 or f32 [M][ldc] */
  const float* bias;    /* [N] or NULL */
  const float* rowvec;  /* [ceil(M/rows_per_vec)][ldv] or NULL */
  const void* res1;     /* bf16 [M][ldr1] or NULL */
  const void* res2;     /* bf16 [M][ldr2] or NULL */
  int32_t M, N, K;
  int32_t lda, lda2, k_split, ldw, ldc, ldr1, ldr2;
  int32_t rows_per_vec, ldv;
  float alpha;
  int32_t mode, flags;
  int32_t batch;                        /* >= 1 */
  int64_t batch_stride_a, batch_stride_w, batch_stride_out;
  /* TMIX */
  int32_t hw, frames, cseg;
  /* CONV3: source image (hs, ws) with cin channels at row stride lda; output (ho, wo) */
  int32_t hs, ws, ho, wo, cin, stride, ups;
  int32_t pad;                          /* CONV3 top/left zero padding: 1 (symmetric "padding=1") or 0 (the VAE encoder's
                                           F.pad(0,1,0,1) + stride-2 conv); bottom/right reads beyond the image are zero */
  int32_t tile;                         /* 0 = library heuristic; 1..3 register-staged tiles, 4..AVSD_GEMM_MAX_TILE LDS-direct
                                           tiles (see gemm.hip dispatch_tile) */
  /* split-K (LDS-direct tiles only): K is cut into split_k slices computed by separate workgroups that
   * store f32 partial tiles to splitk_ws[split_k][M][N]; a second launch reduces them and applies the epilogue.
   * Deterministic (no atomics).  split_k <= 1 disables it.  Not combinable with GEGLU or batch > 1. */
  int32_t split_k;
  float* splitk_ws;
  /* LayerNorm folded into the GEMMs around it (ff_spatio_audio_temp_transformer_3d.py:300-371: every LayerNorm there
   * feeds linear layers only).  Producer side, AVSD_GEMM_ROWSTATS: besides `out`, the epilogue writes for every row m and
   * every 32-column block j the pair (sum, sum of squares) of the bf16-ROUNDED outputs to rowstats[(m * N/32 + j) * 2]
   * (N % 32 == 0; deterministic, no atomics).  Consumer side, AVSD_GEMM_LNFUSE: A is the un-normalised tensor, W has
   * the LayerNorm gain folded in (W' = W * gamma along K), ln_colsum[n] = sum_k W'[n, k], `bias` carries
   * sum_k beta[k] W[n, k] (+ the layer's own bias), and the epilogue computes
   *     v = rstd[m] * (alpha * acc - mean[m] * ln_colsum[n]) + bias[n] + ...
   * with mean / rstd of row m folded from the ln_nblk (= K / 32, or 1: pre-folded by avsd_ln_fold) pairs of ln_stats — exactly LayerNorm(A) . W^T + b.
   * Batched launches read the statistics of row (batch * batch_stride_a / lda + m). */
  float* rowstats;
  const float* ln_stats;
  const float* ln_colsum;
  int32_t ln_nblk;
  float ln_eps;
  float* out_master;                    /* f32 [M][ldm] or NULL: un-rounded copy of the result (not with GEGLU) */
  int32_t ldm;
  int32_t raster_g;                     /* scheduling knob, no effect on the result: rows of the tile blocks an XCD walks (tile_of_item,
                                           gemm_common.h: 0 = the library default of 8; 1..64 = probe values, tools/asm_bench.py).  Must be
                                           0..64: avsd_gemm_bf16 refuses anything else (a large value would overflow the work-item -> tile
                                           map and drop or duplicate tiles).  Was `reserved0` up to ABI v8. */
  /* AVSD_GEMM_X2 (split precision, see "split-precision storage" below): every 16-bit operand is a pair of planes; these are
   * the ELEMENT offsets from each main plane to its rest plane (same strides).  The product is accumulated as
   * W.A + Wr.A + W.Ar (three MFMA passes into one f32 accumulator); 16-bit residuals are read as main + rest and the output
   * is written as main = round16(v), rest = round16(v - main) — and, with `out_master`, the un-rounded f32 value as well (v10).
   * LDS-direct tiles 7, 11, 13, 24, 25, 34, 35, 36 and the asm tiles.  `out_lo` is also the rest-plane offset of AVSD_GEMM_OUT_REST. */
  int64_t a_lo, a2_lo, w_lo, out_lo, res1_lo, res2_lo;
  /* LayerNorm(x + pos[frame]) folded like the plain LayerNorm above (ff_spatio_audio_temp_transformer_3d.py:346-356: norm_temp of
   * h + the temporal position embedding feeds the q|k|v projection of the temporal attention).  Row m belongs to frame
   * f(m) = (m / pos_hw) % pos_frames.  Producer side, `stats_pos` f32 [pos_frames][N] with AVSD_GEMM_ROWSTATS: the row statistics are
   * those of (rounded output + stats_pos[f(m)]) — `out` itself is unchanged.  Consumer side, `ln_rowvec` f32 [pos_frames][N] =
   * pos . W'^T with AVSD_GEMM_LNFUSE: v = rstd[m] * (alpha * acc + ln_rowvec[f(m)][n] - mean[m] * ln_colsum[n]) + bias[n], i.e.
   * LayerNorm(A + pos) . W^T + b with A un-normalised and pos never added to it.  Not with AVSD_GEMM_X2. */
  const float* stats_pos;
  const float* ln_rowvec;
  int32_t pos_hw, pos_frames;
} avsd_gemm_desc;

int avsd_gemm_bf16(const avsd_gemm_desc* desc_host, void* stream);
/* rows per tile of conv3r tile id `tile` if an (hs x ws)-pixel image with cin channels can use it, else 0 */
int avsd_gemm_conv3r_supported(int tile, int hs, int ws, int cin);
int avsd_gemm_conv3r2d_supported(int tile, int hs, int ws, int cin);
/* sizeof(avsd_gemm_desc) as compiled: lets an FFI binding verify its mirror of the struct. */
int avsd_sizeof_gemm_desc(void);

/* ---- fused cross-attention block --------------------------------------------------------------------------------
 * One launch per residual-stream update of the audio / text cross-attention of BasicTransformerBlock
 * (ff_spatio_audio_temp_transformer_3d.py:315-341; diffusers Attention + AttnProcessor2_0):
 *     out = res + to_out( softmax( (LayerNorm(h) Wq^T) K^T * scale ) V ) + o_bias
 * h [M][C] is the 16-bit residual stream with its LayerNorm statistics `ln_stats` [M][C/32][2] as written by
 * AVSD_GEMM_ROWSTATS; wq / q_colsum / q_bias are the LayerNorm-folded to_q of AVSD_GEMM_LNFUSE; `res` is h again (16-bit)
 * or its f32 master (res_f32).  K / V are the step-invariant projections of the conditioning, cached by the host in the
 * layout this kernel stages: k [nkv][lk_pad][C] (rows >= lk are padding) and vt [nkv][C][lk_pad] (V transposed), where
 * rows [q*L, (q+1)*L) of h use block q / q_per_kv — for the audio branch the host gathers the keys the segment mask
 * leaves visible per frame (segmask_imagebind.py:62-78,104-114), so masked keys are simply absent.
 * Outputs like avsd_gemm_bf16: `out` 16-bit [M][ldo], optional `out_master` f32 and `rowstats` of the rounded output.
 * Built for C = 320 with 8 heads (SD1.5 level 0) and lk_pad in {32, 64, 96}: avsd_cross_attention_block_supported()
 * tells; other shapes run the three separate kernels. */
typedef struct avsd_xattn_desc {
  const void* h;        int32_t ldh;
  int32_t res_f32;
  const void* res;      int32_t ldres;
  int32_t M, C, heads, L;
  const float* ln_stats; float ln_eps;
  float scale;
  const void* wq;       int32_t ldwq;  int32_t lk;
  const float* q_colsum;
  const float* q_bias;
  const void* k;        const void* vt;
  int32_t lk_pad, q_per_kv;
  const void* wo;       int32_t ldwo;  int32_t ldo;
  const float* o_bias;
  void* out;
  float* out_master;    int32_t ldm;   int32_t reserved0;
  float* rowstats;
  const float* stats_pos;   /* as avsd_gemm_desc.stats_pos: [pos_frames][C], the row statistics are those of out + stats_pos[frame of the row] */
  int32_t pos_hw, pos_frames;
} avsd_xattn_desc;
int avsd_cross_attention_block_supported(int C, int heads, int lk_pad);
int avsd_cross_attention_block(const avsd_xattn_desc* desc_host, void* stream);
int avsd_sizeof_xattn_desc(void);

/* Stages 1-2 of the block above for the wider levels, split by head: one launch for
 *     out[M][ldo] = softmax( (LayerNorm(h) Wq^T) K^T * scale ) V        (16-bit)
 * in place of the LayerNorm-folded Q projection and the attention launch; the output projection stays a GEMM.  Takes the same
 * descriptor: wo, o_bias, res, rowstats, out_master and stats_pos must be null.  Built for C = 640 / 1280 with 8 heads and
 * lk_pad in {32, 64, 96}, where a K/V block serves rows_per_kv_block = L * q_per_kv rows that are whole 64-row tiles:
 * avsd_qproj_attention_supported() tells; anything else is AVSD_EINVAL and runs as the separate kernels. */
int avsd_qproj_attention_supported(int C, int heads, int lk_pad, int rows_per_kv_block);
int avsd_qproj_attention(const avsd_xattn_desc* desc_host, void* stream);

/* The tail of a 320-channel transformer block as one launch (csrc/ffblock.hip), in place of three GEMMs:
 *     g   = GEGLU(LayerNorm(h) . W1'^T + b1)      [M][4 C]   (AVSD_GEMM_LNFUSE | AVSD_GEMM_GEGLU, W1' packed for GEGLU)
 *     h'  = g . W2^T + b2 + h                     [M][C]
 *     out = h' . Wp^T + bp + x                    [M][C]     (wp_frag == NULL: out = h', and bp, x are ignored)
 * h, x, out: 16-bit rows with leading dimensions ldh, ldx, ldo (multiples of 8); ln_stats: the f32 [M][ln_nblk][2] row statistics of
 * h (ln_nblk = C / 32, or 1: pre-folded), w1_colsum / b1 as ln_colsum / bias of the folded projection; w1_frag [8 C / 32][C / 16][64][8],
 * w2_frag [C / 32][4 C / 16][64][8] and wp_frag [C / 32][C / 16][64][8] are the three weights in MFMA-fragment order
 * (AVSD_GEMM_W_FRAG).  g and h' are rounded to 16 bits as the three launches round them and every product accumulates in f32
 * over ascending K: bit-identical to them on LDS-direct tiles with the unrotated K walk.  Built for C = 320 in the one-pass
 * libraries; anything else is AVSD_EINVAL and launches nothing.  avsd_ff_block_supported() tells where it is built AND measured
 * faster than the launches it replaces (a lower bound on M). */
int avsd_ff_block_supported(int M, int C, int with_proj_out);
int avsd_ff_block(const void* h, int ldh, const float* ln_stats, int ln_nblk, float ln_eps, const void* w1_frag, const float* w1_colsum,
                  const float* b1, const void* w2_frag, const float* b2, const void* wp_frag, const float* bp, const void* x, int ldx,
                  void* out, int ldo, int M, int C, void* stream);

/* The temporal attention of a 320-channel transformer block as one launch (csrc/tblock.hip), in place of a GEMM, avsd_temporal_attention
 * and a GEMM:
 *     qkv = LayerNorm(h + pos[frame]) . Wqkv'^T + b   [M][3 C]   (AVSD_GEMM_LNFUSE with ln_rowvec = posw)
 *     o   = softmax(q k^T . scale) v                  [M][C]     over the `frames` rows of a pixel, per head
 *     out = o . Wo^T + bo + h                         [M][C]     (+ rowstats as AVSD_GEMM_ROWSTATS writes them, unless NULL)
 * M = B frames hw, row (b frames + f) hw + pixel.  h, out: 16-bit rows with leading dimensions ldh, ldo (multiples of 8); ln_stats: the
 * f32 [M][ln_nblk][2] row statistics of h + pos (ln_nblk = C / 32, or 1: pre-folded).  The q|k|v columns come regrouped: 4 groups of 2
 * heads, each [q | k | v] of its heads = 240 columns padded with zeros to 256, so wqkv_frag is [32][C / 16][64][8] (AVSD_GEMM_W_FRAG
 * order of the regrouped [1024][C] matrix), qkv_colsum and qkv_bias [1024] and posw [frames][1024] in the same order; wo_frag
 * [C / 32][C / 16][64][8].  qkv and o are rounded to 16 bits as the three launches round them and every sum runs in their order:
 * bit-identical to them on LDS-direct tiles with the unrotated K walk.  Built for C = 320, 8 heads, 12 frames in the one-pass
 * libraries; anything else is AVSD_EINVAL and launches nothing.  avsd_temporal_block_supported() tells where it is built AND measured
 * faster than the launches it replaces (a lower bound on M). */
int avsd_temporal_block_supported(int M, int C, int heads, int frames);
int avsd_temporal_block(const void* h, int ldh, const float* ln_stats, int ln_nblk, float ln_eps, const void* wqkv_frag,
                        const float* qkv_colsum, const float* qkv_bias, const float* posw, const void* wo_frag, const float* bo,
                        void* out, int ldo, float* rowstats, int B, int frames, int hw, int C, int heads, float scale, void* stream);

/* out[M, N] (f32) = act_out( act_in(x[M, K] f32) . W[N, K]^T + bias ), M <= 16.
 * act: 0 none, 1 SiLU.  Time-embedding MLP and the per-ResBlock time_emb_proj
 * (audio_cond_unet_3d_condition.py:673-680, ff_spatio_temp_resnet_3d.py:170), and the
 * temporal position MLP (ff_spatio_audio_temp_transformer_3d.py:348-349). */
int avsd_linear_small_m(const float* x, const void* W_bf16, const float* bias, float* out,
                        int M, int N, int K, int ldw, int act_in, int act_out, void* stream);

/* ---- normalisation -------------------------------------------------------------------
 * GroupNorm over channels-last data: stats (partials + finalize) then apply.
 * stats: for each of `nb` normalisation batches (a batch = `rows_per_batch` consecutive
 *   rows: F*H*W for the 5-D GroupNorm of ff_spatio_temp_resnet_3d.py:130,146 /
 *   audio_cond_unet_3d_condition.py:445, H*W for the per-frame GroupNorm of
 *   ff_spatio_audio_temp_transformer_3d.py:62) reduces (sum, sumsq) of each of `groups`
 *   channel groups over `nchunks` row chunks (deterministic, no atomics) into `scratch`
 *   (avsd_groupnorm_scratch_floats floats).  groups: a power of two in 4..64.  The input is the channel concat
 *   [x1 (c1 channels) | x2 (c2 channels)] (c2 may be 0) — the UNet skip concat is never
 *   materialised.
 * apply: every workgroup folds the partials of its batch (double, fixed order) into per-channel
 *   (scale, shift) = (rstd*gamma, beta - mean*rstd*gamma), biased variance, eps inside the sqrt, then streams
 *   y[m, c] = act( x * scale[c] + shift[c] ), act 0 none / 1 SiLU, bf16. */
int avsd_groupnorm_stats(const void* x1, int ld1, int c1, const void* x2, int ld2, int c2,
                         int nb, int rows_per_batch, int groups, float* scratch, int nchunks, void* stream);
int avsd_groupnorm_apply(const void* x1, int ld1, int c1, const void* x2, int ld2, int c2,
                         int nb, int rows_per_batch, int groups, const float* gamma, const float* beta, float eps,
                         const float* scratch, int nchunks, int act, void* y, int ldy, void* stream);
/* One-launch form for SMALL batches: a workgroup keeps whole groups (rows_per_batch rows x the channels of a few groups,
 * <= ~1900 16-byte vectors) in registers between the statistics and the apply: no scratch, no second read of the input.
 * Same arithmetic as the pair above (f32 sums per thread, folded in double in a fixed order; results differ from the pair
 * in the last bits only).  avsd_groupnorm_fused_supported(...) != 0 tells whether a geometry qualifies: the UNet's ResBlock
 * norms at 4 x 4 and its per-frame Transformer3D norms up to 16 x 16 do (5-7 us against 10-12 us for the pair); larger
 * batches are refused — too few workgroups own whole groups for the element-wise work (profiles/r3_gn_probe.txt).
 * Replaces the same reference sites as the pair. */
int avsd_groupnorm_fused_supported(int nb, int rows_per_batch, int groups, int c1, int c2, int split);
int avsd_groupnorm_fused(const void* x1, int ld1, int c1, const void* x2, int ld2, int c2, int nb, int rows_per_batch,
                         int groups, const float* gamma, const float* beta, float eps, int act, void* y, int ldy, void* stream);
/* Suggested nchunks, and the scratch size in floats for it (pure host arithmetic). */
int avsd_groupnorm_nchunks(int nb, int rows_per_batch, int channels);
int avsd_groupnorm_scratch_floats(int nb, int nchunks, int groups, int channels);

/* Pre-folds the row statistics of AVSD_GEMM_ROWSTATS: stats [M][nblk][2] -> out [M][2] (sum, sumsq over the whole row, added in ascending
 * block order).  An AVSD_GEMM_LNFUSE consumer given `out` with ln_nblk = 1 computes the same mean / rstd bit for bit without re-folding
 * nblk pairs per row in every column tile. */
int avsd_ln_fold(const float* stats, int M, int nblk, float* out, void* stream);
/* LayerNorm over the last dim (eps 1e-5 in the reference): y = LN(x + pos[f(m)]) with
 * pos == NULL for plain LN; f(m) = (m / hw) % frames.
 * (ff_spatio_audio_temp_transformer_3d.py:300,317,330,354,361) */
int avsd_layernorm(const void* x, int ldx, void* y, int ldy, int M, int C,
                   const float* gamma, const float* beta, float eps,
                   const float* pos, int hw, int frames, void* stream);

/* Row softmax: P[r, :] = softmax(S[r, :L]) ; S f32, P bf16 (VAE mid-block attention). */
int avsd_softmax_rows(const float* S, int lds, void* P, int ldp, int rows, int L, void* stream);

/* ---- attention -----------------------------------------------------------------------
 * Multi-head attention with queries [Bq][Lq] and keys/values [Bk][Lk]; query batch qb
 * attends to kv batch qb / q_per_kv (first-frame attention utils.py:133-153: q_per_kv =
 * frames, K/V computed for frame 0 only; audio / text cross-attention
 * ff_spatio_audio_temp_transformer_3d.py:319-341: K/V computed once per clip branch).
 * Head h occupies columns [h*d, (h+1)*d) of each row.  key_index (optional, int32
 * [frames][Lk]) gathers key rows for frame qb % frames — the boolean audio segment mask
 * (segmask_imagebind.py:104-114) turned into the list of unmasked keys.
 * kv_rows = rows per kv batch in the K/V buffers (229 audio tokens while Lk = 25 gathered).
 * softmax scale = scale (d^-1/2).  d in {40, 64, 80, 128, 160}. */
int avsd_attention(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv,
                   void* O, int ldo, int Bq, int Lq, int Lk, int kv_rows, int heads, int d,
                   int q_per_kv, const int32_t* key_index, int frames, float scale, void* stream);

/* FP8 (OCP e4m3) variant of avsd_attention — BASELINE.json configuration 5: Q, K, V and the probabilities are rounded to
 * e4m3 and both matrix products run on v_mfma_f32_32x32x16_fp8_fp8; softmax, running statistics and accumulation stay
 * f32.  Same tensors (16-bit in, 16-bit out), shapes and gather list as avsd_attention; q / k / v are multiplied by
 * q_scale / k_scale / v_scale before rounding (1.0 = raw values; |x| <= 448 is representable) and the scales are folded
 * back out.  Replaces the SDPA calls of utils.py:151-153 and ff_spatio_audio_temp_transformer_3d.py:315-341. */
int avsd_attention_fp8(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
                       int Bq, int Lq, int Lk, int kv_rows, int heads, int d, int q_per_kv,
                       const int32_t* key_index, int frames, float scale, float q_scale, float k_scale,
                       float v_scale, void* stream);

/* Temporal self-attention across frames for every pixel
 * (ff_spatio_audio_temp_transformer_3d.py:352-358): qkv is [B*F*hw][ldqkv] with q|k|v at
 * column offsets 0, C, 2C; sequence (b, p) = rows {(b*F + f)*hw + p : f}. */
int avsd_temporal_attention(const void* QKV, int ldqkv, void* O, int ldo, int B, int frames,
                            int hw, int heads, int d, float scale, void* stream);

/* ---- elementwise / layout ------------------------------------------------------------ */
/* (B, C, F, H, W) f32  ->  channels-last bf16 [rep*B*F*H*W][cpad] = scale * src, channels >= C
 * zeroed, the batch repeated `rep` times (torch.cat([latents] * k), pipeline...py:331-336). */
int avsd_ncfhw_to_rows(const float* src, void* dst, int B, int C, int F, int HW, int cpad,
                       int rep, float scale, void* stream);
/* channels-last f32 [B*F*HW][ld] (first C columns) -> (B, C, F, H, W) f32. */
int avsd_rows_to_ncfhw(const float* src, int ld, float* dst, int B, int C, int F, int HW,
                       void* stream);
/* Sinusoidal embedding, diffusers Timesteps(dim, flip_sin_to_cos=True, shift=0):
 * out[i, :] = [cos(t_i * w) | sin(t_i * w)], w_j = exp(-ln(1e4) * j / (dim/2)).
 * t is a device f32 array of n values. */
int avsd_timestep_embedding(const float* t, float* out, int n, int dim, void* stream);

/* Guidance + multistep scheduler update on (B, C, F, H, W) f32 latents, frame 0 pinned
 * (pipeline_audio_cond_animation.py:349-364):
 *   n_branch 1: eps = e[0]                                         (no guidance)
 *   n_branch 2: eps = e[0] + g * (e[1] - e[0])                     (:354-361; e = noise_pred of the [null-audio,
 *               audio] batch with g = audio scale, or of [null-text, text] with g = text scale)
 *   n_branch 3: eps = e[0] + g * (e[1] - e[0]) + g2 * (e[2] - e[1]) (:349-353, dual guidance; branches
 *               [uncond, text, text+audio], g = text_guidance_scale, g2 = audio_guidance_scale)
 *   eps_hist[store_slot] = eps                (if store_slot >= 0)
 *   eps'     = w_cur * eps + sum_k w[k] * eps_hist[hist_idx[k]]      (n_hist <= 4 terms)
 *   x_out[:, :, 1:] = ca * x_in[:, :, 1:] + cb * eps'[:, :, 1:] ;  x_out[:, :, 0] = x_in[:, :, 0]
 * PNDM (PLMS, incl. its averaged second step on the saved sample) and DDIM (eta = 0) are both
 * of this form; the scalar schedule lives on the host (asva_amd/schedulers.py). */
int avsd_guided_step(const float* noise_pred, int n_branch, float g, float g2, float* eps_hist,
                     int store_slot, float w_cur, const int32_t* hist_idx_host,
                     const float* w_host, int n_hist, const float* x_in, float* x_out, float ca,
                     float cb, int B, int C, int F, int HW, void* stream);

/* Guidance + DPM-Solver++ multistep update on (B, C, F, H, W) f32 latents, frame 0 pinned:
 *   eps      = guidance combine of noise_pred (n_branch 1 / 2 / 3, g, g2: exactly the rule of avsd_guided_step)
 *   d        = s_x * x_in + s_e * eps        (data prediction x0 = (x - sigma_t eps) / alpha_t: s_x = 1 / alpha_t,
 *                                             s_e = -sigma_t / alpha_t; s_x = 0, s_e = 1 gives eps itself)
 *   hist[store_slot] = d                     (if store_slot >= 0; hist holds slots of B*C*F*HW floats)
 *   x_out[:, :, 1:] = ca * x_in + c_cur * d + sum_k w[k] * hist[hist_idx[k]]   (n_hist <= 4 terms; the slot stored by
 *                                             this call is read from the value just computed) ;  x_out[:, :, 0] = x_in[:, :, 0]
 * x_in == x_out (in place) is allowed.  DPM-Solver++ 1M / 2M / 3M (asva_amd/schedulers.py DPMSolverMultistepScheduler,
 * coefficients on the host) is of this form; PNDM and DDIM stay on avsd_guided_step. */
int avsd_guided_multistep(const float* noise_pred, int n_branch, float g, float g2, float* hist, int store_slot,
                          const int32_t* hist_idx_host, const float* w_host, int n_hist, const float* x_in,
                          float* x_out, float ca, float c_cur, float s_x, float s_e, int B, int C, int F,
                          int HW, void* stream);

/* ---- random numbers (csrc/philox.h, csrc/rng.hip): integers and f32 in both builds ----
 * Philox4x32-10 as published by Random123 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten
 * rounds) with key = (seed lo, seed hi) and counter = (block lo, block hi, step, stream).  Item j of a sequence is lane j & 3 of
 * block j >> 2 (64-bit), so every item is a pure function of (seed, stream, step, j): a range may be produced in any partition,
 * with the same bits.
 *   avsd_philox4x32_u32:   out[k] = word first_word + k, 0 <= k < n_words
 *   avsd_randn_philox_f32: out[k] = normal first + k, 0 <= k < n.  Box-Muller in f32: with w0..w3 the words of a block,
 *       u = ((w0 >> 9) + 0.5) 2^-23 in (0, 1), v = (w1 >> 8) 2^-24 in [0, 1), r = sqrtf(-2 logf(u)),
 *       lane 0 = r cos(2 pi v), lane 1 = r sin(2 pi v) (sincospif(2v)); lanes 2 and 3 the same from w2, w3.  |z| <= 5.77.
 * first / first_word and the counts need not be multiples of 4; out needs 4-byte alignment.  A count of 0 launches nothing. */
int avsd_philox4x32_u32(uint32_t* out, int64_t n_words, uint64_t seed, uint32_t stream, uint32_t step, int64_t first_word,
                        void* hip_stream);
int avsd_randn_philox_f32(float* out, int64_t n, uint64_t seed, uint32_t stream, uint32_t step, int64_t first, void* hip_stream);

/* The stochastic forms of avsd_guided_step and avsd_guided_multistep (DDIM with eta > 0, SDE-DPM-Solver++): every argument of the
 * deterministic entry point, then the noise coefficient and the key of the step's normals.  With `acc` exactly the value the
 * deterministic entry point stores,
 *   x_out[b, c, f, p] = fmaf(c_noise, z, acc)   for f >= 1,   x_out[:, :, 0] = x_in[:, :, 0] bit-exact,
 * where z is normal j = (c (F - 1) + (f - 1)) HW + p (64-bit) of the sequence (seed, stream + b, step) above: block j >> 2, lane
 * j & 3.  The noise of batch row b is therefore avsd_randn_philox_f32(C (F - 1) HW, seed, stream + b, step) laid out as
 * (C, F - 1, H, W), the slice a loop hands to scheduler.step; frame 0 spends no normal, and a clip's noise does not depend on the
 * batch it sits in.  The normals are evaluated in registers: no noise buffer, no second launch.  History stores are those of the
 * deterministic entry points and x_in == x_out stays legal.  F == 1 copies x_in; c_noise == 0 gives the deterministic values.
 * stream + B must not exceed 2^32 (AVSD_EINVAL).  When HW % 4 == 0 and noise_pred, the history, x_in and x_out are 16-byte
 * aligned, a thread moves four elements of a frame row as one vector and evaluates one Philox block for them; otherwise one element
 * per thread.  Both paths give the same bits. */
int avsd_guided_step_sde(const float* noise_pred, int n_branch, float g, float g2, float* eps_hist, int store_slot, float w_cur,
                         const int32_t* hist_idx_host, const float* w_host, int n_hist, const float* x_in, float* x_out,
                         float ca, float cb, int B, int C, int F, int HW, float c_noise, uint64_t seed, uint32_t stream,
                         uint32_t step, void* hip_stream);
int avsd_guided_multistep_sde(const float* noise_pred, int n_branch, float g, float g2, float* hist, int store_slot,
                              const int32_t* hist_idx_host, const float* w_host, int n_hist, const float* x_in, float* x_out,
                              float ca, float c_cur, float s_x, float s_e, int B, int C, int F, int HW, float c_noise,
                              uint64_t seed, uint32_t stream, uint32_t step, void* hip_stream);

/* Guidance + UniPC step (corrector, then predictor) on (B, C, F, H, W) f32 latents, frame 0 pinned, one launch:
 *   eps  = guidance combine of noise_pred (n_branch 1 / 2 / 3, g, g2: exactly the rule of avsd_guided_step)
 *   d    = s_x * x_in + s_e * eps            (data prediction m_i of the PREDICTED sample x_in the UNet just saw)
 *   h_k  = hist[hist_idx[k]], k < n_hist     (n_hist <= 4; every slot is read before the store below)
 *   xc   = use_corrector ? cc_last * x_last + cc_cur * d + sum_k wc[k] * h_k : x_in      (the corrected sample)
 *   hist[store_slot] = d                     (if store_slot >= 0; it may be one of hist_idx: the oldest entry is replaced)
 *   x_last = xc                              (base of the next call's corrector)
 *   x_out  = cp_x * xc + cp_cur * d + sum_k wp[k] * h_k                                  (prediction for the next sigma)
 *   frame 0: x_out = x_in bit-exact, x_last = x_in
 * One index list serves both sums: a zero in wc or wp marks an entry only the other update uses; slots outside
 * hist_idx[0..n_hist) are never read.  x_out may alias x_in; x_last may alias neither (AVSD_EINVAL).
 * asva_amd/schedulers.py UniPCMultistepScheduler computes the coefficients on the host. */
int avsd_guided_unipc(const float* noise_pred, int n_branch, float g, float g2, float* hist, int store_slot,
                      const int32_t* hist_idx_host, const float* wc_host, const float* wp_host, int n_hist,
                      const float* x_in, float* x_out, float* x_last, int use_corrector, float s_x, float s_e,
                      float cc_last, float cc_cur, float cp_x, float cp_cur, int B, int C, int F, int HW,
                      void* stream);

/* Turnover between two chained windows of a long track (asva_amd/pipeline.py animate_track) on (B, C, F, H, W) f32 latents:
 *   x_next[:, :, 0]  = x_prev[:, :, F-1]      (bit-exact: the last finished frame conditions the next window)
 *   x_next[:, :, 1:] = noise * sigma          (noise (B, C, F-1, H, W) f32; sigma = the scheduler's init_noise_sigma)
 * x_next == x_prev (in place) is allowed: frame F-1 is read before frame 0 and frame F-1 are written.  x_next may otherwise
 * not overlap x_prev, and noise may not overlap x_next (AVSD_EINVAL).  Pointers need 4-byte alignment only; noise may be
 * NULL when F == 1.  One launch. */
int avsd_window_turnover(const float* x_prev, const float* noise, float* x_next, float sigma, int B, int C, int F, int HW,
                         void* stream);

/* ---- the training objective's forward value (asva_amd/trainer.py; kernels in csrc/loss.hip): f32 and integers in both builds ----
 * Noising step of audio_cond_animation_trainer.py:119-134 on contiguous (B, C, F, H, W) f32 tensors, one launch.  For sample b
 * with t = timesteps[b] (device int32), a = sqrt_acp[t], s = sqrt_1m_acp[t] (device f32 tables of T entries):
 *   noisy[b, :, f]  = x0[b, :, f]                 bit-exact, when keep_first and f == 0  (the trainer's first-frame splice)
 *                   = fma(a, x0, s * noise)       otherwise                              (scheduler.add_noise)
 *   target[b]       = noise[b]                    bit-exact, every frame, mode AVSD_DIFFUSE_EPSILON
 *                   = fma(a, noise, -(s * x0))    mode AVSD_DIFFUSE_V                    (scheduler.get_velocity)
 * target may be NULL (the caller uses noise itself, or wants add_noise only).  A sample whose timestep lies outside [0, T) is
 * left untouched: nothing of noisy[b] / target[b] is written and the tables are not read (asva_amd/ops.py validates the vector
 * and raises).  Pointers need 4-byte alignment only.  An output that overlaps an input or the other output is AVSD_EINVAL;
 * noisy == x0 is not allowed. */
#define AVSD_DIFFUSE_EPSILON 0
#define AVSD_DIFFUSE_V 1
int avsd_diffuse_clip_f32(const float* x0, const float* noise, const int32_t* timesteps, const float* sqrt_acp,
                          const float* sqrt_1m_acp, int T, float* noisy, float* target, int keep_first, int mode, int B, int C,
                          int F, int HW, void* stream);
/* Denoising loss on (B, C, F, H, W) f32 tensors (audio_cond_animation_trainer.py:145-148):
 *   per_sample[b] = mean((pred - target)[b, :, f0:]^2)        n = C * (F - f0) * HW terms
 *   loss[0]       = mean_b per_sample[b]                      = F.mse_loss on the sliced tensors (every sample has n terms)
 * f0 = 1 is the reference's default, 0 its loss_on_first_frame; 0 <= f0 < F.  Deterministic, no atomics, two launches: each
 * sample is cut into AVSD_FRAME_MSE_PARTS fixed pieces (by n alone), a workgroup folds its piece in f32 in a fixed tree and
 * writes scratch[b * AVSD_FRAME_MSE_PARTS + part]; the second launch folds a sample's partials in double in a fixed tree,
 * then the samples in index order.  per_sample[b] therefore depends neither on B nor on b.  scratch: B *
 * AVSD_FRAME_MSE_PARTS floats, caller-provided, overwritten.  Pointers need 4-byte alignment only. */
#define AVSD_FRAME_MSE_PARTS 64
int avsd_frame_mse_f32(const float* pred, const float* target, int f0, float* scratch, float* per_sample, float* loss, int B, int C,
                       int F, int HW, void* stream);

/* VAE post-processing (pipeline_audio_cond_animation.py:212): channels-last bf16
 * [N*H*W][ld] (3 channels) -> (N, 3, H, W) f32 = clamp(x / 2 + 0.5, 0, 1). */
int avsd_vae_postprocess(const void* src, int ld, float* dst, int N, int HW, void* stream);
/* Same input -> uint8 frames (N, H, W, 3) = trunc(clamp(x / 2 + 0.5, 0, 1) * 255): the post-processing above followed
 * by generate_videos' `(video.permute(0, 2, 3, 1) * 255).byte()` (pipeline_audio_cond_animation.py:448), on device —
 * 4x fewer bytes cross PCIe per clip. */
int avsd_vae_postprocess_u8(const void* src, int ld, void* dst_u8, int N, int HW, void* stream);

/* ---- audio conditioning front-end (once per clip, not on the denoising loop) --------------------------
 * Kaldi-compatible log-mel filterbank + transpose + pad/crop + normalisation: replaces
 * `waveform_to_melspectrogram` (avgen/data/utils.py:26-55) = ImageBind `waveform2melspec` (torchaudio.compliance.
 * kaldi.fbank: htk_compat, hanning window, dither 0, snip_edges) followed by `Normalize(mean, std)`.
 *   wave [batch][wave_stride] f32 (n_samples valid), window [win] f32, mel_fb [n_mel][nfft/2+1] f32 (host-built,
 *   asva_amd/audio_features.py) -> out [batch][n_mel][t_out] f32; frames past 1 + (n_samples - win) / shift are the
 *   normalised zero padding.  nfft must be a power of two; win <= 512. */
int avsd_kaldi_fbank(const float* wave, int batch, int n_samples, int64_t wave_stride, const float* window,
                     const float* mel_fb, int win, int shift, int nfft, int n_mel, float preemph, int remove_dc,
                     float* out, int t_out, float mean, float std, void* stream);
/* Polyphase windowed-sinc sample-rate conversion (torchaudio.functional.resample: avgen/data/utils.py:259,404,
 * compute_avsync.py:141,157), f32 in both builds.  `orig` : `new_` are the two rates divided by their gcd, taps
 * [new_][L] f32 with L = 2 * width + orig is the filter bank (host-built, asva_amd/audio_features.py:resample_taps):
 *   out[w][q * new_ + p] = sum_{k < L} taps[p][k] * xpad(w, q * orig + k - width)      for q * new_ + p < n_out,
 * xpad = x inside [0, n_in) and 0 outside (the kernel pads; it never reads outside a row).  x [n_wav][x_stride],
 * out [n_wav][out_stride]; n_out must be ceil(new_ * n_in / orig) and new_ * L at most 2^24.  Every output is one
 * k-ascending f32 fma chain: bits do not depend on n_wav or on the build. */
int avsd_resample_sinc_f32(const float* x, int n_wav, int n_in, int64_t x_stride, const float* taps, int orig, int new_,
                           int width, float* out, int n_out, int64_t out_stride, void* stream);
/* im2col of non-padded strided patches: src (B, C, H, W) f32 -> dst bf16 [B*ph*pw][C*kh*kw] (c-major, then kh, kw:
 * the order of a flattened nn.Conv2d weight).  Front of ImageBind's audio stem Conv2d(1, 768, 16, stride 10). */
int avsd_patchify(const float* src, void* dst, int B, int C, int H, int W, int kh, int kw, int stride, void* stream);
/* ViT token matrix: out bf16 [B][1 + n_patches + tail_rows][C]; row 0 = cls + pos[0], row 1+p = patches[b, p] + pos[1+p],
 * tail rows = 0 (the add_bias_kv slot of the ImageBind audio trunk's attention).  cls [C], pos [1+n_patches][C] f32. */
int avsd_vit_tokens(const void* patches, const float* cls, const float* pos, void* out, int B, int n_patches, int C,
                    int tail_rows, void* stream);

/* ---- device copies: with these, everything a denoising step does on the device is an entry point of this library
 *      (and therefore part of a launch plan, below) --------------------------------------------------------------------- */
/* dst[r * bytes + i] = src[i] for r in [0, rep): a device-to-device copy (rep = 1), or the torch.cat([x] * rep) along the
 * batch of guidance branches that are still identical (pipeline_audio_cond_animation.py:331-336).  bytes % 16 == 0. */
int avsd_copy(const void* src, void* dst, int64_t bytes, int rep, void* stream);
/* Cached cross-attention K|V rows  kv [n_kv * rows][2C] 16-bit  ->  the operand layout avsd_cross_attention_block stages:
 * k_out [nb][lk_pad][C] and vt_out [nb][C][lk_pad].  Without a gather list (idx == NULL) nb = n_kv and block n holds keys
 * 0..rows-1 of clip n; with idx [n_frames][nk] int32 (the visible keys of each frame under the audio segment mask,
 * audio_attn_mask in segmask_imagebind.py:104-114) nb = n_kv * n_frames and block n * n_frames + f holds keys idx[f][:] of
 * clip n.  The padding slots lk..lk_pad-1 (lk = nk or rows) are written as zeros by the same launch.  Once per clip. */
int avsd_xattn_pack_kv(const void* kv, int n_kv, int rows, int C, const int32_t* idx, int n_frames, int nk,
                       void* k_out, void* vt_out, int lk_pad, void* stream);

/* ---- split-precision ("x2") storage: the mode that meets north_star's 1e-3 against the reference's fp32 pipeline ----------
 * (scripts/animation_gen.py:43-44 runs fp32).  A 16-bit tensor becomes a PAIR of planes with identical strides:
 *     main = round16(v),  rest = round16(v - main)          (16 significant bits in bf16, no range loss)
 * `*_lo` arguments are the ELEMENT offsets from a main plane to its rest plane.  Matrix products run as three MFMA passes
 * (main.main + rest.main + main.rest; the rest.rest term is 2^-18 of the product) into the same f32 accumulator — the
 * GEMM family through AVSD_GEMM_X2, the attentions below — and every other kernel reconstructs v = main + rest (exact in
 * f32), computes in f32 as before and writes both planes.  Same arithmetic otherwise as the entry points they mirror. */
int avsd_linear_small_m_x2(const float* x, const void* W, int64_t w_lo, const float* bias, float* out,
                           int M, int N, int K, int ldw, int act_in, int act_out, void* stream);
int avsd_groupnorm_stats_x2(const void* x1, int ld1, int c1, int64_t x1_lo, const void* x2, int ld2, int c2, int64_t x2_lo,
                            int nb, int rows_per_batch, int groups, float* scratch, int nchunks, void* stream);
int avsd_groupnorm_fused_x2(const void* x1, int ld1, int c1, int64_t x1_lo, const void* x2, int ld2, int c2, int64_t x2_lo,
                            int nb, int rows_per_batch, int groups, const float* gamma, const float* beta, float eps, int act,
                            void* y, int ldy, int64_t y_lo, void* stream);
int avsd_groupnorm_apply_x2(const void* x1, int ld1, int c1, int64_t x1_lo, const void* x2, int ld2, int c2, int64_t x2_lo,
                            int nb, int rows_per_batch, int groups, const float* gamma, const float* beta, float eps,
                            const float* scratch, int nchunks, int act, void* y, int ldy, int64_t y_lo, void* stream);
int avsd_layernorm_x2(const void* x, int ldx, int64_t x_lo, void* y, int ldy, int64_t y_lo, int M, int C,
                      const float* gamma, const float* beta, float eps, const float* pos, int hw, int frames, void* stream);
int avsd_attention_x2(const void* Q, int ldq, int64_t q_lo, const void* K, int ldk, int64_t k_lo, const void* V, int ldv,
                      int64_t v_lo, void* O, int ldo, int64_t o_lo, int Bq, int Lq, int Lk, int kv_rows, int heads, int d,
                      int q_per_kv, const int32_t* key_index, int frames, float scale, void* stream);
int avsd_temporal_attention_x2(const void* QKV, int ldqkv, int64_t qkv_lo, void* O, int ldo, int64_t o_lo, int B, int frames,
                               int hw, int heads, int d, float scale, void* stream);
int avsd_softmax_rows_x2(const float* S, int lds, void* P, int ldp, int64_t p_lo, int rows, int L, void* stream);
int avsd_ncfhw_to_rows_x2(const float* src, void* dst, int64_t dst_lo, int B, int C, int F, int HW, int cpad, int rep,
                          float scale, void* stream);
/* f32 [n] -> planes (conditioning inputs: text / audio encodings handed over in f32). */
int avsd_split_f32(const float* src, void* dst, int64_t dst_lo, int64_t n, void* stream);
int avsd_vae_postprocess_x2(const void* src, int ld, int64_t src_lo, float* dst, int N, int HW, void* stream);
int avsd_vae_postprocess_u8_x2(const void* src, int ld, int64_t src_lo, void* dst_u8, int N, int HW, void* stream);

/* ---- exact-f32 yardstick ---------------------------------------------------------------------------------------------------
 * out[M, N] = A[M, K] . W[N, K]^T + bias[n], all f32, on the f32-input matrix cores (v_mfma_f32_32x32x2_f32: bitwise a
 * k-ordered fmaf chain, 157 TFLOP/s peak = 1/16 of the bf16 rate).  Not on the product path: it is the on-box reference that
 * separates kernel arithmetic from storage rounding when the 16-bit and split-precision GEMMs are validated, and the rate
 * bench.py quotes next to theirs.  The reference computes the same products with fp32 torch.nn.Linear / nn.Conv2d
 * (scripts/animation_gen.py:43-44).  K, lda, ldw multiples of 4; A, W 16-byte aligned. */
int avsd_gemm_f32(const float* A, int lda, const float* W, int ldw, const float* bias, float* out, int ldc, int M, int N, int K,
                  void* stream);

/* ---- AVSync scorer (asva_amd/avsync.py; csrc/avsync.hip) ---------------------------------------------------------------------
 * The reference's evaluation metric: the AVSync classifier (avsync/models/video.py R(2+1)D-18, audio.py 2-D conv net, head.py
 * 3-layer FC) and RelSync on top of it (avgen/evaluations/avsync/compute_avsync.py:37-68).  Everything is f32 on the f32-input
 * matrix cores in BOTH builds of the library, so a score does not depend on the storage mode of the clip it judges.
 * Tensors are channels-last: video activations [n][t][h][w][c], audio activations the same with t = 1.
 *
 * Implicit-GEMM convolution with arbitrary small taps, strides and zero padding; no im2col buffer:
 *   out[n, to, ho, wo, co] = act( sum_{dt, dh, dw, ci} x[n, to*st - pt + dt, ho*sh - ph + dh, wo*sw - pw + dw, ci]
 *                                                      * w[co*ldw + ((dt*kh + dh)*kw + dw)*cin + ci]
 *                                 + bias[co] + rscale[co] * res[n, to, ho, wo, co] ),   act = ReLU if `relu` else identity.
 * bias, res, rscale may be NULL (rscale NULL = 1; rscale needs res).  Eval-mode BatchNorm folds into w / bias / rscale at pack
 * time (video.py:38-43, audio.py:24-27).  With taps (1,1,1) and stride 1 this is A . W^T + b (head.py:14-22).  The output size
 * must follow from input size, window, stride and padding.  Deterministic: every output element is one k-ordered chain. */
int avsd_convnd_f32(const float* x, const float* w, const float* bias, const float* res, const float* rscale, float* out,
                    int n, int ti, int hi, int wi, int cin, int to, int ho, int wo, int cout, int kt, int kh, int kw,
                    int st, int sh, int sw, int pt, int ph, int pw, int ldw, int relu, void* stream);
/* avsd_convnd_f32 on channel slices of wider channels-last buffers: consecutive pixels of x are ldx >= cin elements apart, those of
 * out ldy >= cout, and x / out point at the first channel of their slice.  res, if given, is addressed with ldy as well (it has the
 * layout of out).  A branch of an Inception block (asva_amd/fid.py) writes straight into its slice of the block's concatenated
 * output, and a convolution reads its slice of what a stacked 1 x 1 convolution produced: there is no concat or copy kernel.
 * Channels >= cin of an input pixel are never read and columns >= cout of an output row never written.  The arithmetic is that of
 * avsd_convnd_f32 bit for bit (the same chain per output element; only addresses differ).  The float4 loader is taken when
 * cin % 32 == 0, ldw % 4 == 0, ldx % 4 == 0 and x, w are 16-byte aligned; any other slice falls back to the scalar loader, which
 * gives the same bits. */
int avsd_convnd_ld_f32(const float* x, int ldx, const float* w, const float* bias, const float* res, const float* rscale, float* out,
                       int ldy, int n, int ti, int hi, int wi, int cin, int to, int ho, int wo, int cout, int kt, int kh, int kw,
                       int st, int sh, int sw, int pt, int ph, int pw, int ldw, int relu, void* stream);
/* The 3 x 3 pools of Inception-v3 on [n_img][hi][wi][c] -> [n_img][ho][wo][c], pixels ldx / ldy elements apart (channel slices as
 * above; c, ldx, ldy multiples of 4, pointers 16-byte aligned).  (stride, pad) is (2, 0) or (1, 1) and the output size must follow
 * from it.  avg = 0: maximum, exact; padded positions do not take part (F.max_pool2d).  avg = 1: the taps inside the image summed in
 * (dy, dx) order, divided by their number 4, 6 or 9 (F.avg_pool2d(count_include_pad=False), inception_v3.py:228). */
int avsd_pool3_hw_f32(const float* x, int ldx, float* out, int ldy, int n_img, int hi, int wi, int c, int ho, int wo, int stride,
                      int pad, int avg, void* stream);
/* avsd_convnd_ld_f32 with TensorFlow "same" zero padding (I3D, asva_amd/fvd.py; pytorch_i3d.py:73-98 of the reference), worked out
 * inside from input size, window and stride, per axis: total = max(k - s, 0) if size % s == 0, else max(k - size % s, 0); total / 2
 * (rounded down) in front, the rest behind; output ceil(size / s), which the caller passes as to, ho, wo (anything else is refused).
 * The padding is asymmetric for even windows or strides > 1 (the 7 x 7 x 7 stride-2 stem on an even axis: 2 in front, 3 behind).  No
 * residual.  For a stride-1 odd window the padding is (k - 1) / 2 on both sides and the result equals avsd_convnd_ld_f32 bit for bit.
 * loader: 0 picks, 1 scalar (always legal), 2 float4 (cin % 32 == 0, ldx % 4 == 0, ldw % 4 == 0, x and w 16-byte aligned), 3 run
 * (ldx == cin, ldw % 4 == 0, w 16-byte aligned: the kw * cin floats of one (dt, dh) row of the window are contiguous and are
 * fetched four at a time with 4-byte-aligned wide loads, element by element at run boundaries, the w borders and the K tail — made
 * for the stem, cin = 3, K = 1029); an illegal choice is refused.  0 takes 2 where legal, else 1: on the stem the run loader measured
 * 2 % behind the scalar one (profiles/fvd.md), so it is never picked and stays for A/Bs.  Every loader gives the same bits: each
 * output element is the k-ordered chain 0 .. K-1. */
int avsd_conv3d_same_f32(const float* x, int ldx, const float* w, const float* bias, float* out, int ldy, int n, int ti, int hi, int wi,
                         int cin, int to, int ho, int wo, int cout, int kt, int kh, int kw, int st, int sh, int sw, int ldw, int relu,
                         int loader, void* stream);
/* Max pool with "same" padding on [n][ti][hi][wi][c] -> [n][to][ho][wo][c], pixels ldx / ldy elements apart (channel slices; c, ldx,
 * ldy multiples of 4, pointers 16-byte aligned).  Windows 1 .. 3 and strides 1 .. 2 per axis; to, ho, wo must be ceil(size / stride).
 * A padded position takes part in the maximum as 0.0f: the reference pads with F.pad and then pools without padding
 * (pytorch_i3d.py:17-36), unlike avsd_pool3_hw_f32 and avsd_maxpool_hw_f32.  Exact. */
int avsd_maxpool3d_same_f32(const float* x, int ldx, float* out, int ldy, int n, int ti, int hi, int wi, int c, int to, int ho, int wo,
                            int kt, int kh, int kw, int st, int sh, int sw, void* stream);
/* nn.MaxPool3d((1,3,3), stride (1,2,2), padding (0,1,1)) (video.py:62) on [n_img][hi][wi][c] -> [n_img][ho][wo][c]; padded
 * positions do not take part.  c a multiple of 4. */
int avsd_maxpool_hw_f32(const float* x, float* out, int n_img, int hi, int wi, int c, int ho, int wo, void* stream);
/* x [n][rows][c] -> out [n][c] = mean over rows (video.py:80, audio.py:60); fixed summation order, no atomics. */
int avsd_mean_rows_f32(const float* x, float* out, int n, int rows, int c, void* stream);
/* Video preprocessing of compute_avsync.py:14-34: frames x (n_img, 3, hi, wi) f32 in [0, 1] -> out [n_img][ho][wo][3] =
 * (antialiased bicubic resize - mean[c]) / std[c]; `crop` is the centre-crop size and must equal ho and wo (a no-op, as in the
 * reference after its exact 224 x 224 resize).  The taps come from the host (asva_amd/avsync.py resize_tables): output row oy reads
 * input rows y_start[oy] .. + y_count[oy] with weights y_weight[oy*y_taps + j]; columns likewise.  tmp: n_img*3*hi*wo floats. */
int avsd_resize_aa_normalize_f32(const float* x, float* tmp, float* out, int n_img, int hi, int wi, int ho, int wo,
                                 const int* y_start, const int* y_count, const float* y_weight, int y_taps,
                                 const int* x_start, const int* x_count, const float* x_weight, int x_taps, int crop,
                                 float mean0, float mean1, float mean2, float std0, float std1, float std2, void* stream);
/* The FC head on a MATRIX of pairs (csrc/avsync_pairs.hip): scripts/avsync_eval.py:138-148 scores one audio against k videos and k
 * audios against one video, avsync/models/sync_contrastive_trainer.py:35-38 all k x k pairs of an example.  The head's first layer is
 * linear in cat(a, v), so with U[g, p] = Wa . a[g, p] and Vh[g, q] = Wv . v[g, q] + b1 (two avsd_convnd_f32 calls on the column
 * halves of the packed W1 [H1][2 D]: ldw = 2 D, cin = D, the weight pointer at column 0 and at column D, no ReLU)
 *   scores[(g * P + p) * Q + q] = b3[0] + sum_n w3[n] * relu(b2[n] + sum_k W2[n * ldw2 + k] * relu(U[g, p, k] + Vh[g, q, k]))
 * for g < G, p < P, q < Q, n < H2, k < H1.  U [G][P][H1], Vh [G][Q][H1], W2 [H2][ldw2 >= H1], b2 [H2], w3 = row 0 of the last
 * layer's weight (the reference reads [:, 0]), b3 its bias (element 0 is read); b2 and b3 may be NULL (zero).  One launch: rows of
 * the product are pairs, it runs on v_mfma_f32_32x32x2_f32 with relu(U + Vh) formed on the way into the fragments; neither the
 * (G P Q, 2 D) concatenation nor the (G P Q, H1) hidden layer exists in memory.  The sum over k is the k-ordered chain 0 .. H1-1,
 * the sum over n a fixed tree (by H2 alone): a pair's score depends on its U row, its Vh row and the weights only — not on G, P, Q
 * or on where the pair sits.  H1 a multiple of 32, H2 a multiple of 32 up to 256 (the real head: 512 / 256), ldw2 a multiple of 4,
 * U, Vh, W2 16-byte aligned; anything else is AVSD_EINVAL before a launch (asva_amd/avsync.py then takes the materialised path).
 * Exactly G * P * Q floats are written. */
int avsd_pair_head_f32(const float* U, const float* Vh, const float* W2, int ldw2, const float* b2, const float* w3, const float* b3,
                       float* scores, int G, int P, int Q, int H1, int H2, void* stream);
/* The contrastive objective on a score matrix scores [G][P][Q] (sync_contrastive_trainer.py:40-53), x = scores * inv_tau:
 *   row_loss[g, p]   = -log softmax_q(x[g, p, :])[p]           written when P <= Q (the label of row p is q = p)
 *   col_loss[g, q]   = -log softmax_p(x[g, :, q])[q]           written when Q <= P
 *   row_argmax[g, p] = argmax_q scores[g, p, q], col_argmax[g, q] = argmax_p scores[g, p, q]      int32, always written;
 *                      a tie goes to the lowest index
 *   means[0 .. 3]    = av_loss = mean row_loss, va_loss = mean col_loss, av_acc = mean(row_argmax[g, p] == p), va_acc = mean(
 *                      col_argmax[g, q] == q)                  written when P == Q
 * The maximum is subtracted before exp, so scores of any finite size give a finite loss, and a 1 x 1 matrix gives exactly 0.
 * Deterministic, no atomics, two launches (one when P != Q): a wave folds each line in f32 in a fixed tree; the means are folded
 * in double in a fixed tree.  A line's loss and argmax therefore depend neither on G nor on g.  Pointers of outputs that are not
 * written may be NULL; outputs may overlap neither scores nor each other. */
int avsd_pair_xent_f32(const float* scores, float inv_tau, float* row_loss, float* col_loss, int32_t* row_argmax, int32_t* col_argmax,
                       float* means, int G, int P, int Q, void* stream);

/* ---- CLIP text encoder (asva_amd/text_encoder.py; csrc/clip_text.hip) --------------------------------------------------------
 * The text_encoder of Stable Diffusion 1.5 (CLIP ViT-L/14 text tower: token + position embedding, 12 pre-LN blocks with causal
 * self-attention and a quick-GELU MLP, final LayerNorm), which the reference calls through transformers
 * (avgen/pipelines/pipeline_audio_cond_animation.py:83-119).  Everything is f32 on the f32-input matrix cores in BOTH builds of
 * the library: a conditioning tensor does not move with the storage mode of the clip it conditions.  The linear layers are
 * avsd_convnd_f32 with taps (1,1,1) (q|k|v as one fused [3C][C] weight, out_proj + residual, fc1, fc2 + residual).
 *
 * out[b*L + l][:] = tok[ids[b*L + l]][:] + pos[l][:]; ids int32 [B*L], tok f32 [V][C], pos f32 [L][C], out f32 [B*L][C].  The host
 * checks 0 <= id < V before upload (the entry point cannot see device data); the kernel clamps an id into the table. */
int avsd_embed_tokens_f32(const int* ids, const float* tok, const float* pos, float* out, int B, int L, int C, int V, void* stream);
/* Row LayerNorm in f32: y[m][c] = (x[m][c] - mean_m) * rsqrt(var_m + eps) * gamma[c] + beta[c], two-pass variance
 * (mean first, kept as a rounded value plus its correction, then the mean of squared deviations).  ldx / ldy are row strides in elements; y may equal x. */
int avsd_layernorm_f32(const float* x, int ldx, float* y, int ldy, int M, int C, const float* gamma, const float* beta, float eps,
                       void* stream);
/* Causal self-attention of B sequences of length L: O[b*L + i][h*d + :] = sum_{j <= i} softmax_j(scale * Q_i . K_j) V_j over the keys
 * of the SAME sequence.  Row r of Q / K / V / O is at r * ld{q,k,v,o} (elements), head h in columns [h*d, (h+1)*d): Q, K and V are
 * usually views into one fused [B*L][3C] buffer.  Both products on v_mfma_f32_32x32x2_f32, softmax in f32; key tiles wholly above
 * the diagonal of a query tile are skipped.  One workgroup per (sequence, head): a row's result does not depend on the batch it
 * sits in, and every output element is one fixed-order chain.  Built for d == 64 and 1 <= L <= 128.
 * K and V must be FINITE: a key j > i inside the 32-key tile that holds the diagonal gets probability 0 exactly, but its V row still
 * enters the matrix product as 0 * V_j, and its K row a product that is then masked; an inf or NaN there gives NaN in row i. */
int avsd_attention_causal_f32(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo, int B,
                              int L, int heads, int d, float scale, void* stream);
/* y[i] = x[i] * sigmoid(1.702 x[i]) (CLIP's quick-GELU), i < n; y may equal x. */
int avsd_quick_gelu_f32(const float* x, float* y, int64_t n, void* stream);

/* ---- ImageBind evaluation towers: CLIPSim and AlignSync (asva_amd/imagebind_eval.py; csrc/imagebind_eval.hip) -------------------
 * The reference scores a clip with ImageBind-Huge embeddings (avgen/evaluations/models/clip.py:23-80): a ViT-H/14 vision tower
 * (257 tokens, 32 blocks, 16 heads of 80), an OpenCLIP-H text tower (77 tokens, causal: avsd_attention_causal_f32) and the audio
 * trunk (229 tokens + the bias_kv pair, 12 heads of 64).  f32 on the f32-input matrix cores in BOTH builds of the library, bit for
 * bit the same: a metric does not move with the storage mode of the clip it judges.  Linear layers and patch embeddings are
 * avsd_convnd_f32, LayerNorm is avsd_layernorm_f32.
 *
 * Bidirectional self-attention of B sequences of length L: O[b*L + i][h*d + :] = sum_j softmax_j(scale * Q_i . K_j) V_j over ALL keys
 * of the same sequence.  Row r of Q / K / V / O is at r * ld{q,k,v,o} (elements), head h in columns [h*d, (h+1)*d): Q, K and V are
 * usually views into one fused [B*L][3C] buffer.  Grid (128-query block, head, sequence); K and V stream through LDS in 64-key tiles
 * with a running maximum and denominator per query, so L is not bounded by LDS.  Both products on v_mfma_f32_32x32x2_f32, softmax in
 * f32 with libm's expf.  Keys past L get weight exactly 0, query rows past L are never stored, and for d = 80 the pad to the 32-channel
 * MFMA tile is zeros held in LDS: no column outside the head is read.  Every output element is one chain in a fixed key order: the
 * result of a row does not depend on B, on the query block it lands in, or on the build.  Built for d == 64 and d == 80, L >= 1.
 * K, V and O must be 16-byte aligned with row strides a multiple of 4. */
int avsd_attention_f32(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo, int B, int L,
                       int heads, int d, float scale, void* stream);
/* y[i] = 0.5 x[i] (1 + erf(x[i] / sqrt 2)) (erf-GELU, torch's F.gelu default), i < n; y may equal x.  Finite for any finite x. */
int avsd_gelu_f32(const float* x, float* y, int64_t n, void* stream);
/* avsd_vit_tokens in f32: patches f32 [B*n_patches][C], cls f32 [C], pos f32 [1 + n_patches][C] ->
 * out f32 [B*(1 + n_patches + tail_rows)][C]: row 0 = cls + pos[0], rows 1.. = patches + pos[1..], tail rows = 0 (the audio trunk keeps
 * one spare row per clip for its bias_kv pair). */
int avsd_vit_tokens_f32(const float* patches, const float* cls, const float* pos, float* out, int B, int n_patches, int C, int tail_rows,
                        void* stream);
/* out[i] = <x_i, y_{i / rep}> / (max(|x_i|, 1e-12) * max(|y_{i / rep}|, 1e-12)), i < m: the cosine of row i of x f32 [m][C] and row
 * i / rep of y f32 [m / rep][C] with the norms of F.normalize (a zero row gives 0).  rep must divide m: one audio or text embedding
 * per clip is broadcast over that clip's rep frames.  One wave per row, fixed summation order. */
int avsd_cosine_rows_f32(const float* x, const float* y, float* out, int m, int C, int rep, void* stream);
/* y[i][:] = x[i][:] / max(|x_i|, 1e-12) for the m rows of x f32 [m][C] (F.normalize); y may equal x.  One wave per row, the summation
 * order of avsd_cosine_rows_f32: a row's result does not depend on m. */
int avsd_normalize_rows_f32(const float* x, float* y, int m, int C, void* stream);

/* ---- baseline JPEG encoder for the Motion-JPEG clip writer (csrc/jpeg.hip; asva_amd/video_io.py:encode_jpeg_frames) -------
 * Baseline sequential DCT, 8-bit, three components, 4:4:4: one MCU is one Y, one Cb and one Cr block, MCUs in raster order,
 * no restart markers, the Huffman tables of Annex K.3-K.6.  f32 and integer arithmetic only: both builds give the same bytes.
 * Markers, FF byte stuffing and the container are the caller's (FF -> FF 00 over the entropy-coded bytes). */
#define AVSD_JPEG_SLOT_BYTES 212  /* code string of one block: at most 20 + 63 * 26 bits, rounded up to whole 32-bit words */
/* frames u8 [n][H][W][3] (R, G, B) -> coef i16 [n][H/8][W/8][3][64], the quantised coefficients of Y, Cb, Cr in zigzag order:
 * JFIF full-range YCbCr (Y = .299 R + .587 G + .114 B, Cb = -.168735892 R - .331264108 G + .5 B + 128,
 * Cr = .5 R - .418687589 G - .081312411 B + 128), level shift by -128, orthonormal 8 x 8 DCT-II in f32, IEEE division by the
 * table entry, rounding half away from zero.  qy / qc: the luminance / chrominance quantisation tables, 64 u16 each on the
 * device, in NATURAL order (row-major 8 x 8; a DQT segment carries them in zigzag order).  H and W must be multiples of 8,
 * frames 8-byte aligned.  A block's coefficients do not depend on n or on its neighbours. */
int avsd_jpeg_quantize_u8(const void* frames_u8, int n, int H, int W, const uint16_t* qy, const uint16_t* qc, int16_t* coef,
                          void* stream);
/* coef i16 [n][blocks_per_frame][64] as written above (blocks_per_frame = 3 x the MCUs of a frame, block b belongs to component
 * b % 3) -> the entropy-coded segment of each frame at out_u8 + f * out_stride, unstuffed, the last byte padded with 1-bits,
 * and its length in nbytes[f].  The DC predictor is per component and starts at 0 in every frame; runs above 15 emit ZRL; EOB
 * is emitted unless coefficient 63 is non-zero; bits are written MSB first.  Baseline range is assumed (DC differences within
 * +-2047, AC within +-1023; values outside are clamped).  out_stride: a multiple of 4, at least blocks_per_frame *
 * AVSD_JPEG_SLOT_BYTES (the worst case); the entry point zeroes what it uses, bytes past nbytes[f] are not written.
 * scratch: at least n * blocks_per_frame * (AVSD_JPEG_SLOT_BYTES + 8) bytes on the device.  Three launches: code strings per
 * block, an exclusive scan of their bit lengths per frame, and the shift of every string to its bit offset; words shared by
 * neighbouring blocks are joined with integer atomic OR, so the bytes are a pure function of the coefficients. */
int avsd_jpeg_pack_i16(const int16_t* coef, int n, int blocks_per_frame, void* scratch, int64_t scratch_bytes, void* out_u8,
                       int64_t out_stride, int32_t* nbytes, void* stream);

/* ---- baseline JPEG decoder for the clip readers (csrc/jpeg.hip; asva_amd/video_io.py:decode_jpeg_frames) --------------------
 * Baseline sequential DCT, 8-bit, three components, one interleaved scan, no restart markers; 4:4:4 (an MCU is Y, Cb, Cr) or
 * 4:2:0 (an MCU is four Y blocks in raster order, Cb, Cr).  Integer arithmetic only: both builds give the same bytes, and for a
 * stream an encoder made from pixels they are the bytes libjpeg-turbo returns.  Markers, the removal of FF 00 stuffing and the
 * construction of the Huffman decode tables are the caller's. */
#define AVSD_JPEG_444 0
#define AVSD_JPEG_420 1
#define AVSD_JPEG_MAX_SCAN_BITS (1 << 30)
/* One Huffman table as 32-bit words: lut[256] indexed by the next 8 bits, (length << 8) | symbol for codes of up to 8 bits, else
 * 0; limit[16], limit[l - 1] = the first 16-bit left-aligned value that no code of length <= l starts; offset[16],
 * offset[l - 1] = (index in HUFFVAL of the first code of length l) - (that code), so that code + offset indexes HUFFVAL;
 * vals[64]: HUFFVAL as 256 bytes, little-endian in the words.  A set is [component 0..2][DC, AC]. */
#define AVSD_JPEG_HUFF_WORDS 352
#define AVSD_JPEG_HUFF_SET_WORDS (6 * AVSD_JPEG_HUFF_WORDS)
/* bits of status[f]; 0 = the frame decoded */
#define AVSD_JPEG_BAD_CODE 1    /* a prefix no code of the table has (the decoder moved on by one bit)                     */
#define AVSD_JPEG_TOO_MANY 2    /* more than blocks_per_frame blocks (nothing was written for them)                        */
#define AVSD_JPEG_BAD_INDEX 4   /* a run that leads behind coefficient 63                                                  */
#define AVSD_JPEG_INCOMPLETE 8  /* not exactly blocks_per_frame whole blocks                                               */
#define AVSD_JPEG_BAD_TAIL 16   /* eight or more bits, or a zero bit, behind the last block                                */
#define AVSD_JPEG_BAD_ARGS 32   /* offset, bit length or table index of the frame out of range: nothing was read           */
/* scan: the n entropy-coded segments, stuffing removed, frame f at byte offsets[f] (a multiple of 4) with nbits[f] bits (8 x its
 * bytes, at most AVSD_JPEG_MAX_SCAN_BITS); behind every segment at least 8 bytes of padding inside scan_bytes (any value: bits
 * behind the end read as ones).  table_index[f] < n_tables selects the frame's set in tables u32 [n_tables][SET_WORDS].
 * offsets i64, nbits / table_index i32, all on the device.  -> coef i16 [n][blocks_per_frame][64] in zigzag order, blocks in
 * scan order, DC values absolute (the predictor is per component and starts at 0 in every frame); status i32 [n]; rounds i32 [n]
 * or NULL: the largest number of re-decoding rounds any chunk of the frame needed.  coef 16-byte aligned.
 * One launch, one workgroup of 1024 lanes per frame: the scan is cut into subsequences of subseq_bits bits (a power of two in
 * 128..4096), 1024 at a time; each lane decodes one from a guessed state, lanes whose predecessor ended elsewhere decode again
 * until nothing changes (at most 1023 rounds), a prefix sum of the completed blocks places the stores of a last pass, and a
 * per-component prefix sum undoes the DC prediction.  The result does not depend on subseq_bits.  Every loop is bounded by the
 * bit length; a symbol that would end behind the last bit is not decoded; every store is index-checked, so a damaged stream
 * sets status[f] and writes only inside frame f's coefficients.  The checks of this entry point cover the host arguments; the
 * per-frame device arguments are checked by the kernel (AVSD_JPEG_BAD_ARGS). */
int avsd_jpeg_decode_scan(const void* scan, int64_t scan_bytes, const int64_t* offsets, const int32_t* nbits, const int32_t* table_index,
                          const uint32_t* tables, int n_tables, int n, int blocks_per_frame, int sampling, int subseq_bits, int16_t* coef,
                          int32_t* status, int32_t* rounds, void* stream);
/* coef as written above for n frames of H x W (blocks_per_frame = MCUs x 3 or 6, MCUs = ceil(H / 8v) x ceil(W / 8v), v = 1 for
 * 4:4:4 and 2 for 4:2:0) -> frames u8 [n][H][W][3] (R, G, B).  qtabs u16 [n_qsets][3][64]: the quantisation table of each
 * component in ZIGZAG order (as a DQT segment carries it); q_index i32 [n] on the device selects a frame's set (out of range:
 * set 0).  planes: scratch of at least n x MCUs x 64 x (v * v + 2) bytes, 8-byte aligned.  Two launches.  The first dequantises
 * and runs libjpeg's "islow" IDCT (13-bit constants, descaling by 11 bits down the columns and by 18 along the rows, + 128,
 * clamped) into whole-MCU planes; products, i0 +- i4, z3, z4 wrap to 16 bits, pass results saturate to 16 bits and a block
 * without AC in rows 1..7 is row 0 << 2, as in libjpeg-turbo's vector code (no-ops for streams made from pixels).  The second
 * upsamples 4:2:0 chroma with libjpeg's triangle filter over the ceil(H/2) x ceil(W/2) real samples (edges repeated) and
 * converts with R = Y + ((91881 Cr + 32768) >> 16), G = Y + ((-22554 Cb - 46802 Cr + 32768) >> 16),
 * B = Y + ((116130 Cb + 32768) >> 16), Cb and Cr less 128, clamped. */
int avsd_jpeg_idct_rgb_u8(const int16_t* coef, int n, int H, int W, int sampling, const uint16_t* qtabs, int n_qsets, const int32_t* q_index,
                          void* planes, int64_t planes_bytes, void* frames_u8, void* stream);

/* ---- launch plans (a host without Python runs the path) ----------------------------------------------------
 * A plan is the sequence of calls to the entry points above that one operation of the reference issues — the UNet forward
 * of a denoising step (audio_cond_unet_3d_condition.py:598-798), the per-clip conditioning projections, the VAE decode
 * (pipeline_audio_cond_animation.py:206-213) — for ONE geometry (network config, latent shape, guidance branches), with
 * every device pointer expressed as (buffer, byte offset).  asva_amd/plan.py records plans from the Python host (which owns
 * the network description) and writes a bundle: a buffer table shared by all its plans + the call lists.  Any host then
 *   loads the bundle, allocates (or maps) the buffers, binds them, uploads weights and inputs, and calls avsd_plan_run:
 * the same kernels with the same arguments as the recording run, so the results are bit-identical to the Python host's.
 * tools/plan_host.cpp is such a host (C++, no Python, no torch).
 * Memory model: the bundle's BUFFERS are the device allocations of the recording run (the caching allocator's segments, with
 * their sizes); a replaying host allocates each one zero-filled and binds it.  Named REGIONS (buffer, offset, bytes, kind) say
 * where in those buffers the things a host touches live: */
enum { AVSD_REGION_CONST = 1,    /* weights and tables: contents ship with the bundle (<bundle>.d/<name>.bin); upload once */
       AVSD_REGION_INPUT = 2,    /* written by the host before a run (latents, timestep, conditioning embeddings)         */
       AVSD_REGION_OUTPUT = 3 }; /* read by the host after a run (noise prediction, decoded frames)                       */
typedef struct avsd_plan_bundle avsd_plan_bundle;
int avsd_plan_bundle_load(const char* path_host, avsd_plan_bundle** out_host);
void avsd_plan_bundle_free(avsd_plan_bundle* b);
int avsd_plan_bundle_num_buffers(const avsd_plan_bundle* b);
int64_t avsd_plan_bundle_buffer_bytes(const avsd_plan_bundle* b, int i);                 /* -1 for a bad index */
int avsd_plan_bundle_bind(avsd_plan_bundle* b, int i, void* device_ptr);               /* 256-byte aligned */
int avsd_plan_bundle_num_regions(const avsd_plan_bundle* b);
/* region j: its name (lives as long as the bundle), the buffer it is in, its byte offset and size, its kind */
int avsd_plan_bundle_region(const avsd_plan_bundle* b, int j, const char** name_host, int* buffer_host, int64_t* offset_host,
                            int64_t* bytes_host, int* kind_host);
int avsd_plan_bundle_find_region(const avsd_plan_bundle* b, const char* name_host);    /* index, or -1 */
int avsd_plan_bundle_num_plans(const avsd_plan_bundle* b);
const char* avsd_plan_bundle_plan_name(const avsd_plan_bundle* b, int k);
int avsd_plan_bundle_find_plan(const avsd_plan_bundle* b, const char* name_host);       /* index, or -1 */
int avsd_plan_num_calls(const avsd_plan_bundle* b, int plan);
/* Issues every call of plan `plan` on `stream`, in recording order.  All buffers the plan touches must be bound.
 * Capturable in a hipGraph like the calls themselves.  A bundle is not thread-safe (run patches the stream into its
 * argument lists): one bundle per host thread; bundles on distinct streams are independent. */
int avsd_plan_run(avsd_plan_bundle* b, int plan, void* stream);

/* Operation-level calls on a bundle recorded with the conventional region names (tools/export_plan.py) — the surface
 * SURVEY 8(b)-3 sketched, for hosts that do not want to handle regions themselves.  All pointers are DEVICE pointers of the
 * regions' sizes (the 16-bit CFG-batched text / audio encodings, f32 latents, one f32 timestep); every call only enqueues
 * work on `stream`.  avsd_unet_set_conditioning: audio_cond_unet_3d_condition.py:598-798's step-invariant part, once per clip
 * ("text", "audio" -> plan "set_conditioning").  avsd_unet_forward: one UNet evaluation of the CFG batch ("x", "t" -> plan
 * "forward" -> "noise_pred"; noise_pred_out may be NULL: read the region instead).  avsd_vae_decode:
 * pipeline_audio_cond_animation.py:206-213 + :448 ("latents" -> plan "decode" -> uint8 "frames").  The guidance + scheduler
 * update between two forwards is avsd_guided_step.  avsd_plan_region_ptr: device address (and size) of a region in the
 * bound buffers, NULL if absent or unbound.
 * A "forward" plan bakes in the launch sequence of its recording run, including the shared guidance prefix: when the recording
 * host saw the SAME text rows in every guidance branch (audio-only guidance, text [t, t], pipeline_audio_cond_animation.py:155)
 * the layers in front of the first audio cross-attention were recorded once for all branches.  Such a bundle is valid only for
 * text inputs with that property; record with AVSD_SHARE_PREFIX=0 for per-branch text (text or dual guidance).  The region
 * "share_prefix" (4 bytes, CONST: 1 = the prefix is shared) states which kind a bundle is. */
int avsd_unet_set_conditioning(avsd_plan_bundle* b, const void* text, const void* audio, void* stream);
int avsd_unet_forward(avsd_plan_bundle* b, const float* sample, const float* timestep, float* noise_pred_out, void* stream);
int avsd_vae_decode(avsd_plan_bundle* b, const float* latents, void* frames_u8_out, void* stream);
const void* avsd_plan_region_ptr(avsd_plan_bundle* b, const char* name_host, int64_t* bytes_host);

#ifdef __cplusplus
}
#endif
#endif /* AVSD_H */
