// Baseline JPEG encoder for the Motion-JPEG clip writer (asva_amd/video_io.py:encode_jpeg_frames): 8-bit, three components,
// 4:4:4, one MCU = one Y, one Cb and one Cr block, raster order, no restart markers, the Annex K Huffman tables.  Two stages,
// exported separately (include/avsd.h):
//   avsd_jpeg_quantize_u8   frames u8 -> JFIF YCbCr -> level shift -> 8 x 8 DCT-II in f32 -> quantise -> zigzag, i16
//   avsd_jpeg_pack_i16      coefficients -> one entropy-coded stream per frame (unstuffed, last byte padded with 1-bits)
// f32 and integer arithmetic only: the same instructions in both builds of the library, so the same bytes.  Headers, FF
// byte stuffing and the container are the host's.
// And the baseline JPEG decoder of the clip readers (asva_amd/video_io.py:decode_jpeg_frames), 4:4:4 and 4:2:0, integers only:
//   avsd_jpeg_decode_scan   unstuffed entropy-coded scans -> coefficients i16 (subsequence-parallel Huffman decoding)
//   avsd_jpeg_idct_rgb_u8   coefficients -> dequantise -> libjpeg's integer IDCT -> chroma upsampling -> RGB u8
// Its contract is the bytes libjpeg-turbo (PIL) returns for the same stream.
#include "avsd_common.h"

namespace {

constexpr int JQ_THREADS = 256;                 // 4 waves, one MCU each
constexpr int JP_THREADS = 256;                 // 4 waves, one block each
constexpr int JP_SCAN_THREADS = 256;
constexpr int JP_SLOT_WORDS = AVSD_JPEG_SLOT_BYTES / 4;   // 53: a block is at most 20 + 63 * 26 = 1658 bits

// C[u][x] = c(u) / 2 * cos((2x + 1) u pi / 16), c(0) = 1 / sqrt 2: the orthonormal 8-point DCT-II, rounded from float64
__device__ const float kDct[64] = {
    0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f,
    0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f,
    0.490392625f, 0.415734798f, 0.277785122f, 0.0975451618f,
    -0.0975451618f, -0.277785122f, -0.415734798f, -0.490392625f,
    0.461939752f, 0.191341713f, -0.191341713f, -0.461939752f,
    -0.461939752f, -0.191341713f, 0.191341713f, 0.461939752f,
    0.415734798f, -0.0975451618f, -0.490392625f, -0.277785122f,
    0.277785122f, 0.490392625f, 0.0975451618f, -0.415734798f,
    0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f,
    0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f,
    0.277785122f, -0.490392625f, 0.0975451618f, 0.415734798f,
    -0.415734798f, -0.0975451618f, 0.490392625f, -0.277785122f,
    0.191341713f, -0.461939752f, 0.461939752f, -0.191341713f,
    -0.191341713f, 0.461939752f, -0.461939752f, 0.191341713f,
    0.0975451618f, -0.277785122f, 0.415734798f, -0.490392625f,
    0.490392625f, -0.415734798f, 0.277785122f, -0.0975451618f};

// position in the zigzag scan of the coefficient at natural index 8 u + v
__device__ const unsigned char kZigzagOfNatural[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                                       41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                                       46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// ---- stage 1: colour, DCT, quantise ------------------------------------------------------------------------------------
// One wave per MCU, lane = pixel (r, c) and then coefficient (u, v).  The MCU's 8 rows of 24 bytes are 8-byte aligned (W is a
// multiple of 8): lanes 0..23 fetch them as one uint2 each; the two 1-D passes of the DCT go through LDS.
__global__ __launch_bounds__(JQ_THREADS) void jpeg_quantize_kernel(const unsigned char* __restrict__ frames, const uint16_t* __restrict__ qy,
                                                                   const uint16_t* __restrict__ qc, int16_t* __restrict__ coef, int mcus_w,
                                                                   int mcus_per_frame, int64_t n_mcus, int W) {
  __shared__ uint2 raw[4][24];
  __shared__ float pl[4][3][64];
  __shared__ int16_t zz[4][3][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t mcu = (int64_t)blockIdx.x * 4 + wave;
  const bool live = mcu < n_mcus;                 // uniform per wave; no early return in front of the barriers
  const int r = lane >> 3, c = lane & 7;
  if (live && lane < 24) {
    const int64_t frame = mcu / mcus_per_frame;
    const int m = (int)(mcu - frame * mcus_per_frame);
    const int my = m / mcus_w, mx = m - my * mcus_w;
    const int row = lane / 3, part = lane - row * 3;
    const int64_t px = (frame * (int64_t)(mcus_per_frame / mcus_w) * 8 + my * 8 + row) * W + mx * 8;
    raw[wave][lane] = *reinterpret_cast<const uint2*>(frames + px * 3 + part * 8);
  }
  __syncthreads();
  {
    const unsigned char* b = reinterpret_cast<const unsigned char*>(&raw[wave][0]) + lane * 3;
    const float R = (float)b[0], G = (float)b[1], B = (float)b[2];
    // the +128 of Cb / Cr and the level shift by -128 cancel; Y keeps the shift
    pl[wave][0][lane] = fmaf(0.114f, B, fmaf(0.587f, G, 0.299f * R)) - 128.0f;
    pl[wave][1][lane] = fmaf(0.5f, B, fmaf(-0.331264108f, G, -0.168735892f * R));
    pl[wave][2][lane] = fmaf(-0.081312411f, B, fmaf(-0.418687589f, G, 0.5f * R));
  }
  __syncthreads();
  float t[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {                   // along the row: t[r][v] = sum_x f[r][x] C[v][x], v = c
    float acc = 0.f;
#pragma unroll
    for (int x = 0; x < 8; ++x) acc = fmaf(pl[wave][k][r * 8 + x], kDct[c * 8 + x], acc);
    t[k] = acc;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 3; ++k) pl[wave][k][lane] = t[k];
  __syncthreads();
  const int pos = kZigzagOfNatural[lane];
#pragma unroll
  for (int k = 0; k < 3; ++k) {                   // down the column: F[u][v] = sum_y C[u][y] t[y][v], u = r
    float acc = 0.f;
#pragma unroll
    for (int y = 0; y < 8; ++y) acc = fmaf(kDct[r * 8 + y], pl[wave][k][y * 8 + c], acc);
    const float q = (float)(k == 0 ? qy[lane] : qc[lane]);
    zz[wave][k][pos] = (int16_t)(int)roundf(acc / q);          // IEEE division, half away from zero
  }
  __syncthreads();
  if (live) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&zz[wave][0][0]);      // 3 x 64 i16 = 96 words, contiguous in the output
    uint32_t* dst = reinterpret_cast<uint32_t*>(coef + mcu * 192);
    dst[lane] = src[lane];
    if (lane < 32) dst[64 + lane] = src[64 + lane];
  }
}

// ---- stage 2: entropy coding -------------------------------------------------------------------------------------------
// Annex K.3-K.6 as the standard states them (BITS, HUFFVAL); the code tables are generated from them at compile time by the
// procedure of Annex C.
struct HuffSpec {
  unsigned char bits[16];
  unsigned char vals[162];
  int n;
};
constexpr HuffSpec kDcLuma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr HuffSpec kDcChroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr HuffSpec kAcLuma = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    162};
constexpr HuffSpec kAcChroma = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    162};

// symbol -> (length << 16) | code; 0 for a symbol the table does not hold.  [0]: luminance, [1]: chrominance
struct HuffCodes {
  uint32_t dc[2][16];
  uint32_t ac[2][256];
};
constexpr void huff_fill(const HuffSpec& s, uint32_t* out) {
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < s.bits[len - 1]; ++i) out[s.vals[k++]] = ((uint32_t)len << 16) | code++;
    code <<= 1;
  }
}
constexpr HuffCodes huff_make() {
  HuffCodes h = {};
  huff_fill(kDcLuma, h.dc[0]);
  huff_fill(kDcChroma, h.dc[1]);
  huff_fill(kAcLuma, h.ac[0]);
  huff_fill(kAcChroma, h.ac[1]);
  return h;
}
__device__ const HuffCodes kHuff = huff_make();

// `len` more bits (the low ones of `v`) behind the `n` already in `acc`
__device__ __forceinline__ void put(uint64_t& acc, int& n, uint32_t v, int len) {
  acc = (acc << len) | v;
  n += len;
}
__device__ __forceinline__ void put_code(uint64_t& acc, int& n, uint32_t lc) { put(acc, n, lc & 0xffffu, (int)(lc >> 16)); }

// One wave per block, lane = zigzag index.  A lane holding a non-zero coefficient writes everything the sequential coder
// emits when it reaches that coefficient: the ZRLs of its zero run, its run/size code and its value bits, at most
// 3 * 11 + 16 + 10 = 59 bits; lane 0 writes the DC difference; the lane of the last non-zero coefficient (lane 0 if there is
// none) appends EOB unless it is lane 63.  A wave prefix sum of the lengths places the pieces, integer ORs into LDS join them.
// Values outside the baseline range are clamped (DC difference to +-2047, AC to +-1023) so that no table index and no slot
// can overflow; the quantiser never produces them.
__global__ __launch_bounds__(JP_THREADS) void jpeg_encode_blocks_kernel(const int16_t* __restrict__ coef, uint32_t* __restrict__ slots,
                                                                        uint32_t* __restrict__ bitlen, int blocks_per_frame,
                                                                        int64_t n_blocks) {
  __shared__ uint32_t words[4][56];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t blk = (int64_t)blockIdx.x * 4 + wave;
  const bool live = blk < n_blocks;               // uniform per wave
  if (lane < 56) words[wave][lane] = 0u;
  __syncthreads();
  int total = 0;
  if (live) {
    const int in_frame = (int)(blk % blocks_per_frame);
    const int tab = in_frame % 3 == 0 ? 0 : 1;
    int v = coef[blk * 64 + lane];
    if (lane == 0) {
      if (in_frame >= 3) v -= coef[(blk - 3) * 64];            // the predictor: this component's DC of the MCU before, 0 at a frame's start
      v = max(-2047, min(2047, v));
    } else {
      v = max(-1023, min(1023, v));
    }
    const uint64_t nz = __ballot(lane > 0 && v != 0);
    const int last = nz ? 63 - __builtin_clzll(nz) : 0;
    const int mag = v < 0 ? -v : v;
    const int size = mag ? 32 - __builtin_clz((unsigned)mag) : 0;
    const uint32_t vbits = (uint32_t)(v + (v >> 31)) & ((1u << size) - 1u);     // v, or v - 1 in `size` bits when negative
    uint64_t acc = 0;
    int n = 0;
    if (lane == 0) {
      put_code(acc, n, kHuff.dc[tab][size]);
      put(acc, n, vbits, size);
    } else if (v != 0) {
      const uint64_t below = nz & ((1ull << lane) - 1ull);
      const int prev = below ? 63 - __builtin_clzll(below) : 0;
      const int run = lane - 1 - prev;
      for (int z = run >> 4; z > 0; --z) put_code(acc, n, kHuff.ac[tab][0xF0]);
      put_code(acc, n, kHuff.ac[tab][((run & 15) << 4) | size]);
      put(acc, n, vbits, size);
    }
    if (lane == last && last != 63) put_code(acc, n, kHuff.ac[tab][0x00]);
    int incl = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    total = __shfl(incl, 63, 64);
    if (n > 0) {
      const int pos = incl - n, w = pos >> 5, s = pos & 31;
      const uint64_t left = acc << (64 - n);                   // the piece, MSB first, in the top n bits
      const uint64_t a = left >> s;
      const uint32_t w0 = (uint32_t)(a >> 32), w1 = (uint32_t)a, w2 = s ? (uint32_t)left << (32 - s) : 0u;
      // a non-zero word holds bits below position `total` <= 1658, so its index is below 52
      if (w0) atomicOr(&words[wave][w], w0);
      if (w1) atomicOr(&words[wave][w + 1], w1);
      if (w2) atomicOr(&words[wave][w + 2], w2);
    }
  }
  __syncthreads();
  if (live) {
    if (lane < JP_SLOT_WORDS) slots[blk * JP_SLOT_WORDS + lane] = words[wave][lane];
    if (lane == 0) bitlen[blk] = (uint32_t)total;
  }
}

// One workgroup per frame: exclusive scan of the blocks' bit lengths, the frame's byte count, and zeros over the words the
// stream will occupy (the next kernel ORs into them).  Thread t owns a contiguous run of blocks.
__global__ __launch_bounds__(JP_SCAN_THREADS) void jpeg_scan_kernel(const uint32_t* __restrict__ bitlen, uint32_t* __restrict__ bitoff,
                                                                    int blocks_per_frame, uint32_t* __restrict__ out, int64_t out_stride_words,
                                                                    int32_t* __restrict__ nbytes) {
  __shared__ uint32_t wave_sum_s[JP_SCAN_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t base = (int64_t)blockIdx.x * blocks_per_frame;
  const int per = (blocks_per_frame + JP_SCAN_THREADS - 1) / JP_SCAN_THREADS;
  const int lo = min(tid * per, blocks_per_frame), hi = min(lo + per, blocks_per_frame);
  uint32_t mine = 0;
  for (int i = lo; i < hi; ++i) mine += bitlen[base + i];
  uint32_t incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) wave_sum_s[wave] = incl;
  __syncthreads();
  uint32_t before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < JP_SCAN_THREADS / 64; ++w) {
    const uint32_t s = wave_sum_s[w];
    if (w < wave) before += s;
    total += s;
  }
  uint32_t off = before + incl - mine;
  for (int i = lo; i < hi; ++i) {
    bitoff[base + i] = off;
    off += bitlen[base + i];
  }
  const uint32_t n_words = (total + 31u) >> 5;                  // <= blocks_per_frame * 53 <= out_stride_words
  uint32_t* o = out + (int64_t)blockIdx.x * out_stride_words;
  for (uint32_t i = tid; i < n_words; i += JP_SCAN_THREADS) o[i] = 0u;
  if (tid == 0) nbytes[blockIdx.x] = (int32_t)((total + 7u) >> 3);
}

// One wave per block: its slot, shifted right by the bit offset's low five bits, lands on the stream's words.  A word the
// block covers completely is stored; the first and last word may be shared with neighbouring blocks and are ORed in
// (integer, so the order of arrival cannot change the result).  The last block of a frame adds the 1-bits up to the byte
// boundary.  Words are assembled MSB first and stored byte-swapped, which makes the byte sequence of the stream.
__global__ __launch_bounds__(JP_THREADS) void jpeg_place_blocks_kernel(const uint32_t* __restrict__ slots, const uint32_t* __restrict__ bitlen,
                                                                       const uint32_t* __restrict__ bitoff, int blocks_per_frame,
                                                                       int64_t n_blocks, uint32_t* __restrict__ out, int64_t out_stride_words) {
  const int lane = threadIdx.x & 63;
  const int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blk >= n_blocks) return;                    // uniform per wave, no barrier below
  const int64_t frame = blk / blocks_per_frame;
  const uint32_t off = bitoff[blk], len = bitlen[blk];
  const int s = (int)(off & 31u);
  const uint32_t w0 = off >> 5, end = off + len;
  const int n_words = (int)((s + len + 31u) >> 5);             // <= 53: s + len <= 31 + 1658
  const uint32_t cur = lane < JP_SLOT_WORDS ? slots[blk * JP_SLOT_WORDS + lane] : 0u;
  uint32_t prev = __shfl_up(cur, 1, 64);
  if (lane == 0) prev = 0u;
  uint32_t val = s ? (prev << (32 - s)) | (cur >> s) : cur;
  const bool frame_end = blk - frame * blocks_per_frame == blocks_per_frame - 1;
  if (lane < n_words) {
    const bool first_shared = lane == 0 && s != 0;
    const bool last_shared = lane == n_words - 1 && (end & 31u) != 0u;
    if (frame_end && last_shared) {
      const int used = (int)(end & 31u), pad = (8 - (used & 7)) & 7;
      val |= ((1u << pad) - 1u) << (32 - used - pad);
    }
    uint32_t* dst = out + frame * out_stride_words + w0 + lane;      // w0 + lane < ceil(frame bits / 32), zeroed by jpeg_scan_kernel
    const uint32_t bytes = __builtin_bswap32(val);
    if (first_shared || last_shared) atomicOr(dst, bytes);
    else *dst = bytes;
  }
}

// ---- decoder, stage 1: entropy decoding ----------------------------------------------------------------------------------
// One workgroup owns a frame from the first phase to the last; nothing is handed to another workgroup and nothing spins.
// The scan is cut into subsequences of `S` bits, JD_THREADS of them (a chunk) at a time.  A decoder state is (bit position,
// block inside the MCU, next zigzag index), packed into one word.  Per chunk:
//   A  every lane decodes its subsequence from the assumed state (start, 0, 0) - lane 0 from the state the chunk before ended in,
//      which is final - and records its exit state and the blocks it completed;
//   B  a lane whose predecessor's exit differs from the entry it used decodes again from that exit, until no entry changes.
//      Lane 0 never changes, so lane i is final after at most i rounds: the loop is bounded by the lane count, and at its fixed
//      point every entry IS the predecessor's exit, i.e. the sequential decoder's state - whatever S is and however quickly
//      the streams synchronised;
//   C  an exclusive prefix sum of the block counts, then the one pass that stores: each symbol starts in exactly one
//      subsequence, so exactly one lane writes each coefficient (the frame's coefficients were zeroed first).
// After the last chunk: the pass / fail word, then D, the per-component prefix sum that turns DC differences into DC values.
// Every loop is bounded without trusting the stream: a symbol takes at least one bit and the bit position only grows; a symbol
// that would end behind the scan's last bit is not decoded; block indices are checked before every store.
constexpr int JD_THREADS = 1024;                 // 16 waves: a 4:4:4 frame of 256 x 256 is one chunk (0.66 ms per clip; 1.07 at 256 lanes)
constexpr int JD_TAB = AVSD_JPEG_HUFF_WORDS;      // one table: lut[256], limit[16], offset[16], vals[256 bytes]
constexpr int JD_SET = AVSD_JPEG_HUFF_SET_WORDS;  // [component][DC, AC]

__device__ __forceinline__ uint64_t jd_pack(int p, int b, int k) { return ((uint64_t)(uint32_t)p << 16) | ((uint64_t)b << 8) | (uint64_t)k; }

// The bit reader of one lane: `buf` holds the `avail` bits behind bit position p, MSB first; a word is appended whenever fewer than
// 32 are left, so a symbol (at most 16 + 15 bits) is always whole, and a lane loads each word of its subsequence once per pass.
// Words behind index (nbits >> 5) + 1 are not read (the kernel has checked that the ones up to there are inside the buffer), and
// bits behind the scan's end read as ones, whatever the padding holds.
struct JdBits {
  const uint32_t* __restrict__ words;
  uint64_t buf;
  int avail, next, last;                          // next: index of the word to append; last: the last index that may be read

  __device__ __forceinline__ uint32_t word(int i) const { return i <= last ? __builtin_bswap32(words[i]) : 0xffffffffu; }
  __device__ __forceinline__ void open(const uint32_t* __restrict__ w, int p, int nbits) {
    words = w;
    last = (nbits >> 5) + 1;
    next = p >> 5;
    const uint64_t both = ((uint64_t)word(next) << 32) | word(next + 1);
    next += 2;
    buf = both << (p & 31);
    avail = 64 - (p & 31);
  }
  __device__ __forceinline__ uint32_t peek(int p, int nbits) {
    if (avail < 32) {
      buf |= (uint64_t)word(next++) << (32 - avail);
      avail += 32;
    }
    uint32_t bits = (uint32_t)(buf >> 32);
    const int left = nbits - p;
    if (left < 32) bits |= left <= 0 ? 0xffffffffu : (0xffffffffu >> left);
    return bits;
  }
  __device__ __forceinline__ void skip(int n) {   // n <= 31 <= avail
    buf <<= n;
    avail -= n;
  }
};

// -> the symbol and its code length, or -1 (length 16) for a prefix no code of the table has
__device__ __forceinline__ int jd_symbol(const uint32_t* t, uint32_t bits, int& len) {
  const uint32_t e = t[bits >> 24];
  if (e) {
    len = (int)(e >> 8);
    return (int)(e & 0xffu);
  }
  const uint32_t v = bits >> 16;
  len = 16;
#pragma unroll 1
  for (int l = 9; l <= 16; ++l) {
    if (v < t[256 + l - 1]) {
      len = l;
      const uint32_t idx = ((v >> (16 - l)) + t[272 + l - 1]) & 0xffu;
      return (int)((t[288 + (idx >> 2)] >> ((idx & 3u) * 8u)) & 0xffu);
    }
  }
  return -1;
}

// Decodes the symbols that start in [position of `state`, end).  WRITE: stores them, the block index counted from blk_base, and
// collects the status bits; otherwise only the exit state and the number of completed blocks come out.
template <bool WRITE>
__device__ __forceinline__ uint64_t jd_span(const uint32_t* __restrict__ words, const uint32_t* tabs, int bpm, uint64_t state, int end, int nbits,
                                            int& nblk, int16_t* __restrict__ coef, int blk_base, int blocks_per_frame, int& st) {
  int p = (int)(state >> 16), b = (int)((state >> 8) & 0xffu), k = (int)(state & 0xffu);
  nblk = 0;
  JdBits rd;
  rd.open(words, p, nbits);
  while (p < end) {
    const uint32_t bits = rd.peek(p, nbits);
    const int comp = bpm == 3 ? b : (b < 4 ? 0 : b - 3);
    int len;
    const int sym = jd_symbol(tabs + (comp * 2 + (k ? 1 : 0)) * JD_TAB, bits, len);
    const int size = sym < 0 ? 0 : (sym & 15);
    if (p + len + size > nbits) break;            // would read past the scan's end: not decoded
    if (sym < 0) {
      if (WRITE) st |= AVSD_JPEG_BAD_CODE;
      p += 1;
      rd.skip(1);
      continue;
    }
    const int raw = size ? (int)((bits << len) >> (32 - size)) : 0;
    const int val = size && !(raw >> (size - 1)) ? raw - (1 << size) + 1 : raw;
    p += len + size;
    rd.skip(len + size);
    int at = -1;
    if (k == 0) {
      at = 0;
      k = 1;
    } else if (size == 0) {
      k = (sym >> 4) == 15 ? k + 16 : 64;         // ZRL, or end of block
    } else {
      k += sym >> 4;
      if (k > 63) {
        if (WRITE) st |= AVSD_JPEG_BAD_INDEX;
      } else {
        at = k;
      }
      ++k;
    }
    if (WRITE && at >= 0) {
      const int blk = blk_base + nblk;
      if (blk < blocks_per_frame) coef[(int64_t)blk * 64 + at] = (int16_t)val;
      else st |= AVSD_JPEG_TOO_MANY;
    }
    if (k >= 64) {
      k = 0;
      b = b + 1 == bpm ? 0 : b + 1;
      ++nblk;
    }
  }
  return jd_pack(p, b, k);
}

// exclusive prefix sum of `v` over the workgroup and the total; two barriers
__device__ __forceinline__ int jd_block_scan(int v, int* wave_sums, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  __syncthreads();                                // the sums of the call before have been read
  if (lane == 63) wave_sums[wave] = incl;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < JD_THREADS / 64; ++w) {
    const int s = wave_sums[w];
    if (w < wave) before += s;
    total += s;
  }
  return before + incl - v;
}

__global__ __launch_bounds__(JD_THREADS) void jpeg_decode_scan_kernel(const uint32_t* __restrict__ scan, int64_t scan_bytes,
                                                                      const int64_t* __restrict__ offsets, const int32_t* __restrict__ nbits_of,
                                                                      const int32_t* __restrict__ table_index,
                                                                      const uint32_t* __restrict__ tables, int n_tables, int blocks_per_frame,
                                                                      int bpm, int S, int16_t* __restrict__ coef_all,
                                                                      int32_t* __restrict__ status, int32_t* __restrict__ rounds) {
  __shared__ uint32_t tabs[JD_SET];
  __shared__ uint64_t exit_s[JD_THREADS];
  __shared__ int wave_sums[JD_THREADS / 64];
  __shared__ int dc_sums[3][JD_THREADS / 64];
  __shared__ int st_s;
  const int tid = threadIdx.x, frame = blockIdx.x;
  int16_t* coef = coef_all + (int64_t)frame * blocks_per_frame * 64;
  const int64_t off = offsets[frame];
  const int nbits = nbits_of[frame], ti = table_index[frame];
  // the words a decode may touch: up to the one behind the word of the last bit; all of them inside the buffer, or nothing runs
  const bool ok = off >= 0 && (off & 3) == 0 && nbits >= 0 && nbits <= AVSD_JPEG_MAX_SCAN_BITS && off + ((int64_t)(nbits >> 5) + 2) * 4 <= scan_bytes &&
                  ti >= 0 && ti < n_tables;
  {
    uint4* z = reinterpret_cast<uint4*>(coef);    // blocks_per_frame * 128 bytes, 16-byte aligned (checked by the entry point)
    for (int i = tid; i < blocks_per_frame * 8; i += JD_THREADS) z[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  if (tid == 0) st_s = 0;
  if (!ok) {                                      // uniform over the workgroup
    if (tid == 0) {
      status[frame] = AVSD_JPEG_BAD_ARGS;
      if (rounds) rounds[frame] = 0;
    }
    return;
  }
  for (int i = tid; i < JD_SET; i += JD_THREADS) tabs[i] = tables[(int64_t)ti * JD_SET + i];
  __syncthreads();
  const uint32_t* words = scan + (off >> 2);
  const int nsub = (int)(((int64_t)nbits + S - 1) / S);
  uint64_t carry = 0;                             // (0, 0, 0)
  int carry_blocks = 0, max_rounds = 0, st = 0;
  for (int c0 = 0; c0 < nsub; c0 += JD_THREADS) {
    const int j = c0 + tid;
    const bool live = j < nsub;
    const int start = live ? j * S : 0;           // j * S < nbits < 2^31
    const int end = live ? (int)min((int64_t)start + S, (int64_t)nbits) : 0;
    uint64_t entry = tid == 0 ? carry : jd_pack(start, 0, 0);
    int nblk = 0, unused = 0;
    uint64_t out = entry;
    if (live) out = jd_span<false>(words, tabs, bpm, entry, end, nbits, nblk, nullptr, 0, 0, unused);       // phase A
    exit_s[tid] = out;
    __syncthreads();
    int r = 0;
    for (; r < JD_THREADS; ++r) {                 // phase B
      uint64_t pred = entry;
      if (live && tid > 0) pred = exit_s[tid - 1];
      const bool redo = pred != entry;
      if (!__syncthreads_or(redo)) break;         // also: every lane has read its predecessor before any lane writes
      if (redo) {
        entry = pred;
        out = jd_span<false>(words, tabs, bpm, entry, end, nbits, nblk, nullptr, 0, 0, unused);
        exit_s[tid] = out;
      }
      __syncthreads();
    }
    max_rounds = max(max_rounds, r);
    int total;
    const int base = carry_blocks + jd_block_scan(live ? nblk : 0, wave_sums, total);                       // phase C
    if (live) jd_span<true>(words, tabs, bpm, entry, end, nbits, nblk, coef, base, blocks_per_frame, st);
    carry = exit_s[min(nsub - c0, JD_THREADS) - 1];
    carry_blocks += total;                        // <= nbits
    __syncthreads();                              // exit_s is rewritten by the next chunk
  }
  if (st) atomicOr(&st_s, st);
  __syncthreads();                                // also makes this workgroup's coefficient stores visible to all its lanes
  if (tid == 0) {
    int s = st_s;
    const int p = (int)(carry >> 16), left = nbits - p;
    if (carry_blocks != blocks_per_frame || (carry & 0xffffu) != 0) s |= AVSD_JPEG_INCOMPLETE;
    // the reader gives ones behind the end, so the bits that are left must make the top byte all ones
    JdBits rd;
    rd.open(words, p, nbits);
    if (left >= 8 || (rd.peek(p, nbits) >> 24) != 0xffu) s |= AVSD_JPEG_BAD_TAIL;
    status[frame] = s;
    if (rounds) rounds[frame] = max_rounds;
  }
  // phase D: thread t owns a contiguous run of MCUs; sums of its DC differences per component, scanned over the workgroup
  const int n_mcu = blocks_per_frame / bpm;
  const int per = (n_mcu + JD_THREADS - 1) / JD_THREADS;
  const int lo = min(tid * per, n_mcu), hi = min(lo + per, n_mcu);
  int s0 = 0, s1 = 0, s2 = 0;                     // scalars, not an array: a component index would put it into scratch
  for (int m = lo; m < hi; ++m)
    for (int b = 0; b < bpm; ++b) {
      const int c = bpm == 3 ? b : (b < 4 ? 0 : b - 3), d = coef[((int64_t)m * bpm + b) * 64];
      s0 += c == 0 ? d : 0, s1 += c == 1 ? d : 0, s2 += c == 2 ? d : 0;
    }
  int total;
  int p0 = jd_block_scan(s0, dc_sums[0], total), p1 = jd_block_scan(s1, dc_sums[1], total), p2 = jd_block_scan(s2, dc_sums[2], total);
  for (int m = lo; m < hi; ++m)
    for (int b = 0; b < bpm; ++b) {
      const int c = bpm == 3 ? b : (b < 4 ? 0 : b - 3);
      int16_t* dc = coef + ((int64_t)m * bpm + b) * 64;
      const int d = *dc;
      p0 += c == 0 ? d : 0, p1 += c == 1 ? d : 0, p2 += c == 2 ? d : 0;
      *dc = (int16_t)(c == 0 ? p0 : c == 1 ? p1 : p2);
    }
}

// ---- decoder, stage 2: dequantise, inverse DCT, upsample, colour ---------------------------------------------------------
// jidctint.c ("islow": 13-bit constants, 2 extra bits after the first pass).  libjpeg-turbo runs this arithmetic in 16-bit
// vector lanes: the inputs of a pass, i0 +- i4, z3 and z4 wrap to int16 and the results of a pass saturate to int16.  These are
// no-ops for any stream made from pixels; they are kept so that streams built from extreme coefficients decode to the same bytes.
__device__ __forceinline__ int jd_wrap16(int x) { return (int)(int16_t)x; }
__device__ __forceinline__ int jd_sat16(int x) { return max(-32768, min(32767, x)); }
template <int SHIFT>
__device__ __forceinline__ void jd_idct8(const int (&i)[8], int (&o)[8]) {
  int z1 = (i[2] + i[6]) * 4433;
  const int t2 = z1 - i[6] * 15137, t3 = z1 + i[2] * 6270;
  const int t0 = jd_wrap16(i[0] + i[4]) * 8192, t1 = jd_wrap16(i[0] - i[4]) * 8192;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int a0 = i[7], a1 = i[5], a2 = i[3], a3 = i[1];
  z1 = a0 + a3;
  int z2 = a1 + a2, z3 = jd_wrap16(a0 + a2), z4 = jd_wrap16(a1 + a3);
  const int z5 = (z3 + z4) * 9633;
  a0 *= 2446, a1 *= 16819, a2 *= 25172, a3 *= 12299;
  z1 *= -7373, z2 *= -20995;
  z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
  a0 += z1 + z3, a1 += z2 + z4, a2 += z2 + z3, a3 += z1 + z4;
  const int r = 1 << (SHIFT - 1);
  o[0] = jd_sat16((t10 + a3 + r) >> SHIFT), o[7] = jd_sat16((t10 - a3 + r) >> SHIFT);
  o[1] = jd_sat16((t11 + a2 + r) >> SHIFT), o[6] = jd_sat16((t11 - a2 + r) >> SHIFT);
  o[2] = jd_sat16((t12 + a1 + r) >> SHIFT), o[5] = jd_sat16((t12 - a1 + r) >> SHIFT);
  o[3] = jd_sat16((t13 + a0 + r) >> SHIFT), o[4] = jd_sat16((t13 - a0 + r) >> SHIFT);
}

constexpr int JI_THREADS = 256;                   // 32 blocks of coefficients, eight lanes each
__device__ const unsigned char kNaturalOfZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Eight lanes per block.  Lane (block, c): loads zigzag positions 8c .. 8c + 7 and stores their products with the table at
// their natural places; then does column c; then row c, and stores its eight samples into the component's plane.  Planes of a
// frame: Y [mcus_h * 8 v][mcus_w * 8 v], then Cb and Cr [mcus_h * 8][mcus_w * 8], v = 2 for 4:2:0: whole MCUs, so every row of
// eight samples is 8-byte aligned.
__global__ __launch_bounds__(JI_THREADS) void jpeg_idct_kernel(const int16_t* __restrict__ coef, const uint16_t* __restrict__ qtabs, int n_qsets,
                                                               const int32_t* __restrict__ q_index, int blocks_per_frame, int bpm, int mcus_w,
                                                               int mcus_h, int64_t n_blocks, unsigned char* __restrict__ planes) {
  __shared__ int ws[32][72];                      // 72: in the column pass the 32 lanes of a half-wave fall on 32 banks
  const int tid = threadIdx.x, bl = tid >> 3, c = tid & 7;
  const int64_t blk = (int64_t)blockIdx.x * 32 + bl;
  const bool live = blk < n_blocks;               // uniform over the eight lanes of a block
  int frame = 0, in_frame = 0, comp = 0;
  if (live) {
    frame = (int)(blk / blocks_per_frame);
    in_frame = (int)(blk - (int64_t)frame * blocks_per_frame);
    const int b = in_frame % bpm;
    comp = bpm == 3 ? b : (b < 4 ? 0 : b - 3);
    int qi = q_index[frame];
    if (qi < 0 || qi >= n_qsets) qi = 0;          // never from video_io; keeps the read inside the table
    const uint4 raw = *reinterpret_cast<const uint4*>(coef + blk * 64 + c * 8);
    const uint16_t* q = qtabs + ((int64_t)qi * 3 + comp) * 64 + c * 8;
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int v = (int)(int16_t)(w[e >> 1] >> ((e & 1) * 16));
      ws[bl][kNaturalOfZigzag[c * 8 + e]] = jd_wrap16(v * (int)q[e]);
    }
  }
  __syncthreads();
  int in[8], out[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) in[r] = live ? ws[bl][r * 8 + c] : 0;
  // the vector code's shortcut: a block whose rows 1..7 are all zero becomes row 0 << 2 in 16 bits - the value of the full
  // pass, except that it wraps where the full pass saturates
  const bool col_flat = (in[1] | in[2] | in[3] | in[4] | in[5] | in[6] | in[7]) == 0;
  const uint64_t flat = __ballot(col_flat);
  const bool blk_flat = ((flat >> ((tid & 63) & ~7)) & 0xffull) == 0xffull;
  if (blk_flat) {
#pragma unroll
    for (int r = 0; r < 8; ++r) out[r] = jd_wrap16(in[0] * 4);
  } else {
    jd_idct8<11>(in, out);
  }
  if (live) {
#pragma unroll
    for (int r = 0; r < 8; ++r) ws[bl][r * 8 + c] = out[r];          // own column only
  }
  __syncthreads();
  if (!live) return;
#pragma unroll
  for (int x = 0; x < 8; ++x) in[x] = ws[bl][c * 8 + x];
  jd_idct8<18>(in, out);
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    lo |= (uint32_t)max(0, min(255, out[x] + 128)) << (8 * x);
    hi |= (uint32_t)max(0, min(255, out[x + 4] + 128)) << (8 * x);
  }
  const int v = bpm == 3 ? 1 : 2;
  const int mcu = in_frame / bpm, b = in_frame - mcu * bpm;
  const int my = mcu / mcus_w, mx = mcu - my * mcus_w;
  const int64_t c_plane = (int64_t)mcus_h * mcus_w * 64, y_plane = c_plane * v * v;
  unsigned char* base = planes + (int64_t)frame * (y_plane + 2 * c_plane);
  int by = my, bx = mx, pw = mcus_w * 8;
  if (comp == 0) {
    pw *= v;
    if (v == 2) by = 2 * my + (b >> 1), bx = 2 * mx + (b & 1);
  } else {
    base += y_plane + (comp - 1) * c_plane;
  }
  *reinterpret_cast<uint2*>(base + ((int64_t)by * 8 + c) * pw + bx * 8) = make_uint2(lo, hi);
}

// One lane per pixel.  4:2:0 chroma: libjpeg's "fancy" triangle filter over the ceil(H/2) x ceil(W/2) real samples, the edge
// rows and columns repeated; then jdcolor.c's 16-bit fixed-point YCbCr -> RGB.
__device__ __forceinline__ int jd_fancy(const unsigned char* __restrict__ p, int pw, int ch, int cw, int y, int x) {
  const int r = y >> 1, j = x >> 1;
  const int rn = (y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);
  const int jn = (x & 1) ? min(j + 1, cw - 1) : max(j - 1, 0);
  const int v = 3 * (int)p[(int64_t)r * pw + j] + (int)p[(int64_t)rn * pw + j];
  const int vn = 3 * (int)p[(int64_t)r * pw + jn] + (int)p[(int64_t)rn * pw + jn];
  return (3 * v + vn + ((x & 1) ? 7 : 8)) >> 4;
}

__global__ __launch_bounds__(256) void jpeg_colour_kernel(const unsigned char* __restrict__ planes, int H, int W, int v, int mcus_w, int mcus_h,
                                                          int64_t n_pixels, unsigned char* __restrict__ frames) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pixels) return;
  const int64_t hw = (int64_t)H * W;
  const int64_t frame = i / hw;
  const int in_frame = (int)(i - frame * hw);     // H, W <= 65535 and H * W < 2^31 (checked by the entry point)
  const int y = in_frame / W, x = in_frame - y * W;
  const int64_t c_plane = (int64_t)mcus_h * mcus_w * 64, y_plane = c_plane * v * v;
  const unsigned char* base = planes + frame * (y_plane + 2 * c_plane);
  const int cpw = mcus_w * 8;
  const int Y = base[(int64_t)y * (cpw * v) + x];
  int cb, cr;
  if (v == 1) {
    cb = base[y_plane + (int64_t)y * cpw + x];
    cr = base[y_plane + c_plane + (int64_t)y * cpw + x];
  } else {
    const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;
    cb = jd_fancy(base + y_plane, cpw, ch, cw, y, x);
    cr = jd_fancy(base + y_plane + c_plane, cpw, ch, cw, y, x);
  }
  cb -= 128, cr -= 128;
  unsigned char* o = frames + i * 3;
  o[0] = (unsigned char)max(0, min(255, Y + ((91881 * cr + 32768) >> 16)));
  o[1] = (unsigned char)max(0, min(255, Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)));
  o[2] = (unsigned char)max(0, min(255, Y + ((116130 * cb + 32768) >> 16)));
}

}  // namespace

extern "C" int avsd_jpeg_quantize_u8(const void* frames_u8, int n, int H, int W, const uint16_t* qy, const uint16_t* qc, int16_t* coef,
                                     void* stream) {
  AVSD_REQUIRE(frames_u8 && qy && qc && coef, "jpeg_quantize: null pointer");
  AVSD_REQUIRE(n > 0 && H > 0 && W > 0, "jpeg_quantize: bad sizes (n %d, H %d, W %d)", n, H, W);
  AVSD_REQUIRE(H % 8 == 0 && W % 8 == 0, "jpeg_quantize: H (%d) and W (%d) must be multiples of 8 (4:4:4, whole MCUs only)", H, W);
  AVSD_REQUIRE(H <= 65535 && W <= 65535, "jpeg_quantize: a JPEG frame is at most 65535 x 65535, got %d x %d", H, W);
  AVSD_REQUIRE((uintptr_t)frames_u8 % 8 == 0 && (uintptr_t)coef % 4 == 0, "jpeg_quantize: frames need 8-byte, coefficients 4-byte alignment");
  const int mcus_w = W / 8, mcus = (H / 8) * mcus_w;
  const int64_t n_mcus = (int64_t)n * mcus;
  const int64_t grid = (n_mcus + 3) / 4;
  AVSD_REQUIRE(grid <= 0x7fffffffLL, "jpeg_quantize: %d frames of %d MCUs exceed the grid", n, mcus);
  hipLaunchKernelGGL(jpeg_quantize_kernel, dim3((unsigned)grid), dim3(JQ_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     static_cast<const unsigned char*>(frames_u8), qy, qc, coef, mcus_w, mcus, n_mcus, W);
  AVSD_CHECK_LAUNCH("jpeg_quantize launch");
  return AVSD_OK;
}

extern "C" int avsd_jpeg_pack_i16(const int16_t* coef, int n, int blocks_per_frame, void* scratch, int64_t scratch_bytes, void* out_u8,
                                  int64_t out_stride, int32_t* nbytes, void* stream) {
  AVSD_REQUIRE(coef && scratch && out_u8 && nbytes, "jpeg_pack: null pointer");
  AVSD_REQUIRE(n > 0 && blocks_per_frame > 0 && blocks_per_frame % 3 == 0,
               "jpeg_pack: blocks_per_frame (%d) must be 3 x the number of MCUs, n (%d) positive", blocks_per_frame, n);
  // bit offsets inside a frame are 32-bit, and a 65535 x 65535 frame is out of reach long before
  AVSD_REQUIRE(blocks_per_frame <= (1 << 20), "jpeg_pack: %d blocks per frame exceed 2^20 (a 4:4:4 frame of 22 megapixels)", blocks_per_frame);
  const int64_t n_blocks = (int64_t)n * blocks_per_frame;
  const int64_t need = n_blocks * (AVSD_JPEG_SLOT_BYTES + 8);    // a slot, a bit length and a bit offset per block
  AVSD_REQUIRE(scratch_bytes >= need, "jpeg_pack: scratch of %lld bytes, need %lld (%d bytes per block)", (long long)scratch_bytes,
               (long long)need, AVSD_JPEG_SLOT_BYTES + 8);
  AVSD_REQUIRE(out_stride % 4 == 0 && out_stride >= (int64_t)blocks_per_frame * AVSD_JPEG_SLOT_BYTES,
               "jpeg_pack: out_stride (%lld) must be a multiple of 4 and at least %d bytes per block (%lld)", (long long)out_stride,
               AVSD_JPEG_SLOT_BYTES, (long long)blocks_per_frame * AVSD_JPEG_SLOT_BYTES);
  AVSD_REQUIRE((uintptr_t)scratch % 4 == 0 && (uintptr_t)out_u8 % 4 == 0, "jpeg_pack: scratch and out need 4-byte alignment");
  const int64_t grid = (n_blocks + 3) / 4;
  AVSD_REQUIRE(grid <= 0x7fffffffLL, "jpeg_pack: %d frames of %d blocks exceed the grid", n, blocks_per_frame);
  uint32_t* slots = static_cast<uint32_t*>(scratch);
  uint32_t* bitlen = slots + n_blocks * JP_SLOT_WORDS;
  uint32_t* bitoff = bitlen + n_blocks;
  uint32_t* out = static_cast<uint32_t*>(out_u8);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(jpeg_encode_blocks_kernel, dim3((unsigned)grid), dim3(JP_THREADS), 0, s, coef, slots, bitlen, blocks_per_frame, n_blocks);
  AVSD_CHECK_LAUNCH("jpeg_pack encode launch");
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3((unsigned)n), dim3(JP_SCAN_THREADS), 0, s, bitlen, bitoff, blocks_per_frame, out, out_stride / 4,
                     nbytes);
  AVSD_CHECK_LAUNCH("jpeg_pack scan launch");
  hipLaunchKernelGGL(jpeg_place_blocks_kernel, dim3((unsigned)grid), dim3(JP_THREADS), 0, s, slots, bitlen, bitoff, blocks_per_frame, n_blocks,
                     out, out_stride / 4);
  AVSD_CHECK_LAUNCH("jpeg_pack place launch");
  return AVSD_OK;
}

extern "C" int avsd_jpeg_decode_scan(const void* scan, int64_t scan_bytes, const int64_t* offsets, const int32_t* nbits, const int32_t* table_index,
                                     const uint32_t* tables, int n_tables, int n, int blocks_per_frame, int sampling, int subseq_bits,
                                     int16_t* coef, int32_t* status, int32_t* rounds, void* stream) {
  AVSD_REQUIRE(scan && offsets && nbits && table_index && tables && coef && status, "jpeg_decode_scan: null pointer");
  AVSD_REQUIRE(sampling == AVSD_JPEG_444 || sampling == AVSD_JPEG_420, "jpeg_decode_scan: sampling %d is neither AVSD_JPEG_444 nor AVSD_JPEG_420",
               sampling);
  const int bpm = sampling == AVSD_JPEG_444 ? 3 : 6;
  AVSD_REQUIRE(n > 0 && n_tables > 0 && blocks_per_frame > 0 && blocks_per_frame % bpm == 0,
               "jpeg_decode_scan: n (%d) and n_tables (%d) must be positive, blocks_per_frame (%d) a multiple of the %d blocks of an MCU", n,
               n_tables, blocks_per_frame, bpm);
  AVSD_REQUIRE(blocks_per_frame <= (1 << 22), "jpeg_decode_scan: %d blocks per frame exceed 2^22", blocks_per_frame);
  AVSD_REQUIRE(subseq_bits >= 128 && subseq_bits <= 4096 && (subseq_bits & (subseq_bits - 1)) == 0,
               "jpeg_decode_scan: subseq_bits (%d) must be a power of two in 128..4096", subseq_bits);
  AVSD_REQUIRE(scan_bytes >= 8 && scan_bytes % 4 == 0, "jpeg_decode_scan: scan_bytes (%lld) must be a multiple of 4, at least 8", (long long)scan_bytes);
  AVSD_REQUIRE((uintptr_t)scan % 4 == 0 && (uintptr_t)coef % 16 == 0 && (uintptr_t)tables % 4 == 0,
               "jpeg_decode_scan: scan and tables need 4-byte, coefficients 16-byte alignment");
  hipLaunchKernelGGL(jpeg_decode_scan_kernel, dim3((unsigned)n), dim3(JD_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     static_cast<const uint32_t*>(scan), scan_bytes, offsets, nbits, table_index, tables, n_tables, blocks_per_frame, bpm, subseq_bits,
                     coef, status, rounds);
  AVSD_CHECK_LAUNCH("jpeg_decode_scan launch");
  return AVSD_OK;
}

extern "C" int avsd_jpeg_idct_rgb_u8(const int16_t* coef, int n, int H, int W, int sampling, const uint16_t* qtabs, int n_qsets,
                                     const int32_t* q_index, void* planes, int64_t planes_bytes, void* frames_u8, void* stream) {
  AVSD_REQUIRE(coef && qtabs && q_index && planes && frames_u8, "jpeg_idct_rgb: null pointer");
  AVSD_REQUIRE(sampling == AVSD_JPEG_444 || sampling == AVSD_JPEG_420, "jpeg_idct_rgb: sampling %d is neither AVSD_JPEG_444 nor AVSD_JPEG_420", sampling);
  AVSD_REQUIRE(n > 0 && n_qsets > 0 && H > 0 && W > 0 && H <= 65535 && W <= 65535 && (int64_t)H * W < (1ll << 31),
               "jpeg_idct_rgb: bad sizes (n %d, n_qsets %d, H %d, W %d)", n, n_qsets, H, W);
  const int v = sampling == AVSD_JPEG_444 ? 1 : 2, bpm = v == 1 ? 3 : 6;
  const int mcus_w = (W + 8 * v - 1) / (8 * v), mcus_h = (H + 8 * v - 1) / (8 * v);
  const int64_t blocks_per_frame = (int64_t)mcus_w * mcus_h * bpm;
  AVSD_REQUIRE(blocks_per_frame <= (1 << 22), "jpeg_idct_rgb: %lld blocks per frame exceed 2^22", (long long)blocks_per_frame);
  const int64_t need = (int64_t)n * mcus_w * mcus_h * 64 * (v * v + 2);
  AVSD_REQUIRE(planes_bytes >= need, "jpeg_idct_rgb: planes of %lld bytes, need %lld", (long long)planes_bytes, (long long)need);
  AVSD_REQUIRE((uintptr_t)coef % 16 == 0 && (uintptr_t)planes % 8 == 0, "jpeg_idct_rgb: coefficients need 16-byte, planes 8-byte alignment");
  const int64_t n_blocks = (int64_t)n * blocks_per_frame, n_pixels = (int64_t)n * H * W;
  const int64_t grid1 = (n_blocks + 31) / 32, grid2 = (n_pixels + 255) / 256;
  AVSD_REQUIRE(grid1 <= 0x7fffffffLL && grid2 <= 0x7fffffffLL, "jpeg_idct_rgb: %d frames of %d x %d exceed the grid", n, H, W);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)grid1), dim3(JI_THREADS), 0, s, coef, qtabs, n_qsets, q_index, (int)blocks_per_frame, bpm,
                     mcus_w, mcus_h, n_blocks, static_cast<unsigned char*>(planes));
  AVSD_CHECK_LAUNCH("jpeg_idct_rgb idct launch");
  hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)grid2), dim3(256), 0, s, static_cast<const unsigned char*>(planes), H, W, v, mcus_w, mcus_h,
                     n_pixels, static_cast<unsigned char*>(frames_u8));
  AVSD_CHECK_LAUNCH("jpeg_idct_rgb colour launch");
  return AVSD_OK;
}
