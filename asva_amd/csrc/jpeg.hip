// Baseline JPEG encoder for the Motion-JPEG clip writer (asva_amd/video_io.py:encode_jpeg_frames): 8-bit, three components,
// 4:4:4, one MCU = one Y, one Cb and one Cr block, raster order, no restart markers, the Annex K Huffman tables.  Two stages,
// exported separately (include/avsd.h):
//   avsd_jpeg_quantize_u8   frames u8 -> JFIF YCbCr -> level shift -> 8 x 8 DCT-II in f32 -> quantise -> zigzag, i16
//   avsd_jpeg_pack_i16      coefficients -> one entropy-coded stream per frame (unstuffed, last byte padded with 1-bits)
// f32 and integer arithmetic only: the same instructions in both builds of the library, so the same bytes.  Headers, FF
// byte stuffing and the container are the host's.
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
