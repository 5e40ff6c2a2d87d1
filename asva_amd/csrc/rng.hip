// Random numbers on the device (include/avsd.h, "random numbers"): the raw Philox4x32-10 words and the normal sequence built on
// them (csrc/philox.h), written out: the normals for a clip's initial latents, the words for the tests that pin the generator.
#include "avsd_common.h"
#include "philox.h"

namespace {

inline unsigned rng_grid(int64_t nblocks) {
  int64_t g = (nblocks + 255) / 256;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (unsigned)g;
}

// One thread per Philox block: block b holds items 4b .. 4b+3 of the sequence, out[j - first] receives item j for
// first <= j < first + n.  The first and the last block of a range may be partial; a full block whose destination is
// 16-byte aligned is stored as one vector.  NORMAL: f32 normals, otherwise the raw words.
template <bool NORMAL>
__global__ __launch_bounds__(256) void philox_fill_kernel(uint32_t* out, int64_t n, int64_t first, philox::Key key, bool aligned) {
  const int64_t b0 = first >> 2;
  const int64_t nb = ((first + n - 1) >> 2) - b0 + 1;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < nb; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = b0 + t;
    uint32_t w[4];
    if (NORMAL) {
      float z[4];
      philox::normal4(key, (uint64_t)b, z);
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = __float_as_uint(z[e]);
    } else {
      philox::words4(key, (uint64_t)b, w);
    }
    const int64_t o = b * 4 - first;             // destination of lane 0: in [-3, n)
    if (aligned && o >= 0 && o + 4 <= n) {
      *reinterpret_cast<uint4*>(out + o) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (o + e >= 0 && o + e < n) out[o + e] = w[e];
    }
  }
}

template <bool NORMAL>
int philox_fill(const char* who, void* out, int64_t n, uint64_t seed, uint32_t stream, uint32_t step, int64_t first, void* hip_stream) {
  AVSD_REQUIRE(n >= 0 && first >= 0 && first <= INT64_MAX - n, "%s: need n >= 0 and first >= 0 (n=%lld first=%lld)", who, (long long)n,
               (long long)first);
  if (n == 0) return AVSD_OK;
  AVSD_REQUIRE(out != nullptr && (uintptr_t)out % 4 == 0, "%s: null or misaligned pointer", who);
  // vector stores need out + (4b - first) on a 16-byte boundary for every block b
  const bool aligned = ((uintptr_t)out % 16 == 0) && (first % 4 == 0);
  const int64_t nb = ((first + n - 1) >> 2) - (first >> 2) + 1;
  hipLaunchKernelGGL(philox_fill_kernel<NORMAL>, dim3(rng_grid(nb)), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream),
                     (uint32_t*)out, n, first, philox::make_key(seed, stream, step), aligned);
  AVSD_CHECK_LAUNCH(who);
  return AVSD_OK;
}

}  // namespace

extern "C" int avsd_philox4x32_u32(uint32_t* out, int64_t n_words, uint64_t seed, uint32_t stream, uint32_t step, int64_t first_word,
                                   void* hip_stream) {
  return philox_fill<false>("philox4x32_u32", out, n_words, seed, stream, step, first_word, hip_stream);
}

extern "C" int avsd_randn_philox_f32(float* out, int64_t n, uint64_t seed, uint32_t stream, uint32_t step, int64_t first,
                                     void* hip_stream) {
  return philox_fill<true>("randn_philox_f32", out, n, seed, stream, step, first, hip_stream);
}
