// Counter-based normal generator (include/avsd.h, "random numbers"): Philox4x32-10 as published by Random123 (Salmon et al.,
// "Parallel random numbers: as easy as 1, 2, 3", SC'11) and Box-Muller on top of it.  Every normal is a pure function of
// (seed, stream, step, element index): no state and no memory, so a kernel evaluates the ones it needs in registers and any
// partition of a range gives the same bits.
//
//   key      = (seed lo, seed hi)
//   counter  = (block lo, block hi, step, stream),  block = element index >> 2 (64-bit)
//   element  = lane (element index & 3) of its block
//
// tests/philox_ref.py restates the same construction in numpy (integers exactly, the normals in float64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace philox {

struct Key {
  uint32_t k0, k1, stream, step;
};

__host__ __device__ inline Key make_key(uint64_t seed, uint32_t stream, uint32_t step) {
  return Key{(uint32_t)seed, (uint32_t)(seed >> 32), stream, step};
}

// the four words of block `block`
__host__ __device__ inline void words4(const Key& key, uint64_t block, uint32_t w[4]) {
  uint32_t c0 = (uint32_t)block, c1 = (uint32_t)(block >> 32), c2 = key.step, c3 = key.stream;
  uint32_t k0 = key.k0, k1 = key.k1;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;      // Weyl sequence of the key
    k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

#if defined(__HIPCC__)
// One Box-Muller pair from two words.  Both uniforms are exact in f32: u = ((wu >> 9) + 0.5) 2^-23 lies in (0, 1), so that
// |z| <= sqrt(-2 log 2^-24) < 5.77, and v = (wv >> 8) 2^-24 lies in [0, 1).  logf / sqrtf / sincospif are the accurate ones
// (the library is built without fast-math).
__device__ __forceinline__ void box_muller(uint32_t wu, uint32_t wv, float& z_cos, float& z_sin) {
  const float u = ((float)(wu >> 9) + 0.5f) * 1.1920928955078125e-07f;    // 2^-23
  const float v = (float)(wv >> 8) * 5.9604644775390625e-08f;             // 2^-24
  const float r = sqrtf(-2.0f * logf(u));
  float s, c;
  sincospif(2.0f * v, &s, &c);
  z_cos = r * c;
  z_sin = r * s;
}

// the four normals of block `block`: lanes 0, 1 from words 0, 1 and lanes 2, 3 from words 2, 3
__device__ __forceinline__ void normal4(const Key& key, uint64_t block, float z[4]) {
  uint32_t w[4];
  words4(key, block, w);
  box_muller(w[0], w[1], z[0], z[1]);
  box_muller(w[2], w[3], z[2], z[3]);
}
#endif

}  // namespace philox
