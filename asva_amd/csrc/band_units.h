// Shared by the band kernels (ffblock.hip, tblock.hip): the finish of one 32 x 32 output unit.
#pragma once
#include "avsd_common.h"

// v = acc + bias[n] + R[row][n] for one 32 x 32 unit, rounded to 16 bits: the shared epilogue's terms in its order and its wide form
// (the lanes l / l ^ 32 of a row trade halves, so each reads and writes 32 contiguous bytes: columns 16 (l >> 5) .. + 15 of the unit).
// res -> this lane's 16 residual values; the packed result comes back in lo (columns .. + 7) and hi.
__device__ __forceinline__ void unit_finish(const f32x16& a, const float* bias, int hsel, const uint4& rlo, const uint4& rhi, uint4& lo, uint4& hi) {
  float v[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 bb = *reinterpret_cast<const float4*>(bias + 8 * q + hsel);
    v[4 * q] = a[4 * q] + bb.x; v[4 * q + 1] = a[4 * q + 1] + bb.y; v[4 * q + 2] = a[4 * q + 2] + bb.z; v[4 * q + 3] = a[4 * q + 3] + bb.w;
  }
  const unsigned s0[2] = {rlo.x, rlo.y}, s1[2] = {rlo.z, rlo.w}, s2[2] = {rhi.x, rhi.y}, s3[2] = {rhi.z, rhi.w};
  unsigned x[2][2], y[2][2];
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const auto e = __builtin_amdgcn_permlane32_swap(s0[d], s1[d], false, false);   // -> quads 0 and 2
    const auto o = __builtin_amdgcn_permlane32_swap(s2[d], s3[d], false, false);   // -> quads 1 and 3
    v[0 + 2 * d] += lo2f(e[0]); v[1 + 2 * d] += hi2f(e[0]);
    v[8 + 2 * d] += lo2f(e[1]); v[9 + 2 * d] += hi2f(e[1]);
    v[4 + 2 * d] += lo2f(o[0]); v[5 + 2 * d] += hi2f(o[0]);
    v[12 + 2 * d] += lo2f(o[1]); v[13 + 2 * d] += hi2f(o[1]);
  }
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const auto e = __builtin_amdgcn_permlane32_swap(pack2h(v[0 + 2 * d], v[1 + 2 * d]), pack2h(v[8 + 2 * d], v[9 + 2 * d]), false, false);
    const auto o = __builtin_amdgcn_permlane32_swap(pack2h(v[4 + 2 * d], v[5 + 2 * d]), pack2h(v[12 + 2 * d], v[13 + 2 * d]), false, false);
    x[0][d] = e[0]; x[1][d] = e[1];
    y[0][d] = o[0]; y[1][d] = o[1];
  }
  lo = make_uint4(x[0][0], x[0][1], x[1][0], x[1][1]);
  hi = make_uint4(y[0][0], y[0][1], y[1][0], y[1][1]);
}
