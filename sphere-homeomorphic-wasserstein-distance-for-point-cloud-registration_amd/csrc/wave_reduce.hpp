// wave_reduce.hpp -- sums over the 64 lanes of a wave of many per-lane values at once, shared by the units whose backward
// kernels reduce per-point parameter gradients without atomics (shw_flow.hip, shw_sphere_map.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace shw {

// N (a power of two, at most 64) per-lane values -> lane L returns the sum over the wave of v[L & (N - 1)].  Step s halves
// the values: a lane whose bit s is clear keeps the even one of a pair and hands the odd one to its partner, and the other
// way round; after log2 N steps one value is left and the remaining lane bits are folded by plain exchanges.
template <int N>
__device__ __forceinline__ float transpose_reduce(float (&v)[N], int lane) {
  int s = 0;
#pragma unroll
  for (int n = N; n > 1; n >>= 1, ++s) {
    const bool odd = (lane >> s) & 1;
#pragma unroll
    for (int m = 0; m < n / 2; ++m) {
      const float keep = odd ? v[2 * m + 1] : v[2 * m];
      const float send = odd ? v[2 * m] : v[2 * m + 1];
      v[m] = keep + __shfl_xor(send, 1 << s);
    }
  }
  float r = v[0];
#pragma unroll
  for (int mask = N; mask < 64; mask <<= 1) r += __shfl_xor(r, mask);
  return r;
}

__host__ __device__ constexpr int flow_pow2_ceil(int n) { return n <= 1 ? 1 : 2 * flow_pow2_ceil((n + 1) / 2); }

}  // namespace shw
