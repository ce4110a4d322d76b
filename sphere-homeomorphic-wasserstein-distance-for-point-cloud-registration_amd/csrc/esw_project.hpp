// esw_project.hpp -- the D-generic projection loader of the Euclidean sliced-W kernels, shared by shw_esw_dim.hip (equal
// sizes) and shw_line_ot.hip (unequal sizes and weights): both must form bit-identical keys.
#pragma once
#include "ssw_common.hpp"

namespace shw {

// projections of one cloud (count, dim) on the wave-uniform direction row T (scalar loads); padding keys are +inf.
// Chunks of CH points x DG coordinates: the CH*DG loads of a chunk are in flight together (the R^3 loader's 8 x 3),
// then the FMAs run in coordinate order, so key = x0*t0, then fma(x_d, t_d, key) for d = 1..dim-1.  Coordinates past
// dim re-read the last one and are not used.
template <int EPT>
__device__ __forceinline__ void load_projections_dim(const float* __restrict__ X, int count, int dim, int lane,
                                                     const float* __restrict__ T, float (&key)[EPT]) {
  constexpr int CH = EPT < 8 ? EPT : 8;
  constexpr int DG = 4;
#pragma unroll
  for (int r0 = 0; r0 < EPT; r0 += CH) {
    int off[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) off[j] = min((r0 + j) * kWave + lane, count - 1) * dim;
#pragma nounroll
    for (int d0 = 0; d0 < dim; d0 += DG) {
      float xv[CH][DG];
#pragma unroll
      for (int j = 0; j < CH; ++j)
#pragma unroll
        for (int k = 0; k < DG; ++k) xv[j][k] = X[off[j] + min(d0 + k, dim - 1)];
#pragma unroll
      for (int k = 0; k < DG; ++k) {
        const int d = d0 + k;
        if (d < dim) {
          const float t = T[d];
#pragma unroll
          for (int j = 0; j < CH; ++j) key[r0 + j] = (d == 0) ? xv[j][k] * t : fmaf(xv[j][k], t, key[r0 + j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < CH; ++j)
      if ((r0 + j) * kWave + lane >= count) key[r0 + j] = __builtin_inff();
    __builtin_amdgcn_sched_barrier(0);
  }
}

}  // namespace shw
