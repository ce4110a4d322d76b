// shw_ssw_dirs.hip -- spherical sliced-Wasserstein: gradients with respect to the slicing frames.
//
// Every training-form forward leaves the coefficient rows coef[b,l,i] = d cost(b,l) / d coord[b,l,i] in original point
// order.  The point-gradient kernels fold them with d coord / d x; the kernels here fold the SAME rows with
// d coord / d U.  With (a, bb) = U_l^T x_i, r2 = a^2 + bb^2 and coord = (atan2(-bb, -a) + pi) / (2 pi):
//   grad_dirs[b,l,:,0] = sc_b sum_i coef[b,l,i] (-bb_i) / (2 pi r2_i) x_i
//   grad_dirs[b,l,:,1] = sc_b sum_i coef[b,l,i] (  a_i) / (2 pi r2_i) x_i,      sc_b = scale (pair_w[b] + total_w[0]),
// the sum over the points of both clouds (coef_s with xs, then coef_t with xt); a point with r2 == 0 adds 0, the guard
// of the point-gradient kernels.  grad_dirs is always (pairs, slices, dim, 2): frames shared by several pairs sum their
// rows on the host side (the convention of shw_esw_backward_dirs).
//
//   ssw_backward_dirs_kernel       dim = 3, float or double: one wavefront owns R consecutive slices of one pair and
//                                  walks both clouds, a lane holding V points in registers across the R rows;
//   ssw_backward_dirs_dim_kernel   dim 2..64, float: a block shares 64-point tiles in LDS among its rows; per tile a
//                                  wavefront forms the two weights per point of its rows (lane = point), then the lanes
//                                  turn to own a coordinate and add weight x coordinate over the tile's points.
// Sums run in a fixed order -- a lane adds its points in ascending order, lanes are added in a butterfly -- and nothing
// is atomic: the result has the same bits on every run.  No kernel of another unit is touched.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "../../include/shw.h"

namespace shw {
namespace dirs {

constexpr int kWaveLanes = 64;
constexpr int kMaxDim = 64;

template <typename T> struct Consts;
template <> struct Consts<float> { static constexpr float inv_two_pi = 0.159154936671257019f; };
template <> struct Consts<double> { static constexpr double inv_two_pi = 0.15915494309189533577; };

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWaveLanes);     // fixed tree
  return v;
}

template <typename T>
__device__ __forceinline__ T upstream(T scale, const T* pair_w, const T* total_w, int b) {
  T up = (pair_w || total_w) ? T(0) : T(1);
  if (pair_w) up += pair_w[b];
  if (total_w) up += total_w[0];
  return scale * up;
}

// One cloud of one pair into the R x 6 accumulators of a lane.  V = 4 (float, cnt a multiple of 4, 16-byte aligned
// rows): a lane owns four consecutive points, their 12 coordinates come in as three 16-byte loads and their coefficients
// of one slice as one -- the load shape of ssw_backward_points4_kernel.  V = 1: one point, scalar loads, any cnt.
// The point stays in registers across the R slices, so a coefficient row costs 3 / R bytes of (cached) point traffic
// per byte streamed.  U: the R frames of the wave, wave-uniform.
template <typename T, int V, int R>
__device__ __forceinline__ void fold_cloud(const T* __restrict__ X, const T* __restrict__ C, int cnt,
                                           const int (&rows_off)[R], const T (&U)[R][6], int lane, T (&acc)[R][6]) {
  for (int i0 = lane * V; i0 < cnt; i0 += kWaveLanes * V) {
    T p[3 * V];
    T c[R][V];
    if constexpr (V == 4) {
      const float4* X4 = reinterpret_cast<const float4*>(X + 3 * (long)i0);
      const float4 q0 = X4[0], q1 = X4[1], q2 = X4[2];
      p[0] = q0.x; p[1] = q0.y; p[2] = q0.z; p[3] = q0.w; p[4] = q1.x; p[5] = q1.y; p[6] = q1.z; p[7] = q1.w;
      p[8] = q2.x; p[9] = q2.y; p[10] = q2.z; p[11] = q2.w;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float4 c4 = *reinterpret_cast<const float4*>(C + (long)rows_off[r] * cnt + i0);
        c[r][0] = c4.x; c[r][1] = c4.y; c[r][2] = c4.z; c[r][3] = c4.w;
      }
    } else {
      p[0] = X[3 * (long)i0]; p[1] = X[3 * (long)i0 + 1]; p[2] = X[3 * (long)i0 + 2];
#pragma unroll
      for (int r = 0; r < R; ++r) c[r][0] = C[(long)rows_off[r] * cnt + i0];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int q = 0; q < V; ++q) {
        const T px = p[3 * q], py = p[3 * q + 1], pz = p[3 * q + 2];
        // the projection as the point-gradient kernels form it
        const T a = fma(pz, U[r][4], fma(py, U[r][2], px * U[r][0]));
        const T bb = fma(pz, U[r][5], fma(py, U[r][3], px * U[r][1]));
        const T r2 = fma(a, a, bb * bb);
        const T w = r2 > T(0) ? c[r][q] * Consts<T>::inv_two_pi / r2 : T(0);   // (0, 0) projection: no angle, no gradient
        const T s0 = -w * bb, s1 = w * a;
        acc[r][0] = fma(s0, px, acc[r][0]);
        acc[r][1] = fma(s1, px, acc[r][1]);
        acc[r][2] = fma(s0, py, acc[r][2]);
        acc[r][3] = fma(s1, py, acc[r][3]);
        acc[r][4] = fma(s0, pz, acc[r][4]);
        acc[r][5] = fma(s1, pz, acc[r][5]);
      }
    }
  }
}

// grid (ceil(ceil(slices / R) / waves), pairs of this launch), block 64 * waves: wave w of block x owns slices
// [R g, R g + R) of pair blockIdx.y, g = x * waves + w.  No LDS, no barrier: the only exchange is the butterfly that ends
// a row.  A slice past the end is computed on the last row's data and not written.
template <typename T, int V, int R>
__global__ __launch_bounds__(256) void ssw_backward_dirs_kernel(
    const T* __restrict__ xs, const T* __restrict__ xt, const T* __restrict__ dirs, const T* __restrict__ coef_s,
    const T* __restrict__ coef_t, int n, int m, int slices, long u_pair_stride, T scale, const T* __restrict__ pair_w,
    const T* __restrict__ total_w, T* __restrict__ grad_dirs) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int waves = blockDim.x >> 6;
  const int b = blockIdx.y;
  const int l0 = (blockIdx.x * waves + wave) * R;
  if (l0 >= slices) return;                                   // (wave-uniform; the kernel has no barrier)
  const T* Ub = dirs + (long)b * u_pair_stride;
  T U[R][6];
  T acc[R][6];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int l = min(l0 + r, slices - 1);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      U[r][k] = Ub[(long)l * 6 + k];
      acc[r][k] = T(0);
    }
  }
  // row r of the group is rows_off[r] rows behind row l0; a row past the last slice re-reads the last one
  int rows_off[R];
#pragma unroll
  for (int r = 0; r < R; ++r) rows_off[r] = min(l0 + r, slices - 1) - l0;
  fold_cloud<T, V, R>(xs + (long)b * n * 3, coef_s + ((long)b * slices + l0) * n, n, rows_off, U, lane, acc);
  fold_cloud<T, V, R>(xt + (long)b * m * 3, coef_t + ((long)b * slices + l0) * m, m, rows_off, U, lane, acc);
  const T sc = upstream<T>(scale, pair_w, total_w, b);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    T out[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) out[k] = wave_sum(acc[r][k]) * sc;
    if (lane == 0 && l0 + r < slices) {
      T* G = grad_dirs + ((long)b * slices + l0 + r) * 6;
#pragma unroll
      for (int k = 0; k < 6; ++k) G[k] = out[k];              // [d][k] order: (slices, 3, 2)
    }
  }
}

// Any dim in 2..64.  Per pair this is a small matrix product, G (2 L x dim) = S (2 L x N) X (N x dim) with
// S[l, i] = (-w bb, w a), w = coef / (2 pi r2).  Holding the 2 dim sums of a row per lane would be 128 accumulators at
// dim = 64 and spill; instead the lanes change roles inside a 64-point tile, and the tile is shared by all rows of the
// block (waves x RW consecutive slices of one pair, RW rows per wavefront):
//   1. the block copies the tile (64 points x dim floats, contiguous in memory) to LDS, rows padded to an odd stride;
//   2. lane = point: (a, bb) of the wave's RW rows from the LDS row (conflict-free: odd stride; one read of x serves the
//      RW frames), then the RW weight pairs, written to LDS;
//   3. lane = (group, coordinate): DC = the power of two >= dim lanes span the coordinates, the 64 / DC groups split the
//      tile's points; a lane adds s0[j] x[j][d] and s1[j] x[j][d] over its group's points in ascending order, one read
//      of x[j][d] serving the RW rows.
// 2 RW accumulators per lane whatever dim is; after both clouds the groups are added in a butterfly over the lane bits
// above DC.  A row past the last slice repeats the last one and is not written, so every wave meets every barrier.
template <int RW>
__global__ __launch_bounds__(256) void ssw_backward_dirs_dim_kernel(
    const float* __restrict__ xs, const float* __restrict__ xt, const float* __restrict__ dirs,
    const float* __restrict__ coef_s, const float* __restrict__ coef_t, int n, int m, int dim, int dc_log2, int slices,
    long u_pair_stride, float scale, const float* __restrict__ pair_w, const float* __restrict__ total_w,
    float* __restrict__ grad_dirs) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int waves = blockDim.x >> 6;
  const int b = blockIdx.y;
  const int l_base = (blockIdx.x * waves + wave) * RW;
  const int ld = dim | 1;                                     // odd row stride of the tile
  float* tile = lds;                                          // [64][ld], shared by the block
  float2* fr = reinterpret_cast<float2*>(tile + kWaveLanes * ld) + wave * RW * dim;                  // [RW][dim] (u1_d, u2_d)
  float2* sw = reinterpret_cast<float2*>(tile + kWaveLanes * ld) + waves * RW * dim + wave * RW * kWaveLanes;   // [RW][64]
  int lrow[RW];
#pragma unroll
  for (int r = 0; r < RW; ++r) {
    lrow[r] = min(l_base + r, slices - 1);
    const float* U = dirs + (long)b * u_pair_stride + (long)lrow[r] * dim * 2;
    for (int d = lane; d < dim; d += kWaveLanes) fr[r * dim + d] = make_float2(U[2 * d], U[2 * d + 1]);
  }
  const int DC = 1 << dc_log2;
  const int groups = kWaveLanes >> dc_log2;
  const int grp = lane >> dc_log2, dl = lane & (DC - 1);
  const int stage_rows = blockDim.x >> dc_log2, stage_row = tid >> dc_log2;     // the block's (row, coordinate) copy grid
  const float inv_two_pi = 0.159154936671257019f;
  float g0[RW], g1[RW];
#pragma unroll
  for (int r = 0; r < RW; ++r) g0[r] = g1[r] = 0.f;
  for (int cloud = 0; cloud < 2; ++cloud) {
    const int cnt = cloud ? m : n;
    const float* X = (cloud ? xt : xs) + (long)b * cnt * dim;
    const float* C = (cloud ? coef_t : coef_s) + (long)b * slices * cnt;
    for (int i0 = 0; i0 < cnt; i0 += kWaveLanes) {
      const int tp = min(kWaveLanes, cnt - i0);               // points of this tile
      float c[RW];
#pragma unroll
      for (int r = 0; r < RW; ++r) c[r] = lane < tp ? C[(long)lrow[r] * cnt + i0 + lane] : 0.f;
      __syncthreads();                                        // the tile before is read
      if (dl < dim)
        for (int j = stage_row; j < tp; j += stage_rows) tile[j * ld + dl] = X[(long)(i0 + j) * dim + dl];
      __syncthreads();
      {
        const float* row = tile + min(lane, tp - 1) * ld;
        float a[RW], bb[RW];
#pragma unroll
        for (int r = 0; r < RW; ++r) a[r] = bb[r] = 0.f;
        for (int d = 0; d < dim; ++d) {
          const float xv = row[d];
#pragma unroll
          for (int r = 0; r < RW; ++r) {
            const float2 u = fr[r * dim + d];
            a[r] = fmaf(xv, u.x, a[r]);
            bb[r] = fmaf(xv, u.y, bb[r]);
          }
        }
#pragma unroll
        for (int r = 0; r < RW; ++r) {
          const float r2 = fmaf(a[r], a[r], bb[r] * bb[r]);
          const float w = (lane < tp && r2 > 0.f) ? c[r] * inv_two_pi / r2 : 0.f;
          sw[r * kWaveLanes + lane] = make_float2(-w * bb[r], w * a[r]);
        }
      }
      __syncthreads();
      if (dl < dim) {
        for (int j = grp; j < tp; j += groups) {
          const float xv = tile[j * ld + dl];
#pragma unroll
          for (int r = 0; r < RW; ++r) {
            const float2 s = sw[r * kWaveLanes + j];
            g0[r] = fmaf(s.x, xv, g0[r]);
            g1[r] = fmaf(s.y, xv, g1[r]);
          }
        }
      }
    }
  }
  const float sc = upstream<float>(scale, pair_w, total_w, b);
#pragma unroll
  for (int r = 0; r < RW; ++r) {
    float s0 = g0[r], s1 = g1[r];
    for (int off = 32; off >= DC; off >>= 1) {                // the groups, in a fixed tree
      s0 += __shfl_xor(s0, off, kWaveLanes);
      s1 += __shfl_xor(s1, off, kWaveLanes);
    }
    if (l_base + r < slices && lane < dim) {
      float* G = grad_dirs + ((long)b * slices + l_base + r) * dim * 2 + 2 * lane;
      G[0] = s0 * sc;
      G[1] = s1 * sc;
    }
  }
}

// floats of dynamic LDS of a block of the kernel above
static size_t dim_lds_floats(int dim, int waves, int rw) {
  return (size_t)kWaveLanes * (dim | 1) + 2 * ((size_t)waves * rw * dim + (size_t)waves * rw * kWaveLanes);
}

static bool sizes_ok(int pairs, int n, int m, int dim, int slices, long u_pair_stride, int limit) {
  if (dim < 2 || dim > kMaxDim) return false;
  if (pairs < 0 || slices < 0 || n < 1 || m < 1 || n > limit || m > limit) return false;
  if (u_pair_stride != 0 && u_pair_stride < (long)slices * dim * 2) return false;
  return true;
}

// Rows per wave: 4 once the grid fills the chip several times over without it (the point loads are then shared by four
// rows), 1 for small problems (the notebooks' one pair x 100 slices keeps 100 waves instead of 25).  Waves per block: 4,
// or as many as the pair has row groups.
template <typename T, int V>
static int launch3(const T* xs, const T* xt, const T* dirs, const T* coef_s, const T* coef_t, int pairs, int n, int m,
                   int slices, long u_pair_stride, T scale, const T* pair_w, const T* total_w, T* grad_dirs,
                   hipStream_t stream) {
  const bool wide = (long)pairs * slices >= 8192 && slices >= 4;
  const int R = wide ? 4 : 1;
  const int groups = (slices + R - 1) / R;
  const int waves = groups < 4 ? groups : 4;
  for (int b0 = 0; b0 < pairs; b0 += 65535) {                // pairs ride on gridDim.y
    const int nb = pairs - b0 < 65535 ? pairs - b0 : 65535;
    const dim3 grid((unsigned)((groups + waves - 1) / waves), (unsigned)nb), block(64 * waves);
#define SHW_LAUNCH_DIRS(RR)                                                                                             \
    hipLaunchKernelGGL((ssw_backward_dirs_kernel<T, V, RR>), grid, block, 0, stream, xs + (size_t)b0 * n * 3,            \
                       xt + (size_t)b0 * m * 3, dirs + (size_t)b0 * u_pair_stride, coef_s + (size_t)b0 * slices * n,     \
                       coef_t + (size_t)b0 * slices * m, n, m, slices, u_pair_stride, scale,                             \
                       pair_w ? pair_w + b0 : nullptr, total_w, grad_dirs + (size_t)b0 * slices * 6)
    if (wide) SHW_LAUNCH_DIRS(4);
    else SHW_LAUNCH_DIRS(1);
#undef SHW_LAUNCH_DIRS
  }
  return (int)hipGetLastError();
}

}  // namespace dirs
}  // namespace shw

extern "C" {

int shw_ssw_backward_dirs(const float* xs, const float* xt, const float* dirs, const float* coef_s, const float* coef_t,
                          int pairs, int n, int m, int slices, long u_pair_stride, float scale, const float* pair_w,
                          const float* total_w, float* grad_dirs, void* stream) {
  if (!xs || !xt || !dirs || !coef_s || !coef_t || !grad_dirs) return (int)hipErrorInvalidValue;
  if (!shw::dirs::sizes_ok(pairs, n, m, 3, slices, u_pair_stride, SHW_MAX_POINTS)) return (int)hipErrorInvalidValue;
  if (pairs == 0 || slices == 0) return 0;
  const bool vec = n % 4 == 0 && m % 4 == 0 &&
                   ((reinterpret_cast<uintptr_t>(xs) | reinterpret_cast<uintptr_t>(xt) | reinterpret_cast<uintptr_t>(coef_s) |
                     reinterpret_cast<uintptr_t>(coef_t)) & 15) == 0;
  if (vec)
    return shw::dirs::launch3<float, 4>(xs, xt, dirs, coef_s, coef_t, pairs, n, m, slices, u_pair_stride, scale, pair_w,
                                        total_w, grad_dirs, (hipStream_t)stream);
  return shw::dirs::launch3<float, 1>(xs, xt, dirs, coef_s, coef_t, pairs, n, m, slices, u_pair_stride, scale, pair_w,
                                      total_w, grad_dirs, (hipStream_t)stream);
}

int shw_ssw_backward_dirs_f64(const double* xs, const double* xt, const double* dirs, const double* coef_s,
                              const double* coef_t, int pairs, int n, int m, int slices, long u_pair_stride, double scale,
                              const double* pair_w, const double* total_w, double* grad_dirs, void* stream) {
  if (!xs || !xt || !dirs || !coef_s || !coef_t || !grad_dirs) return (int)hipErrorInvalidValue;
  // one entry for both float64 paths: the larger of their two limits, n != m allowed
  const int l1 = shw_max_points_f64(), l2 = shw_max_points_f64_general();
  if (!shw::dirs::sizes_ok(pairs, n, m, 3, slices, u_pair_stride, l1 > l2 ? l1 : l2)) return (int)hipErrorInvalidValue;
  if (pairs == 0 || slices == 0) return 0;
  return shw::dirs::launch3<double, 1>(xs, xt, dirs, coef_s, coef_t, pairs, n, m, slices, u_pair_stride, scale, pair_w,
                                       total_w, grad_dirs, (hipStream_t)stream);
}

int shw_ssw_backward_dirs_dim(const float* xs, const float* xt, const float* dirs, const float* coef_s,
                              const float* coef_t, int pairs, int n, int m, int dim, int slices, long u_pair_stride,
                              float scale, const float* pair_w, const float* total_w, float* grad_dirs, void* stream) {
  if (!xs || !xt || !dirs || !coef_s || !coef_t || !grad_dirs) return (int)hipErrorInvalidValue;
  if (!shw::dirs::sizes_ok(pairs, n, m, dim, slices, u_pair_stride, SHW_MAX_POINTS)) return (int)hipErrorInvalidValue;
  if (pairs == 0 || slices == 0) return 0;
  int dc_log2 = 1;
  while ((1 << dc_log2) < dim) ++dc_log2;
  // rows per wave: 4 once that still leaves a thousand blocks (a point tile in LDS then serves 16 rows), else 1
  const bool wide = (long)pairs * slices >= 4096 && slices >= 4;
  const int rw = wide ? 4 : 1;
  const int row_groups = (slices + rw - 1) / rw;
  const int waves = row_groups < 4 ? row_groups : 4;
  const size_t lds = shw::dirs::dim_lds_floats(dim, waves, rw) * sizeof(float);   // at most 33 KB (dim 64, 4 x 4 rows)
  for (int b0 = 0; b0 < pairs; b0 += 65535) {                         // pairs ride on gridDim.y
    const int nb = pairs - b0 < 65535 ? pairs - b0 : 65535;
    const dim3 grid((unsigned)((row_groups + waves - 1) / waves), (unsigned)nb), block(64 * waves);
#define SHW_LAUNCH_DIRS_DIM(RW)                                                                                         \
    hipLaunchKernelGGL(shw::dirs::ssw_backward_dirs_dim_kernel<RW>, grid, block, lds, (hipStream_t)stream,              \
                       xs + (size_t)b0 * n * dim, xt + (size_t)b0 * m * dim, dirs + (size_t)b0 * u_pair_stride,          \
                       coef_s + (size_t)b0 * slices * n, coef_t + (size_t)b0 * slices * m, n, m, dim, dc_log2, slices,   \
                       u_pair_stride, scale, pair_w ? pair_w + b0 : nullptr, total_w,                                    \
                       grad_dirs + (size_t)b0 * slices * dim * 2)
    if (wide) SHW_LAUNCH_DIRS_DIM(4);
    else SHW_LAUNCH_DIRS_DIM(1);
#undef SHW_LAUNCH_DIRS_DIM
  }
  return (int)hipGetLastError();
}

}  // extern "C"
