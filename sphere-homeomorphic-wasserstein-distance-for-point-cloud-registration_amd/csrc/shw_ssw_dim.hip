// shw_ssw_dim.hip -- spherical sliced-Wasserstein for points on S^(D-1), D in 2..64 (the reference reads the point
// dimension from its input: `d = Xs.shape[1]`, max_spherical_sliced_w.py:304, frames (L, d, 2)).  The circular-OT
// solvers do not depend on D: they run on rows of circle coordinates (shw_circle_ot).  What depends on D sits on either
// side of the solve and lives here:
//   ssw_coords_dim_kernel            points x frames -> circle coordinates (reference :270-279), materialised;
//   ssw_backward_points_dim_kernel   coefficient rows (d cost / d coordinate) -> point gradients;
//   stiefel_frames_dim_kernel        reduced QR of (count, D, 2) Gaussian matrices (reference :307-308).
// The entries at the end run coordinates -> shw_circle_ot -> (caller: reduce) and the point gradients.  Nothing of the
// R^3 units is touched: every call with D = 3 that reached them still does.
#include <type_traits>

#include "ssw_common.hpp"

namespace shw {

constexpr int kMaxPointDim = 64;
constexpr int kDimSliceTile = 8;       // slices whose frames sit in LDS together
constexpr int kDimSliceGroup = 128;    // most slices of one workgroup of the coordinates kernel (blockIdx.y picks the group)

// Frames of slices [l0, l0 + kDimSliceTile) of one pair into LDS as [slice][d][2], zero beyond `dim` and beyond `l1`:
// a padded coordinate then adds fma(0, 0, acc) = acc (acc is never -0: it starts at +0), so one code path of DCAP
// coordinates serves every D of its class with the bits of the D-term sum.
template <int DCAP>
__device__ __forceinline__ void stage_frames(const float* __restrict__ Ub, int dim, int l0, int l1, float* fr) {
  constexpr int PER = DCAP * 2;
  for (int t = threadIdx.x; t < kDimSliceTile * PER; t += blockDim.x) {
    const int s = t / PER, e = t - s * PER;          // e = 2 d + k
    const int l = l0 + s;
    fr[t] = (l < l1 && e < 2 * dim) ? Ub[(long)l * (2 * dim) + e] : 0.f;
  }
}

// One lane owns one point: its DCAP coordinates (zero beyond dim) stay in registers across the slices of the group.
// (a, b) = U_l^T x accumulated as fma(x_d, U[d][k], acc) for d = 0..D-1 from +0 -- at D = 3 the expression of the R^3
// loader (ssw_common.hpp load_coords), hence the same bits; an all-zero point projects to (+0, +0) and lands on
// coordinate 0.  Frames are wave-uniform LDS reads (broadcast); stores run consecutive lanes along i.
template <int DCAP>
__global__ __launch_bounds__(256) void ssw_coords_dim_kernel(const float* __restrict__ x, const float* __restrict__ dirs,
                                                             int n, int dim, int slices, long u_pair_stride,
                                                             float* __restrict__ coords, int chunks, int group) {
  __shared__ float fr[kDimSliceTile * DCAP * 2];
  const int b = blockIdx.x / chunks;
  const int chunk = blockIdx.x - b * chunks;
  const int i = chunk * 256 + threadIdx.x;
  const int ic = min(i, n - 1);
  const float* X = x + ((long)b * n + ic) * dim;
  float px[DCAP];
#pragma unroll
  for (int d = 0; d < DCAP; ++d) px[d] = d < dim ? X[d] : 0.f;
  const float* Ub = dirs + (long)b * u_pair_stride;
  float* out = coords + (long)b * slices * n + i;            // + l * n per slice (64-bit)
  const int g0 = blockIdx.y * group;
  const int g1 = min(g0 + group, slices);
  for (int l0 = g0; l0 < g1; l0 += kDimSliceTile) {
    __syncthreads();                                          // the tile before is read
    stage_frames<DCAP>(Ub, dim, l0, g1, fr);
    __syncthreads();
    // one slice after the other (two in flight): unrolled over the tile, the compiler reads every frame of the tile ahead
    // and the largest D class spills
    const int live = min(kDimSliceTile, g1 - l0);
#pragma unroll 2
    for (int s = 0; s < live; ++s) {
      const float* U = fr + s * (DCAP * 2);
      float a = 0.f, bb = 0.f;
#pragma unroll
      for (int d = 0; d < DCAP; ++d) {
        a = fmaf(px[d], U[2 * d], a);
        bb = fmaf(px[d], U[2 * d + 1], bb);
      }
      const float c = circle_coord(a, bb);
      if (i < n) out[(long)(l0 + s) * n] = c;
    }
  }
}

// coefficient rows -> point gradients, the D-generic form of ssw_backward_points_kernel (shw_ssw_grad.hip):
//   grad[b,i,:] = scale (pair_w[b] + total_w[0]) sum_l coef[b,l,i] (-bb U_l[:,0] + a U_l[:,1]) / (2 pi (a^2 + bb^2)),
//   (a, bb) = U_l^T x[b,i], recomputed from the point; zero where a^2 + bb^2 == 0 as there.
// One thread owns a gradient row: it carries the point and the row in registers (2 DCAP) and adds the slices in
// ascending order -- no atomics, no partial sums, the same bits on every run.  The coefficients of a tile of slices are
// loaded before its arithmetic (kDimSliceTile loads in flight per lane).
template <int DCAP>
__global__ __launch_bounds__(256) void ssw_backward_points_dim_kernel(
    const float* __restrict__ xs, const float* __restrict__ xt, const float* __restrict__ dirs,
    const float* __restrict__ coef_s, const float* __restrict__ coef_t, int n, int m, int dim, int slices,
    long u_pair_stride, float scale, const float* __restrict__ pair_w, const float* __restrict__ total_w,
    float* __restrict__ grad_xs, float* __restrict__ grad_xt, int chunks_s) {
  __shared__ float fr[kDimSliceTile * DCAP * 2];
  const int b = blockIdx.y;
  const bool is_t = (int)blockIdx.x >= chunks_s;
  const int chunk = is_t ? blockIdx.x - chunks_s : blockIdx.x;
  const int cnt = is_t ? m : n;
  const int i = chunk * 256 + threadIdx.x;
  const int ic = min(i, cnt - 1);
  const float* X = (is_t ? xt : xs) + ((long)b * cnt + ic) * dim;
  const float* C = (is_t ? coef_t : coef_s) + (long)b * slices * cnt + ic;
  const float* Ub = dirs + (long)b * u_pair_stride;
  const float inv_two_pi = 0.159154936671257019f;
  float px[DCAP], g[DCAP];
#pragma unroll
  for (int d = 0; d < DCAP; ++d) {
    px[d] = d < dim ? X[d] : 0.f;
    g[d] = 0.f;
  }
  for (int l0 = 0; l0 < slices; l0 += kDimSliceTile) {
    float c[kDimSliceTile];
#pragma unroll
    for (int s = 0; s < kDimSliceTile; ++s) c[s] = C[(long)min(l0 + s, slices - 1) * cnt];
    __syncthreads();
    stage_frames<DCAP>(Ub, dim, l0, slices, fr);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kDimSliceTile; ++s) {
      if (l0 + s < slices) {                                  // (wave-uniform)
        const float* U = fr + s * (DCAP * 2);
        float a = 0.f, bb = 0.f;
#pragma unroll
        for (int d = 0; d < DCAP; ++d) {
          a = fmaf(px[d], U[2 * d], a);
          bb = fmaf(px[d], U[2 * d + 1], bb);
        }
        const float r2 = fmaf(a, a, bb * bb);
        const float w = r2 > 0.f ? c[s] * inv_two_pi / r2 : 0.f;
        const float wa = w * a, wb = -w * bb;
#pragma unroll
        for (int d = 0; d < DCAP; ++d) g[d] = fmaf(wa, U[2 * d + 1], fmaf(wb, U[2 * d], g[d]));
      }
    }
  }
  if (i < cnt) {
    float up = (pair_w || total_w) ? 0.f : 1.f;
    if (pair_w) up += pair_w[b];
    if (total_w) up += total_w[0];
    const float sc = scale * up;
    float* G = (is_t ? grad_xt : grad_xs) + ((long)b * cnt + i) * dim;
#pragma unroll
    for (int d = 0; d < DCAP; ++d)
      if (d < dim) G[d] = g[d] * sc;
  }
}

// Orthonormal 2-frames from Gaussian (D, 2) matrices: stiefel_frames_kernel (shw_capi.hip) for any D -- LAPACK's
// sgeqr2 + sorg2r for two columns, beta = -sign(alpha) * norm, one thread per matrix.  The columns are not held in
// registers (D is a run-time number): each step is a pass over the matrix in memory, and the updated second column
// c_d = z_d1 - tau1 w v_d is formed again by the one expression below wherever it is needed.  The arithmetic between
// the float input and the float output is double: the sums run over up to 64 terms, and a frame is then the float
// nearest to the exact factor instead of carrying a rounding per term (the kernel handles a few thousand matrices: its
// time does not show).
__device__ __forceinline__ double second_column(double z1, double tw, double v) { return fma(-tw, v, z1); }

__global__ __launch_bounds__(256) void stiefel_frames_dim_kernel(const float* __restrict__ z, int count, int dim,
                                                                 float* __restrict__ u) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const float* Z = z + (long)i * dim * 2;                   // (D, 2) row-major: Z[2 d + k]
  float* U = u + (long)i * dim * 2;
  // H1 from the first column
  const double alpha1 = Z[0];
  double ss = 0.0;
  for (int d = 1; d < dim; ++d) ss = fma((double)Z[2 * d], (double)Z[2 * d], ss);
  double tau1 = 0.0, scale1 = 0.0;
  if (ss != 0.0) {
    const double beta = -copysign(sqrt(fma(alpha1, alpha1, ss)), alpha1);
    tau1 = (beta - alpha1) / beta;
    scale1 = 1.0 / (alpha1 - beta);
  }
  // H1 applied to the second column: w = v^T z_1 (v_0 = 1, v_d = z_d0 * scale1)
  double w = Z[1];
  for (int d = 1; d < dim; ++d) w = fma(Z[2 * d] * scale1, (double)Z[2 * d + 1], w);
  const double tw = tau1 * w;
  // H2 from rows 1.. of the updated second column
  const double alpha2 = second_column(Z[3], tw, Z[2] * scale1);
  double ss2 = 0.0;
  for (int d = 2; d < dim; ++d) {
    const double c = second_column(Z[2 * d + 1], tw, Z[2 * d] * scale1);
    ss2 = fma(c, c, ss2);
  }
  double tau2 = 0.0, scale2 = 0.0;
  if (ss2 != 0.0) {
    const double beta = -copysign(sqrt(fma(alpha2, alpha2, ss2)), alpha2);
    tau2 = (beta - alpha2) / beta;
    scale2 = 1.0 / (alpha2 - beta);
  }
  // sorg2r: Q = H1 H2 [e1 e2].  q2 = H2 e2 = (0, 1 - tau2, -tau2 w2_d ...), then s = v^T q2
  const double q21 = 1.0 - tau2;
  double s = (Z[2] * scale1) * q21;
  for (int d = 2; d < dim; ++d) {
    const double c = second_column(Z[2 * d + 1], tw, Z[2 * d] * scale1);
    s = fma(Z[2 * d] * scale1, -tau2 * (c * scale2), s);
  }
  const double ts = tau1 * s;
  U[0] = (float)(1.0 - tau1);
  U[1] = (float)(-ts);
  for (int d = 1; d < dim; ++d) {
    const double v = Z[2 * d] * scale1;
    const double c = second_column(Z[2 * d + 1], tw, v);
    const double q2 = d == 1 ? q21 : -tau2 * (c * scale2);
    U[2 * d] = (float)(-tau1 * v);
    U[2 * d + 1] = (float)fma(-ts, v, q2);
  }
}

// D class of the two point kernels: coordinates carried per lane
inline int dim_class(int dim) { return dim <= 4 ? 4 : dim <= 8 ? 8 : dim <= 16 ? 16 : dim <= 32 ? 32 : 64; }

template <typename F>
static void with_dim_class(int dim, F&& f) {
  switch (dim_class(dim)) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    default: f(std::integral_constant<int, 64>{});
  }
}

static int launch_coords_dim(const float* x, const float* dirs, int pairs, int n, int dim, int slices,
                             long u_pair_stride, float* coords, hipStream_t stream) {
  const int chunks = (n + 255) / 256;
  const long blocks = (long)pairs * chunks;
  if (blocks > 0x7fffffffL) return (int)hipErrorInvalidValue;
  // slices per workgroup: 128 where the grid fills the chip (the point is read once per 128 coordinates written); a
  // small grid -- one pair of 1200 points is 5 workgroups -- is cut into groups down to one LDS tile of slices until
  // there are 1024 workgroups
  int group = kDimSliceGroup;
  while (group > kDimSliceTile && blocks * ((slices + group - 1) / group) < 1024) group >>= 1;
  const dim3 grid((unsigned)blocks, (unsigned)((slices + group - 1) / group)), block(256);
  with_dim_class(dim, [&](auto dc) {
    hipLaunchKernelGGL((ssw_coords_dim_kernel<decltype(dc)::value>), grid, block, 0, stream, x, dirs, n, dim, slices,
                       u_pair_stride, coords, chunks, group);
  });
  return (int)hipGetLastError();
}

static bool dim_sizes_ok(int pairs, int n, int m, int dim, int slices, long u_pair_stride) {
  if (dim < 2 || dim > kMaxPointDim) return false;
  if (pairs < 0 || slices < 0 || n < 1 || m < 1) return false;
  if (slices > 65535 * kDimSliceGroup) return false;
  if (u_pair_stride != 0 && u_pair_stride < (long)slices * dim * 2) return false;
  return true;
}

}  // namespace shw

extern "C" {

int shw_max_point_dim(void) { return shw::kMaxPointDim; }

int shw_stiefel_frames_dim(const float* z, long count, int dim, float* u, void* stream) {
  if (dim < 2 || dim > shw::kMaxPointDim) return (int)hipErrorInvalidValue;
  if (!z || !u || count < 0 || count > 0x7fffffffL) return (int)hipErrorInvalidValue;
  if (count == 0) return 0;
  hipLaunchKernelGGL(shw::stiefel_frames_dim_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, z, (int)count, dim, u);
  return (int)hipGetLastError();
}

int shw_ssw_coords_dim(const float* x, const float* dirs, int pairs, int n, int dim, int slices, long u_pair_stride,
                       float* coords, void* stream) {
  if (!shw::dim_sizes_ok(pairs, n, n, dim, slices, u_pair_stride) || n > SHW_MAX_POINTS) return (int)hipErrorInvalidValue;
  if (!x || !dirs || !coords) return (int)hipErrorInvalidValue;
  if (pairs == 0 || slices == 0) return 0;
  return shw::launch_coords_dim(x, dirs, pairs, n, dim, slices, u_pair_stride, coords, (hipStream_t)stream);
}

size_t shw_ssw_dim_workspace_bytes(int pairs, int n, int m, int slices) {
  if (pairs < 0 || n < 0 || m < 0 || slices < 0) return 0;
  return (size_t)pairs * (size_t)slices * ((size_t)n + (size_t)m) * sizeof(float);
}

int shw_ssw_forward_dim(const float* xs, const float* xt, const float* dirs, const float* wu, const float* wv,
                        long wu_pair_stride, long wv_pair_stride, int pairs, int n, int m, int dim, int slices,
                        long u_pair_stride, float p, void* workspace, float* slice_cost, float* slice_aux, float* coef_s,
                        float* coef_t, void* stream) {
  if (!shw::dim_sizes_ok(pairs, n, m, dim, slices, u_pair_stride) || !(p >= 1.f)) return (int)hipErrorInvalidValue;
  // the limits of shw_circle_ot, checked here so that nothing is enqueued for a call it would refuse
  const int limit = (wu || wv || (p != 1.f && n != m)) ? 4096 : SHW_MAX_POINTS;
  if (n > limit || m > limit) return (int)hipErrorInvalidValue;
  if ((long)pairs * slices > 0x7fffffffL) return (int)hipErrorInvalidValue;
  if ((wu_pair_stride != 0 && wu_pair_stride < n) || (wv_pair_stride != 0 && wv_pair_stride < m)) return (int)hipErrorInvalidValue;
  if (!xs || !xt || !dirs || !workspace || !slice_cost) return (int)hipErrorInvalidValue;
  if ((coef_s == nullptr) != (coef_t == nullptr)) return (int)hipErrorInvalidValue;
  if (pairs == 0 || slices == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  float* cs = static_cast<float*>(workspace);
  float* ct = cs + (size_t)pairs * slices * n;
  int rc = shw::launch_coords_dim(xs, dirs, pairs, n, dim, slices, u_pair_stride, cs, st);
  if (rc) return rc;
  rc = shw::launch_coords_dim(xt, dirs, pairs, m, dim, slices, u_pair_stride, ct, st);
  if (rc) return rc;
  const bool per_pair = (wu && wu_pair_stride != 0) || (wv && wv_pair_stride != 0);
  if (!per_pair)                     // uniform or shared weights: every (pair, slice) is one row of one launch
    return shw_circle_ot(cs, ct, wu, wv, 0, 0, pairs * slices, n, m, p, SHW_CIRCLE_AS_SLICED, slice_cost, slice_aux,
                         coef_s, coef_t, stream);
  // per-pair weights: the circle level's row stride cannot say "one row of weights per `slices` rows"
  for (int b = 0; b < pairs; ++b) {
    const size_t r0 = (size_t)b * slices;
    rc = shw_circle_ot(cs + r0 * n, ct + r0 * m, wu ? wu + (size_t)b * wu_pair_stride : nullptr,
                       wv ? wv + (size_t)b * wv_pair_stride : nullptr, 0, 0, slices, n, m, p, SHW_CIRCLE_AS_SLICED,
                       slice_cost + r0, slice_aux ? slice_aux + r0 : nullptr, coef_s ? coef_s + r0 * n : nullptr,
                       coef_t ? coef_t + r0 * m : nullptr, stream);
    if (rc) return rc;
  }
  return 0;
}

int shw_ssw_backward_points_dim(const float* xs, const float* xt, const float* dirs, const float* coef_s,
                                const float* coef_t, int pairs, int n, int m, int dim, int slices, long u_pair_stride,
                                float scale, const float* pair_w, const float* total_w, float* grad_xs, float* grad_xt,
                                void* stream) {
  if (!shw::dim_sizes_ok(pairs, n, m, dim, slices, u_pair_stride)) return (int)hipErrorInvalidValue;
  if (n > SHW_MAX_POINTS || m > SHW_MAX_POINTS) return (int)hipErrorInvalidValue;
  if (!xs || !xt || !dirs || !coef_s || !coef_t || !grad_xs || !grad_xt) return (int)hipErrorInvalidValue;
  if (pairs == 0) return 0;
  const int chunks_s = (n + 255) / 256, chunks_t = (m + 255) / 256;
  // pairs ride on gridDim.y (<= 65535): larger batches go out as several launches over pair blocks
  for (int b0 = 0; b0 < pairs; b0 += 65535) {
    const int nb = pairs - b0 < 65535 ? pairs - b0 : 65535;
    const dim3 grid(chunks_s + chunks_t, nb), block(256);
    shw::with_dim_class(dim, [&](auto dc) {
      hipLaunchKernelGGL((shw::ssw_backward_points_dim_kernel<decltype(dc)::value>), grid, block, 0, (hipStream_t)stream,
                         xs + (size_t)b0 * n * dim, xt + (size_t)b0 * m * dim, dirs + (size_t)b0 * u_pair_stride,
                         coef_s + (size_t)b0 * slices * n, coef_t + (size_t)b0 * slices * m, n, m, dim, slices,
                         u_pair_stride, scale, pair_w ? pair_w + b0 : nullptr, total_w, grad_xs + (size_t)b0 * n * dim,
                         grad_xt + (size_t)b0 * m * dim, chunks_s);
    });
  }
  return (int)hipGetLastError();
}

}  // extern "C"
