// shw_esw.hip -- Euclidean sliced-Wasserstein (the notebooks' SWD baseline): project both clouds on L
// unit directions of R^3, sort both projected sequences, sum |u_(i) - v_(i)|^p.
//
// Replaces `sliced_wasserstein_distance` (Wasserstein_flow_problem/Flow_cube.ipynb:280-292; the same cell
// in Flow_ellipsoid*.ipynb), which needs equal sample counts.  It is the spherical kernel without the
// circle: no atan2, no cyclic shift (k = 0), no wrap -- one wavefront per (pair, slice), the same
// register-resident sort.  Per slice it returns S_l = sum_i |u_(i) - v_(i)|^p; the outer
// (mean_l S_l)^(1/p) of the notebook is host-side arithmetic on L numbers.  The forward kernel is the shared body
// euclid_forward (euclid_common.hpp) with the R^3 projection as its key.
#include "euclid_common.hpp"

namespace shw {

struct EswArgs {
  const float* xs;
  const float* xt;
  const float* thetas;     // (slices, 3) or (pairs, slices, 3) unit directions
  float* slice_sum;        // (pairs*slices)
  float* coef_s;           // optional (pairs*slices*n): d S_l / d projection, original point order
  float* coef_t;
  int pairs, n, slices;
  long theta_pair_stride;  // 0 = shared
  float p;
  int p_int;
  int num_groups;
};

// the key of a point is its projection on the slice's direction; the coefficient is the derivative itself
struct EswKey {
  static constexpr bool kRolledGeneralP = false;
  using row_t = int;       // pairs * slices, as the entry computes it
  const float *xs, *xt, *thetas;
  long theta_pair_stride;
  int slices;
  long cloud;              // offset of the pair's clouds
  float tx, ty, tz;
  __device__ __forceinline__ void begin_row(int s, int n) {
    const int b = s / slices, l = s - b * slices;
    const float* T = thetas + (long)b * theta_pair_stride + (long)l * 3;
    tx = T[0]; ty = T[1]; tz = T[2];
    cloud = (long)b * n * 3;
  }
  template <int EPT>
  __device__ __forceinline__ void load(int which, int, int n, int lane, float (&key)[EPT]) const {
    load_projections<EPT>((which == 0 ? xt : xs) + cloud, n, lane, tx, ty, tz, key);
  }
  template <bool NEG>
  static __device__ __forceinline__ float coef(float g, float) { return NEG ? -g : g; }
};

template <int EPT, int WAVES, int PMODE, bool GRAD>
__global__ __launch_bounds__(WAVES * 64) void esw_kernel(EswArgs A) {
  euclid_forward<EPT, WAVES, PMODE, GRAD>(EswKey{A.xs, A.xt, A.thetas, A.theta_pair_stride, A.slices},
                                          A.pairs * A.slices, A.n, A.num_groups, A.p, A.p_int, A.slice_sum,
                                          A.coef_s, A.coef_t);
}

// grad[b,i,:] = sum_l w[b,l] * coef[b,l,i] * theta[b,l,:]   (w = upstream gradient of the per-slice sums)
__global__ __launch_bounds__(256) void esw_backward_points_kernel(const float* __restrict__ thetas,
                                                                  const float* __restrict__ coef_s,
                                                                  const float* __restrict__ coef_t,
                                                                  const float* __restrict__ slice_w, int n,
                                                                  int slices, long theta_pair_stride,
                                                                  float* __restrict__ grad_xs,
                                                                  float* __restrict__ grad_xt, int chunks) {
  const int b = blockIdx.y;
  const bool is_t = (int)blockIdx.x >= chunks;
  const int chunk = is_t ? blockIdx.x - chunks : blockIdx.x;
  const int i = chunk * 256 + threadIdx.x;
  const int ic = min(i, n - 1);
  const float* C = (is_t ? coef_t : coef_s) + (long)b * slices * n;
  float* G = (is_t ? grad_xt : grad_xs) + (long)b * n * 3;
  const float* Tb = thetas + (long)b * theta_pair_stride;
  const float* W = slice_w + (long)b * slices;
  float gx = 0.f, gy = 0.f, gz = 0.f;
  for (int l = 0; l < slices; ++l) {
    const float c = C[(long)l * n + ic] * W[l];
    gx = fmaf(c, Tb[3 * l], gx);
    gy = fmaf(c, Tb[3 * l + 1], gy);
    gz = fmaf(c, Tb[3 * l + 2], gz);
  }
  if (i < n) { G[3 * i] = gx; G[3 * i + 1] = gy; G[3 * i + 2] = gz; }
}

// grad_theta[b,l,:] = w[b,l] * sum_i ( coef_s[b,l,i] * xs[b,i,:] + coef_t[b,l,i] * xt[b,i,:] )
// (the projections are x . theta, so d S_l / d theta is the coefficient-weighted sum of the points; used by
// the notebooks' max-sliced-W, which ascends on the direction).  One workgroup per (slice, pair), fixed-order tree.
__global__ __launch_bounds__(256) void esw_backward_dirs_kernel(const float* __restrict__ xs,
                                                                const float* __restrict__ xt,
                                                                const float* __restrict__ coef_s,
                                                                const float* __restrict__ coef_t,
                                                                const float* __restrict__ slice_w, int n, int slices,
                                                                float* __restrict__ grad_thetas) {
  __shared__ float red[3][4];
  const int l = blockIdx.x, b = blockIdx.y;
  const float* Xs = xs + (long)b * n * 3;
  const float* Xt = xt + (long)b * n * 3;
  const float* Cs = coef_s + ((long)b * slices + l) * n;
  const float* Ct = coef_t + ((long)b * slices + l) * n;
  float g[3] = {0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < n; i += 256) {
    const float cs = Cs[i], ct = Ct[i];
#pragma unroll
    for (int d = 0; d < 3; ++d) g[d] = fmaf(cs, Xs[3 * i + d], fmaf(ct, Xt[3 * i + d], g[d]));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float v = wave_sum(g[d], lane);
    if (lane == 0) red[d][wave] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int d = threadIdx.x;
    grad_thetas[((long)b * slices + l) * 3 + d] =
        ((red[d][0] + red[d][1]) + (red[d][2] + red[d][3])) * slice_w[(long)b * slices + l];
  }
}

}  // namespace shw

extern "C" {

int shw_esw_forward(const float* xs, const float* xt, const float* thetas, int pairs, int n, int slices,
                    long theta_pair_stride, float p, float* slice_sum, float* coef_s, float* coef_t, void* stream) {
  if (!xs || !xt || !thetas || !slice_sum) return (int)hipErrorInvalidValue;
  if ((coef_s == nullptr) != (coef_t == nullptr)) return (int)hipErrorInvalidValue;
  if (!shw::euclid_sizes_ok(shw::kAnyPairs, pairs, n, n, 3, slices, theta_pair_stride) || !(p >= 1.f))
    return (int)hipErrorInvalidValue;
  if (pairs == 0 || slices == 0) return 0;
  shw::EswArgs A{};
  A.xs = xs; A.xt = xt; A.thetas = thetas; A.slice_sum = slice_sum; A.coef_s = coef_s; A.coef_t = coef_t;
  A.pairs = pairs; A.n = n; A.slices = slices; A.theta_pair_stride = theta_pair_stride;
  A.p = p; A.p_int = shw::small_integer_power(p);
  return shw::launch_euclid_forward<shw::EswKey::kRolledGeneralP>(
      (long)pairs * slices, n, A.p_int, coef_s != nullptr, A.num_groups,
      [&](auto ept, auto waves, auto pm, auto g, dim3 grid, dim3 block, size_t lds) {
        hipLaunchKernelGGL((shw::esw_kernel<decltype(ept)::value, decltype(waves)::value, decltype(pm)::value,
                                            decltype(g)::value>), grid, block, lds, (hipStream_t)stream, A);
      });
}

int shw_esw_backward_points(const float* thetas, const float* coef_s, const float* coef_t, const float* slice_w,
                            int pairs, int n, int slices, long theta_pair_stride, float* grad_xs, float* grad_xt,
                            void* stream) {
  if (!thetas || !coef_s || !coef_t || !slice_w || !grad_xs || !grad_xt) return (int)hipErrorInvalidValue;
  if (pairs < 0 || pairs > 65535 || slices < 0 || n < 1) return (int)hipErrorInvalidValue;
  if (pairs == 0) return 0;
  const int chunks = (n + 255) / 256;
  hipLaunchKernelGGL(shw::esw_backward_points_kernel, dim3(2 * chunks, pairs), dim3(256), 0, (hipStream_t)stream,
                     thetas, coef_s, coef_t, slice_w, n, slices, theta_pair_stride, grad_xs, grad_xt, chunks);
  return (int)hipGetLastError();
}

int shw_esw_backward_dirs(const float* xs, const float* xt, const float* coef_s, const float* coef_t,
                          const float* slice_w, int pairs, int n, int slices, float* grad_thetas, void* stream) {
  if (!xs || !xt || !coef_s || !coef_t || !slice_w || !grad_thetas) return (int)hipErrorInvalidValue;
  if (pairs < 0 || pairs > 65535 || slices < 0 || n < 1) return (int)hipErrorInvalidValue;
  if (pairs == 0 || slices == 0) return 0;
  hipLaunchKernelGGL(shw::esw_backward_dirs_kernel, dim3(slices, pairs), dim3(256), 0, (hipStream_t)stream, xs, xt,
                     coef_s, coef_t, slice_w, n, slices, grad_thetas);
  return (int)hipGetLastError();
}

}  // extern "C"
