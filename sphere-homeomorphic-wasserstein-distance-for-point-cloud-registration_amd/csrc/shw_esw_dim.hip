// shw_esw_dim.hip -- Euclidean sliced-Wasserstein for points of any dimension D in 1..64 (the notebooks' ASWD
// baseline projects points augmented to 6 coordinates; `sliced_wasserstein_distance` reads its dimension from the
// clouds).  Same math as shw_esw.hip with D coordinates per point instead of 3: one wavefront per (pair, slice), the
// key of point i is sum_d x[i,d] * theta[l,d] accumulated in the order d = 0..D-1 (at D = 3 exactly the expression of
// shw_esw.hip), then the same register sort, sorted difference and coefficient rows.  The coefficient rows
// d S_l / d projection do not depend on D; only the projection and the two gradient kernels do.  The forward kernel is
// the shared body euclid_forward (euclid_common.hpp) with the D-generic projection as its key.
#include "euclid_common.hpp"   // load_projections_dim: the projection loader, shared with shw_line_ot.hip

namespace shw {

struct EswDimArgs {
  const float* xs;
  const float* xt;
  const float* thetas;     // (slices, dim) or (pairs, slices, dim)
  float* slice_sum;        // (pairs*slices)
  float* coef_s;           // optional (pairs*slices*n): d S_l / d projection, original point order
  float* coef_t;
  int pairs, n, dim, slices;
  long theta_pair_stride;  // 0 = shared
  float p;
  int p_int;
  int num_groups;
};

// the key of a point is its projection on the slice's direction row; the coefficient is the derivative itself
struct EswDimKey {
  static constexpr bool kRolledGeneralP = false;
  using row_t = int;       // pairs * slices, as the entry computes it
  const float *xs, *xt, *thetas;
  long theta_pair_stride;
  int dim, slices;
  const float* T;          // the slice's direction row
  long cloud;              // offset of the pair's clouds
  __device__ __forceinline__ void begin_row(int s, int n) {
    const int b = s / slices, l = s - b * slices;
    T = thetas + (long)b * theta_pair_stride + (long)l * dim;
    cloud = (long)b * n * dim;
  }
  template <int EPT>
  __device__ __forceinline__ void load(int which, int, int n, int lane, float (&key)[EPT]) const {
    load_projections_dim<EPT>((which == 0 ? xt : xs) + cloud, n, dim, lane, T, key);
  }
  template <bool NEG>
  static __device__ __forceinline__ float coef(float g, float) { return NEG ? -g : g; }
};

template <int EPT, int WAVES, int PMODE, bool GRAD>
__global__ __launch_bounds__(WAVES * 64) void esw_dim_kernel(EswDimArgs A) {
  euclid_forward<EPT, WAVES, PMODE, GRAD>(EswDimKey{A.xs, A.xt, A.thetas, A.theta_pair_stride, A.dim, A.slices},
                                          A.pairs * A.slices, A.n, A.num_groups, A.p, A.p_int, A.slice_sum,
                                          A.coef_s, A.coef_t);
}

// (the points gradient is line_esw_backward_points_kernel of shw_line_ot.hip with m = n: launch_line_esw_backward_points)

// grad_theta[b,l,d0+k] = w[b,l] * sum_i ( coef_s[b,l,i] * xs[b,i,d0+k] + coef_t[b,l,i] * xt[b,i,d0+k] ), k < DC:
// one workgroup per (slice, pair, coordinate chunk), each lane a strided run of points, then the fixed-order tree of
// shw_esw.hip (wave sums, then (w0 + w1) + (w2 + w3)).  No atomics: the result is the same bits on every run.
template <int DC>
__global__ __launch_bounds__(256) void esw_dim_backward_dirs_kernel(const float* __restrict__ xs,
                                                                    const float* __restrict__ xt,
                                                                    const float* __restrict__ coef_s,
                                                                    const float* __restrict__ coef_t,
                                                                    const float* __restrict__ slice_w, int n, int dim,
                                                                    int slices, float* __restrict__ grad_thetas) {
  __shared__ float red[DC][4];
  const int l = blockIdx.x, b = blockIdx.y;
  const int d0 = blockIdx.z * DC;
  const int last = dim - d0 - 1;
  const float* Xs = xs + (long)b * n * dim + d0;
  const float* Xt = xt + (long)b * n * dim + d0;
  const float* Cs = coef_s + ((long)b * slices + l) * n;
  const float* Ct = coef_t + ((long)b * slices + l) * n;
  float g[DC];
#pragma unroll
  for (int k = 0; k < DC; ++k) g[k] = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float cs = Cs[i], ct = Ct[i];
    const long row = (long)i * dim;
#pragma unroll
    for (int k = 0; k < DC; ++k) {
      const int kk = min(k, last);
      g[k] = fmaf(cs, Xs[row + kk], fmaf(ct, Xt[row + kk], g[k]));
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < DC; ++k) {
    const float v = wave_sum(g[k], lane);
    if (lane == 0) red[k][wave] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < DC && (int)threadIdx.x <= last) {
    const int k = threadIdx.x;
    grad_thetas[((long)b * slices + l) * dim + d0 + k] =
        ((red[k][0] + red[k][1]) + (red[k][2] + red[k][3])) * slice_w[(long)b * slices + l];
  }
}

}  // namespace shw

extern "C" {

int shw_esw_forward_dim(const float* xs, const float* xt, const float* thetas, int pairs, int n, int dim, int slices,
                        long theta_pair_stride, float p, float* slice_sum, float* coef_s, float* coef_t, void* stream) {
  if (!xs || !xt || !thetas || !slice_sum) return (int)hipErrorInvalidValue;
  if ((coef_s == nullptr) != (coef_t == nullptr)) return (int)hipErrorInvalidValue;
  if (!shw::euclid_sizes_ok(shw::kAnyPairs, pairs, n, n, dim, slices, theta_pair_stride) || !(p >= 1.f))
    return (int)hipErrorInvalidValue;
  if (pairs == 0 || slices == 0) return 0;
  shw::EswDimArgs A{};
  A.xs = xs; A.xt = xt; A.thetas = thetas; A.slice_sum = slice_sum; A.coef_s = coef_s; A.coef_t = coef_t;
  A.pairs = pairs; A.n = n; A.dim = dim; A.slices = slices; A.theta_pair_stride = theta_pair_stride;
  A.p = p; A.p_int = shw::small_integer_power(p);
  return shw::launch_euclid_forward<shw::EswDimKey::kRolledGeneralP>(
      (long)pairs * slices, n, A.p_int, coef_s != nullptr, A.num_groups,
      [&](auto ept, auto waves, auto pm, auto g, dim3 grid, dim3 block, size_t lds) {
        hipLaunchKernelGGL((shw::esw_dim_kernel<decltype(ept)::value, decltype(waves)::value, decltype(pm)::value,
                                                decltype(g)::value>), grid, block, lds, (hipStream_t)stream, A);
      });
}

int shw_esw_backward_points_dim(const float* thetas, const float* coef_s, const float* coef_t, const float* slice_w,
                                int pairs, int n, int dim, int slices, long theta_pair_stride, float* grad_xs,
                                float* grad_xt, void* stream) {
  if (!thetas || !coef_s || !coef_t || !slice_w || !grad_xs || !grad_xt) return (int)hipErrorInvalidValue;
  if (!shw::euclid_sizes_ok(shw::kGridYPairs, pairs, n, n, dim, slices, theta_pair_stride)) return (int)hipErrorInvalidValue;
  if (pairs == 0) return 0;
  return shw::launch_line_esw_backward_points(thetas, coef_s, coef_t, slice_w, pairs, n, n, dim, slices, theta_pair_stride,
                                              grad_xs, grad_xt, (hipStream_t)stream);
}

int shw_esw_backward_dirs_dim(const float* xs, const float* xt, const float* coef_s, const float* coef_t,
                              const float* slice_w, int pairs, int n, int dim, int slices, float* grad_thetas,
                              void* stream) {
  if (!xs || !xt || !coef_s || !coef_t || !slice_w || !grad_thetas) return (int)hipErrorInvalidValue;
  if (!shw::euclid_sizes_ok(shw::kGridYPairs, pairs, n, n, dim, slices, 0)) return (int)hipErrorInvalidValue;
  if (pairs == 0 || slices == 0) return 0;
  shw::with_coord_chunk(dim, [&](auto dc, unsigned z) {
    hipLaunchKernelGGL(shw::esw_dim_backward_dirs_kernel<decltype(dc)::value>, dim3(slices, pairs, z), dim3(256), 0,
                       (hipStream_t)stream, xs, xt, coef_s, coef_t, slice_w, n, dim, slices, grad_thetas);
  });
  return (int)hipGetLastError();
}

}  // extern "C"
