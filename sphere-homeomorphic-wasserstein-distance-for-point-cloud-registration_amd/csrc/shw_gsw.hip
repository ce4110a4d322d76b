// shw_gsw.hip -- generalised sliced-Wasserstein: the sort-and-difference of the notebooks' GSWD / max-GSWD / DSWD family
// (Wasserstein_flow_problem/Flow_cube.ipynb, the cell that starts with `def rand_projections`) for keys that are not a
// dot product with a direction.  Two forms of one kernel, a wrapper of euclid_forward (euclid_common.hpp): one wavefront per
// row, or per (pair, slice); 64 * EPT key slots, EPT = 1 .. 64 (up to 4096 points); +inf padding keys; the second
// operand's sorted keys (and indices) parked in LDS while the first sorts; a value-only instantiation that sorts bare
// keys and skips the index half.
//   rows      : the caller computed the keys (a network's output, any defining function): rows u, v of n keys each.
//   circular  : the key of point i on slice l is g(x_i, theta_l) = || x_i - r theta_l ||_2, formed in the kernel from the
//               differences x[i,d] - (r * theta[l,d]) accumulated in the order d = 0..dim-1 (never from the expansion
//               |x|^2 - 2 r x.theta + r^2 |theta|^2, which cancels when a point is near r theta).
// The circular form stores coef / key (0 where key == 0) as its coefficient rows: both gradients need the unit vector
// (x - r theta) / key, so the two gradient kernels read one number per (slice, point) and never recompute a key.  A point
// exactly at r theta therefore contributes gradient 0 where the notebook's autograd yields NaN (the one deliberate
// deviation).  Gradient sums run in a fixed order, no atomics: the same bits on every run.
#include "euclid_common.hpp"

namespace shw {

struct GswArgs {
  const float* a;          // rows: u (rows, n); circular: xs (pairs, n, dim)
  const float* b;          // rows: v;           circular: xt
  const float* thetas;     // circular only: (slices, dim) or (pairs, slices, dim)
  float* sums;             // (rows) or (pairs*slices)
  float* coef_a;           // optional, (rows*n) or (pairs*slices*n), original element order
  float* coef_b;
  long rows;               // rows, or pairs*slices
  int n, dim, slices;
  long theta_pair_stride;  // 0 = shared
  float r;
  float p;
  int p_int;
  int num_groups;
};

// rows: the key is the caller's, the coefficient the derivative itself.  circular: the key is || x - r theta ||, the
// coefficient coef / key; a point at r theta (key 0) contributes 0.
template <bool CIRC>
struct GswKey {
  static constexpr bool kRolledGeneralP = true;
  using row_t = long;      // rows form: the caller's row count
  const float *a, *b, *thetas;
  long theta_pair_stride;
  int dim, slices;
  float r;
  const float* T;          // circular: the slice's direction row
  long cloud;              // circular: offset of the pair's clouds
  __device__ __forceinline__ void begin_row(long s, int n) {
    if constexpr (CIRC) {
      const int si = (int)s, pair = si / slices, l = si - pair * slices;   // pairs*slices fits an int (checked by the entry)
      T = thetas + (long)pair * theta_pair_stride + (long)l * dim;
      cloud = (long)pair * n * dim;
    }
  }
  template <int EPT>
  __device__ __forceinline__ void load(int which, long s, int n, int lane, float (&key)[EPT]) const {
    if constexpr (CIRC) load_circular_keys<EPT>((which == 0 ? b : a) + cloud, n, dim, lane, T, r, key);
    else load_row_keys<EPT>((which == 0 ? b : a) + s * n, n, lane, key);
  }
  template <bool NEG>
  static __device__ __forceinline__ float coef(float g, float key) {
    if constexpr (CIRC) return key > 0.f ? (NEG ? -g / key : g / key) : 0.f;
    else return NEG ? -g : g;
  }
};

template <int EPT, int WAVES, int PMODE, bool GRAD, bool CIRC>
__global__ __launch_bounds__(WAVES * 64) void gsw_kernel(GswArgs A) {
  euclid_forward<EPT, WAVES, PMODE, GRAD>(GswKey<CIRC>{A.a, A.b, A.thetas, A.theta_pair_stride, A.dim, A.slices, A.r},
                                          A.rows, A.n, A.num_groups, A.p, A.p_int, A.sums, A.coef_a, A.coef_b);
}

// grad[b,i,d0+k] = sum_l w[b,l] * c'[b,l,i] * (x[b,i,d0+k] - r theta[b,l,d0+k]), c' = coef / key from the forward:
// one point per lane, DC coordinates per workgroup (blockIdx.z picks the chunk), slices in the order l = 0..slices-1.
// Coordinates past dim re-read the last one and are not stored.
template <int DC>
__global__ __launch_bounds__(256) void gsw_circular_backward_points_kernel(
    const float* __restrict__ xs, const float* __restrict__ xt, const float* __restrict__ thetas,
    const float* __restrict__ coef_s, const float* __restrict__ coef_t, const float* __restrict__ slice_w, int n, int dim,
    int slices, long theta_pair_stride, float r, float* __restrict__ grad_xs, float* __restrict__ grad_xt, int chunks) {
  const int b = blockIdx.y;
  const int d0 = blockIdx.z * DC;
  const bool is_t = (int)blockIdx.x >= chunks;
  const int chunk = is_t ? blockIdx.x - chunks : blockIdx.x;
  const int i = chunk * 256 + threadIdx.x;
  const int ic = min(i, n - 1);
  const int last = dim - d0 - 1;
  const float* C = (is_t ? coef_t : coef_s) + (long)b * slices * n;
  const float* X = (is_t ? xt : xs) + ((long)b * n + ic) * dim + d0;
  float* G = (is_t ? grad_xt : grad_xs) + (long)b * n * dim + d0;
  const float* Tb = thetas + (long)b * theta_pair_stride + d0;
  const float* W = slice_w + (long)b * slices;
  float x[DC], g[DC];
#pragma unroll
  for (int k = 0; k < DC; ++k) {
    x[k] = X[min(k, last)];
    g[k] = 0.f;
  }
  for (int l = 0; l < slices; ++l) {
    const float c = C[(long)l * n + ic] * W[l];
    const float* Tl = Tb + (long)l * dim;
#pragma unroll
    for (int k = 0; k < DC; ++k) g[k] = fmaf(c, x[k] - scaled_theta(r, Tl[min(k, last)]), g[k]);
  }
  if (i < n) {
#pragma unroll
    for (int k = 0; k < DC; ++k)
      if (k <= last) G[(long)i * dim + k] = g[k];
  }
}

// grad_theta[b,l,d0+k] = -r w[b,l] sum_i ( c's[b,l,i] (xs[b,i,d0+k] - r theta) + c't[b,l,i] (xt[b,i,d0+k] - r theta) ):
// one workgroup per (slice, pair, coordinate chunk), each lane a strided run of points, then wave sums and
// (w0 + w1) + (w2 + w3), the fixed-order tree of the Euclidean direction gradient.
template <int DC>
__global__ __launch_bounds__(256) void gsw_circular_backward_dirs_kernel(
    const float* __restrict__ xs, const float* __restrict__ xt, const float* __restrict__ thetas,
    const float* __restrict__ coef_s, const float* __restrict__ coef_t, const float* __restrict__ slice_w, int n, int dim,
    int slices, long theta_pair_stride, float r, float* __restrict__ grad_thetas) {
  __shared__ float red[DC][4];
  const int l = blockIdx.x, b = blockIdx.y;
  const int d0 = blockIdx.z * DC;
  const int last = dim - d0 - 1;
  const float* Xs = xs + (long)b * n * dim + d0;
  const float* Xt = xt + (long)b * n * dim + d0;
  const float* Cs = coef_s + ((long)b * slices + l) * n;
  const float* Ct = coef_t + ((long)b * slices + l) * n;
  const float* Tl = thetas + (long)b * theta_pair_stride + (long)l * dim + d0;
  float t[DC], g[DC];
#pragma unroll
  for (int k = 0; k < DC; ++k) {
    t[k] = scaled_theta(r, Tl[min(k, last)]);
    g[k] = 0.f;
  }
  for (int i = threadIdx.x; i < n; i += 256) {
    const float cs = Cs[i], ct = Ct[i];
    const long row = (long)i * dim;
#pragma unroll
    for (int k = 0; k < DC; ++k) {
      const int kk = min(k, last);
      g[k] = fmaf(cs, Xs[row + kk] - t[k], fmaf(ct, Xt[row + kk] - t[k], g[k]));
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
        ((red[k][0] + red[k][1]) + (red[k][2] + red[k][3])) * (-r * slice_w[(long)b * slices + l]);
  }
}

template <bool CIRC>
static int launch_gsw(GswArgs& A, hipStream_t stream) {
  return launch_euclid_forward<GswKey<CIRC>::kRolledGeneralP>(
      A.rows, A.n, A.p_int, A.coef_a != nullptr, A.num_groups,
      [&](auto ept, auto waves, auto pm, auto g, dim3 grid, dim3 block, size_t lds) {
        hipLaunchKernelGGL((gsw_kernel<decltype(ept)::value, decltype(waves)::value, decltype(pm)::value,
                                       decltype(g)::value, CIRC>), grid, block, lds, stream, A);
      });
}

}  // namespace shw

extern "C" {

int shw_gsw_rows_forward(const float* u, const float* v, long rows, int n, float p, float* row_sum, float* coef_u,
                         float* coef_v, void* stream) {
  if (!u || !v || !row_sum) return (int)hipErrorInvalidValue;
  if ((coef_u == nullptr) != (coef_v == nullptr)) return (int)hipErrorInvalidValue;
  if (rows < 0 || n < 1 || n > 4096 || !(p >= 1.f)) return (int)hipErrorInvalidValue;
  if (rows == 0) return 0;
  shw::GswArgs A{};
  A.a = u; A.b = v; A.sums = row_sum; A.coef_a = coef_u; A.coef_b = coef_v;
  A.rows = rows; A.n = n; A.dim = 1; A.slices = 1;
  A.p = p; A.p_int = shw::small_integer_power(p);
  return shw::launch_gsw<false>(A, (hipStream_t)stream);
}

int shw_gsw_circular_forward(const float* xs, const float* xt, const float* thetas, int pairs, int n, int dim, int slices,
                             long theta_pair_stride, float r, float p, float* slice_sum, float* coef_s, float* coef_t,
                             void* stream) {
  if (!xs || !xt || !thetas || !slice_sum) return (int)hipErrorInvalidValue;
  if ((coef_s == nullptr) != (coef_t == nullptr)) return (int)hipErrorInvalidValue;
  if (!shw::euclid_sizes_ok(shw::kAnyPairs, pairs, n, n, dim, slices, theta_pair_stride) || !(p >= 1.f))
    return (int)hipErrorInvalidValue;
  if (pairs == 0 || slices == 0) return 0;
  if ((long)pairs * slices > 0x7fffffffL) return (int)hipErrorInvalidValue;
  shw::GswArgs A{};
  A.a = xs; A.b = xt; A.thetas = thetas; A.sums = slice_sum; A.coef_a = coef_s; A.coef_b = coef_t;
  A.rows = (long)pairs * slices; A.n = n; A.dim = dim; A.slices = slices; A.theta_pair_stride = theta_pair_stride;
  A.r = r; A.p = p; A.p_int = shw::small_integer_power(p);
  return shw::launch_gsw<true>(A, (hipStream_t)stream);
}

int shw_gsw_circular_backward_points(const float* xs, const float* xt, const float* thetas, const float* coef_s,
                                     const float* coef_t, const float* slice_w, int pairs, int n, int dim, int slices,
                                     long theta_pair_stride, float r, float* grad_xs, float* grad_xt, void* stream) {
  if (!xs || !xt || !thetas || !coef_s || !coef_t || !slice_w || !grad_xs || !grad_xt) return (int)hipErrorInvalidValue;
  if (!shw::euclid_sizes_ok(shw::kGridYPairs, pairs, n, n, dim, slices, theta_pair_stride)) return (int)hipErrorInvalidValue;
  if (pairs == 0) return 0;
  const int chunks = (n + 255) / 256;
  shw::with_coord_chunk(dim, [&](auto dc, unsigned z) {
    hipLaunchKernelGGL(shw::gsw_circular_backward_points_kernel<decltype(dc)::value>, dim3(2 * chunks, pairs, z), dim3(256),
                       0, (hipStream_t)stream, xs, xt, thetas, coef_s, coef_t, slice_w, n, dim, slices, theta_pair_stride,
                       r, grad_xs, grad_xt, chunks);
  });
  return (int)hipGetLastError();
}

int shw_gsw_circular_backward_dirs(const float* xs, const float* xt, const float* thetas, const float* coef_s,
                                   const float* coef_t, const float* slice_w, int pairs, int n, int dim, int slices,
                                   long theta_pair_stride, float r, float* grad_thetas, void* stream) {
  if (!xs || !xt || !thetas || !coef_s || !coef_t || !slice_w || !grad_thetas) return (int)hipErrorInvalidValue;
  if (!shw::euclid_sizes_ok(shw::kGridYPairs, pairs, n, n, dim, slices, theta_pair_stride)) return (int)hipErrorInvalidValue;
  if (pairs == 0 || slices == 0) return 0;
  shw::with_coord_chunk(dim, [&](auto dc, unsigned z) {
    hipLaunchKernelGGL(shw::gsw_circular_backward_dirs_kernel<decltype(dc)::value>, dim3(slices, pairs, z), dim3(256), 0,
                       (hipStream_t)stream, xs, xt, thetas, coef_s, coef_t, slice_w, n, dim, slices, theta_pair_stride, r,
                       grad_thetas);
  });
  return (int)hipGetLastError();
}

}  // extern "C"
