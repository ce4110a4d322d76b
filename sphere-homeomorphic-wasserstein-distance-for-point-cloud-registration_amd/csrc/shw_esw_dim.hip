// shw_esw_dim.hip -- Euclidean sliced-Wasserstein for points of any dimension D in 1..64 (the notebooks' ASWD
// baseline projects points augmented to 6 coordinates; `sliced_wasserstein_distance` reads its dimension from the
// clouds).  Same math as shw_esw.hip with D coordinates per point instead of 3: one wavefront per (pair, slice), the
// key of point i is sum_d x[i,d] * theta[l,d] accumulated in the order d = 0..D-1 (at D = 3 exactly the expression of
// shw_esw.hip), then the same register sort, sorted difference and coefficient rows.  The coefficient rows
// d S_l / d projection do not depend on D; only the projection and the two gradient kernels do.
#include "esw_project.hpp"   // load_projections_dim: the projection loader, shared with shw_line_ot.hip

namespace shw {

constexpr int kMaxEswDim = 64;

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

template <int EPT, int WAVES, int PMODE, bool GRAD>
__global__ __launch_bounds__(WAVES * 64) void esw_dim_kernel(EswDimArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int ROW = EPT * kWave;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* vbuf = lds + wave * ((GRAD ? 2 : 1) * ROW);
  int* vidx = reinterpret_cast<int*>(vbuf + ROW);            // GRAD only

  const int vid = xcd_contiguous_id(blockIdx.x, A.num_groups);
  const int s = vid * WAVES + wave;
  if (s >= A.pairs * A.slices) return;
  const int b = s / A.slices, l = s - b * A.slices;
  const int n = A.n, dim = A.dim;
  const float* T = A.thetas + (long)b * A.theta_pair_stride + (long)l * dim;

  float u[EPT];
  int uidx[EPT];
#pragma nounroll
  for (int which = 0; which < 2; ++which) {
    const float* X = (which == 0 ? A.xt : A.xs) + (long)b * n * dim;
    int ln = lane;
    asm volatile("" : "+v"(ln));
    load_projections_dim<EPT>(X, n, dim, ln, T, u);
    if constexpr (GRAD) {
      item_t item[EPT];
#pragma unroll
      for (int r = 0; r < EPT; ++r) item[r] = make_item(orderable(u[r]), r * kWave + ln);
      wave_sort_kv<EPT>(item, ln);
#pragma unroll
      for (int r = 0; r < EPT; ++r) {
        u[r] = from_orderable(item_key(item[r]));
        uidx[r] = item_idx(item[r]);
      }
    } else {
      wave_sort<EPT>(u, ln);
    }
    if (which == 0) {
#pragma unroll
      for (int r = 0; r < EPT; ++r) {
        vbuf[r * kWave + lane] = u[r];
        if constexpr (GRAD) vidx[r * kWave + lane] = uidx[r];
      }
    }
  }
  __builtin_amdgcn_wave_barrier();

  float acc = 0.f;
  float* cs = GRAD ? A.coef_s + (long)s * n : nullptr;
  float* ct = GRAD ? A.coef_t + (long)s * n : nullptr;
#pragma unroll
  for (int r = 0; r < EPT; ++r) {
    const int e = lane * EPT + r;                            // sorted position; target e sits in the same slot
    const float d = u[r] - vbuf[r * kWave + lane];
    if (e < n) {
      acc += pow_abs<PMODE>(d, A.p, A.p_int);
      if constexpr (GRAD) {
        const float g = dpow_abs<PMODE>(d, A.p, A.p_int);
        cs[uidx[r]] = g;
        ct[vidx[r * kWave + lane]] = -g;
      }
    }
  }
  acc = wave_sum(acc, lane);
  if (lane == 0) A.slice_sum[s] = acc;
}

// grad[b,i,d0+k] = sum_l w[b,l] * coef[b,l,i] * theta[b,l,d0+k], k < DC: one point per lane, DC coordinates per
// workgroup (blockIdx.z picks the chunk, so D > 16 splits over the grid instead of spilling).  Coordinates past D
// re-read the last one and are not stored.
template <int DC>
__global__ __launch_bounds__(256) void esw_dim_backward_points_kernel(const float* __restrict__ thetas,
                                                                      const float* __restrict__ coef_s,
                                                                      const float* __restrict__ coef_t,
                                                                      const float* __restrict__ slice_w, int n,
                                                                      int dim, int slices, long theta_pair_stride,
                                                                      float* __restrict__ grad_xs,
                                                                      float* __restrict__ grad_xt, int chunks) {
  const int b = blockIdx.y;
  const int d0 = blockIdx.z * DC;
  const bool is_t = (int)blockIdx.x >= chunks;
  const int chunk = is_t ? blockIdx.x - chunks : blockIdx.x;
  const int i = chunk * 256 + threadIdx.x;
  const int ic = min(i, n - 1);
  const int last = dim - d0 - 1;
  const float* C = (is_t ? coef_t : coef_s) + (long)b * slices * n;
  float* G = (is_t ? grad_xt : grad_xs) + (long)b * n * dim + d0;
  const float* Tb = thetas + (long)b * theta_pair_stride + d0;
  const float* W = slice_w + (long)b * slices;
  float g[DC];
#pragma unroll
  for (int k = 0; k < DC; ++k) g[k] = 0.f;
  for (int l = 0; l < slices; ++l) {
    const float c = C[(long)l * n + ic] * W[l];
    const float* Tl = Tb + (long)l * dim;
#pragma unroll
    for (int k = 0; k < DC; ++k) g[k] = fmaf(c, Tl[min(k, last)], g[k]);
  }
  if (i < n) {
#pragma unroll
    for (int k = 0; k < DC; ++k)
      if (k <= last) G[(long)i * dim + k] = g[k];
  }
}

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

template <int EPT, int WAVES>
static int launch_esw_dim(EswDimArgs& A, hipStream_t stream) {
  const long total = (long)A.pairs * A.slices;
  const long groups = (total + WAVES - 1) / WAVES;
  if (groups > 0x7fffffffL) return (int)hipErrorInvalidValue;
  A.num_groups = (int)groups;
  const bool grad = A.coef_s != nullptr;
  const size_t lds = (size_t)WAVES * (grad ? 2 : 1) * EPT * kWave * sizeof(float);
  const dim3 grid((unsigned)groups), block(WAVES * 64);
  if (A.p_int == 2) {
    if (grad) hipLaunchKernelGGL((esw_dim_kernel<EPT, WAVES, 2, true>), grid, block, lds, stream, A);
    else hipLaunchKernelGGL((esw_dim_kernel<EPT, WAVES, 2, false>), grid, block, lds, stream, A);
  } else {
    if (grad) hipLaunchKernelGGL((esw_dim_kernel<EPT, WAVES, 0, true>), grid, block, lds, stream, A);
    else hipLaunchKernelGGL((esw_dim_kernel<EPT, WAVES, 0, false>), grid, block, lds, stream, A);
  }
  return (int)hipGetLastError();
}

// coordinates per workgroup of the two gradient kernels: 4, 8, or 16 with the rest of D split over blockIdx.z
inline int coord_chunk(int dim) { return dim <= 4 ? 4 : dim <= 8 ? 8 : 16; }

}  // namespace shw

extern "C" {

int shw_esw_forward_dim(const float* xs, const float* xt, const float* thetas, int pairs, int n, int dim, int slices,
                        long theta_pair_stride, float p, float* slice_sum, float* coef_s, float* coef_t, void* stream) {
  if (!xs || !xt || !thetas || !slice_sum) return (int)hipErrorInvalidValue;
  if ((coef_s == nullptr) != (coef_t == nullptr)) return (int)hipErrorInvalidValue;
  if (dim < 1 || dim > shw::kMaxEswDim) return (int)hipErrorInvalidValue;
  if (pairs < 0 || slices < 0 || n < 1 || n > 4096 || !(p >= 1.f)) return (int)hipErrorInvalidValue;
  if (theta_pair_stride != 0 && theta_pair_stride < (long)slices * dim) return (int)hipErrorInvalidValue;
  if (pairs == 0 || slices == 0) return 0;
  shw::EswDimArgs A{};
  A.xs = xs; A.xt = xt; A.thetas = thetas; A.slice_sum = slice_sum; A.coef_s = coef_s; A.coef_t = coef_t;
  A.pairs = pairs; A.n = n; A.dim = dim; A.slices = slices; A.theta_pair_stride = theta_pair_stride;
  A.p = p; A.p_int = shw::small_integer_power(p);
  if (p == 1.f) A.p_int = 1;
  switch (shw::ept_for(n, n)) {
    case 1: return shw::launch_esw_dim<1, 4>(A, (hipStream_t)stream);
    case 2: return shw::launch_esw_dim<2, 4>(A, (hipStream_t)stream);
    case 4: return shw::launch_esw_dim<4, 4>(A, (hipStream_t)stream);
    case 8: return shw::launch_esw_dim<8, 4>(A, (hipStream_t)stream);
    case 16: return shw::launch_esw_dim<16, 4>(A, (hipStream_t)stream);
    case 32: return shw::launch_esw_dim<32, 2>(A, (hipStream_t)stream);
    case 64: return shw::launch_esw_dim<64, 1>(A, (hipStream_t)stream);
    default: return (int)hipErrorInvalidValue;
  }
}

int shw_esw_backward_points_dim(const float* thetas, const float* coef_s, const float* coef_t, const float* slice_w,
                                int pairs, int n, int dim, int slices, long theta_pair_stride, float* grad_xs,
                                float* grad_xt, void* stream) {
  if (!thetas || !coef_s || !coef_t || !slice_w || !grad_xs || !grad_xt) return (int)hipErrorInvalidValue;
  if (dim < 1 || dim > shw::kMaxEswDim) return (int)hipErrorInvalidValue;
  if (pairs < 0 || pairs > 65535 || slices < 0 || n < 1 || n > 4096) return (int)hipErrorInvalidValue;
  if (theta_pair_stride != 0 && theta_pair_stride < (long)slices * dim) return (int)hipErrorInvalidValue;
  if (pairs == 0) return 0;
  const int chunks = (n + 255) / 256;
  const int dc = shw::coord_chunk(dim);
  const dim3 grid(2 * chunks, pairs, (dim + dc - 1) / dc), block(256);
  const hipStream_t st = (hipStream_t)stream;
  switch (dc) {
    case 4:
      hipLaunchKernelGGL(shw::esw_dim_backward_points_kernel<4>, grid, block, 0, st, thetas, coef_s, coef_t, slice_w, n,
                         dim, slices, theta_pair_stride, grad_xs, grad_xt, chunks);
      break;
    case 8:
      hipLaunchKernelGGL(shw::esw_dim_backward_points_kernel<8>, grid, block, 0, st, thetas, coef_s, coef_t, slice_w, n,
                         dim, slices, theta_pair_stride, grad_xs, grad_xt, chunks);
      break;
    default:
      hipLaunchKernelGGL(shw::esw_dim_backward_points_kernel<16>, grid, block, 0, st, thetas, coef_s, coef_t, slice_w,
                         n, dim, slices, theta_pair_stride, grad_xs, grad_xt, chunks);
  }
  return (int)hipGetLastError();
}

int shw_esw_backward_dirs_dim(const float* xs, const float* xt, const float* coef_s, const float* coef_t,
                              const float* slice_w, int pairs, int n, int dim, int slices, float* grad_thetas,
                              void* stream) {
  if (!xs || !xt || !coef_s || !coef_t || !slice_w || !grad_thetas) return (int)hipErrorInvalidValue;
  if (dim < 1 || dim > shw::kMaxEswDim) return (int)hipErrorInvalidValue;
  if (pairs < 0 || pairs > 65535 || slices < 0 || n < 1 || n > 4096) return (int)hipErrorInvalidValue;
  if (pairs == 0 || slices == 0) return 0;
  const int dc = shw::coord_chunk(dim);
  const dim3 grid(slices, pairs, (dim + dc - 1) / dc), block(256);
  const hipStream_t st = (hipStream_t)stream;
  switch (dc) {
    case 4:
      hipLaunchKernelGGL(shw::esw_dim_backward_dirs_kernel<4>, grid, block, 0, st, xs, xt, coef_s, coef_t, slice_w, n,
                         dim, slices, grad_thetas);
      break;
    case 8:
      hipLaunchKernelGGL(shw::esw_dim_backward_dirs_kernel<8>, grid, block, 0, st, xs, xt, coef_s, coef_t, slice_w, n,
                         dim, slices, grad_thetas);
      break;
    default:
      hipLaunchKernelGGL(shw::esw_dim_backward_dirs_kernel<16>, grid, block, 0, st, xs, xt, coef_s, coef_t, slice_w, n,
                         dim, slices, grad_thetas);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
