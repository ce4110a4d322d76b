// shw_gsw.hip -- generalised sliced-Wasserstein: the sort-and-difference of the notebooks' GSWD / max-GSWD / DSWD family
// (Wasserstein_flow_problem/Flow_cube.ipynb, the cell that starts with `def rand_projections`) for keys that are not a
// dot product with a direction.  Two forms of one kernel, laid out as esw_dim_kernel (shw_esw_dim.hip): one wavefront per
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
#include "ssw_common.hpp"

namespace shw {

constexpr int kMaxGswDim = 64;

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

// r * theta[d] rounded on its own (the notebook forms theta * r first), never contracted into the subtraction
__device__ __forceinline__ float scaled_theta(float r, float t) { return __fmul_rn(r, t); }

// keys of one row of `count` caller-computed values; padding keys are +inf
template <int EPT>
__device__ __forceinline__ void load_row_keys(const float* __restrict__ U, int count, int lane, float (&key)[EPT]) {
#pragma unroll
  for (int j = 0; j < EPT; ++j) {
    const int i = j * kWave + lane;
    const float v = U[min(i, count - 1)];
    key[j] = i < count ? v : __builtin_inff();
  }
}

// circular keys of one cloud (count, dim) against the wave-uniform row T (scalar loads).  Chunks of CH points x DG
// coordinates in flight together, as the D-generic projection loader; coordinates past dim re-read the last one and are
// not used.  key = e0*e0, then fma(e_d, e_d, key) for d = 1..dim-1, e_d = x_d - (r t_d); then the square root.
template <int EPT>
__device__ __forceinline__ void load_circular_keys(const float* __restrict__ X, int count, int dim, int lane,
                                                   const float* __restrict__ T, float r, float (&key)[EPT]) {
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
          const float t = scaled_theta(r, T[d]);
#pragma unroll
          for (int j = 0; j < CH; ++j) {
            const float e = xv[j][k] - t;
            key[r0 + j] = (d == 0) ? e * e : fmaf(e, e, key[r0 + j]);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < CH; ++j)
      key[r0 + j] = ((r0 + j) * kWave + lane >= count) ? __builtin_inff() : sqrtf(key[r0 + j]);
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <int EPT, int WAVES, int PMODE, bool GRAD, bool CIRC>
__global__ __launch_bounds__(WAVES * 64) void gsw_kernel(GswArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int ROW = EPT * kWave;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* vbuf = lds + wave * ((PMODE == 2 ? 1 : 2) * (GRAD ? 2 : 1) * ROW);   // general p parks both operands
  int* vidx = reinterpret_cast<int*>(vbuf + ROW);            // GRAD only

  const int vid = xcd_contiguous_id(blockIdx.x, A.num_groups);
  const long s = (long)vid * WAVES + wave;
  if (s >= A.rows) return;
  const int n = A.n;
  const float* T = nullptr;
  long cloud = 0;                                            // circular: offset of the pair's clouds
  if constexpr (CIRC) {
    const int si = (int)s, b = si / A.slices, l = si - b * A.slices;   // pairs*slices fits an int (checked by the entry)
    T = A.thetas + (long)b * A.theta_pair_stride + (long)l * A.dim;
    cloud = (long)b * n * A.dim;
  }

  float u[EPT];
  int uidx[EPT];
#pragma nounroll
  for (int which = 0; which < 2; ++which) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
    if constexpr (CIRC) {
      load_circular_keys<EPT>((which == 0 ? A.b : A.a) + cloud, n, A.dim, ln, T, A.r, u);
    } else {
      load_row_keys<EPT>((which == 0 ? A.b : A.a) + s * n, n, ln, u);
    }
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
  float* ca = GRAD ? A.coef_a + s * n : nullptr;
  float* cb = GRAD ? A.coef_b + s * n : nullptr;
  // one sorted position: e = lane * EPT + r, the other operand's e sits in the same slot
  auto term = [&](int r, float uu, float v, int ia, int ib) {
    const float d = uu - v;
    if (lane * EPT + r < n) {
      acc += pow_abs<PMODE>(d, A.p, A.p_int);
      if constexpr (GRAD) {
        const float g = dpow_abs<PMODE>(d, A.p, A.p_int);
        // (a NaN key orders after the +inf pads and would put a pad's index here: such rows get no store past n)
        if constexpr (CIRC) {                                // coef / key; a point at r theta (key 0) contributes 0
          if (ia < n) ca[ia] = uu > 0.f ? g / uu : 0.f;
          if (ib < n) cb[ib] = v > 0.f ? -g / v : 0.f;
        } else {
          if (ia < n) ca[ia] = g;
          if (ib < n) cb[ib] = -g;
        }
      }
    }
  };
  if constexpr (PMODE == 2) {
#pragma unroll
    for (int r = 0; r < EPT; ++r)
      term(r, u[r], vbuf[r * kWave + lane], GRAD ? uidx[r] : 0, GRAD ? vidx[r * kWave + lane] : 0);
  } else {
    // general p: |d|^p is a loop or powf per key; unrolled EPT = 64 times it spills.  The sorted first operand goes to
    // LDS as well and one rolled loop walks both.
    float* ubuf = vbuf + (GRAD ? 2 : 1) * ROW;
    int* uixb = reinterpret_cast<int*>(ubuf + ROW);          // GRAD only
#pragma unroll
    for (int r = 0; r < EPT; ++r) {
      ubuf[r * kWave + lane] = u[r];
      if constexpr (GRAD) uixb[r * kWave + lane] = uidx[r];
    }
    __builtin_amdgcn_wave_barrier();
#pragma nounroll
    for (int r = 0; r < EPT; ++r)
      term(r, ubuf[r * kWave + lane], vbuf[r * kWave + lane], GRAD ? uixb[r * kWave + lane] : 0,
           GRAD ? vidx[r * kWave + lane] : 0);
  }
  acc = wave_sum(acc, lane);
  if (lane == 0) A.sums[s] = acc;
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

template <int EPT, int WAVES, bool CIRC>
static int launch_gsw(GswArgs& A, hipStream_t stream) {
  const long groups = (A.rows + WAVES - 1) / WAVES;
  if (groups > 0x7fffffffL) return (int)hipErrorInvalidValue;
  A.num_groups = (int)groups;
  const bool grad = A.coef_a != nullptr;
  const size_t lds = (size_t)WAVES * (A.p_int == 2 ? 1 : 2) * (grad ? 2 : 1) * EPT * kWave * sizeof(float);
  const dim3 grid((unsigned)groups), block(WAVES * 64);
  if (A.p_int == 2) {
    if (grad) hipLaunchKernelGGL((gsw_kernel<EPT, WAVES, 2, true, CIRC>), grid, block, lds, stream, A);
    else hipLaunchKernelGGL((gsw_kernel<EPT, WAVES, 2, false, CIRC>), grid, block, lds, stream, A);
  } else {
    if (grad) hipLaunchKernelGGL((gsw_kernel<EPT, WAVES, 0, true, CIRC>), grid, block, lds, stream, A);
    else hipLaunchKernelGGL((gsw_kernel<EPT, WAVES, 0, false, CIRC>), grid, block, lds, stream, A);
  }
  return (int)hipGetLastError();
}

template <bool CIRC>
static int launch_gsw_class(GswArgs& A, hipStream_t stream) {
  switch (ept_for(A.n, A.n)) {
    case 1: return launch_gsw<1, 4, CIRC>(A, stream);
    case 2: return launch_gsw<2, 4, CIRC>(A, stream);
    case 4: return launch_gsw<4, 4, CIRC>(A, stream);
    case 8: return launch_gsw<8, 4, CIRC>(A, stream);
    case 16: return launch_gsw<16, 4, CIRC>(A, stream);
    case 32: return launch_gsw<32, 2, CIRC>(A, stream);
    case 64: return launch_gsw<64, 1, CIRC>(A, stream);
    default: return (int)hipErrorInvalidValue;
  }
}

// coordinates per workgroup of the two gradient kernels: 4, 8, or 16 with the rest of dim split over blockIdx.z
inline int gsw_coord_chunk(int dim) { return dim <= 4 ? 4 : dim <= 8 ? 8 : 16; }

inline bool gsw_circular_sizes_ok(int pairs, int n, int dim, int slices, long theta_pair_stride) {
  if (dim < 1 || dim > kMaxGswDim) return false;
  if (pairs < 0 || slices < 0 || n < 1 || n > 4096) return false;
  if (theta_pair_stride != 0 && theta_pair_stride < (long)slices * dim) return false;
  return true;
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
  return shw::launch_gsw_class<false>(A, (hipStream_t)stream);
}

int shw_gsw_circular_forward(const float* xs, const float* xt, const float* thetas, int pairs, int n, int dim, int slices,
                             long theta_pair_stride, float r, float p, float* slice_sum, float* coef_s, float* coef_t,
                             void* stream) {
  if (!xs || !xt || !thetas || !slice_sum) return (int)hipErrorInvalidValue;
  if ((coef_s == nullptr) != (coef_t == nullptr)) return (int)hipErrorInvalidValue;
  if (!shw::gsw_circular_sizes_ok(pairs, n, dim, slices, theta_pair_stride) || !(p >= 1.f))
    return (int)hipErrorInvalidValue;
  if (pairs == 0 || slices == 0) return 0;
  if ((long)pairs * slices > 0x7fffffffL) return (int)hipErrorInvalidValue;
  shw::GswArgs A{};
  A.a = xs; A.b = xt; A.thetas = thetas; A.sums = slice_sum; A.coef_a = coef_s; A.coef_b = coef_t;
  A.rows = (long)pairs * slices; A.n = n; A.dim = dim; A.slices = slices; A.theta_pair_stride = theta_pair_stride;
  A.r = r; A.p = p; A.p_int = shw::small_integer_power(p);
  return shw::launch_gsw_class<true>(A, (hipStream_t)stream);
}

int shw_gsw_circular_backward_points(const float* xs, const float* xt, const float* thetas, const float* coef_s,
                                     const float* coef_t, const float* slice_w, int pairs, int n, int dim, int slices,
                                     long theta_pair_stride, float r, float* grad_xs, float* grad_xt, void* stream) {
  if (!xs || !xt || !thetas || !coef_s || !coef_t || !slice_w || !grad_xs || !grad_xt) return (int)hipErrorInvalidValue;
  if (!shw::gsw_circular_sizes_ok(pairs, n, dim, slices, theta_pair_stride) || pairs > 65535)
    return (int)hipErrorInvalidValue;
  if (pairs == 0) return 0;
  const int chunks = (n + 255) / 256;
  const int dc = shw::gsw_coord_chunk(dim);
  const dim3 grid(2 * chunks, pairs, (dim + dc - 1) / dc), block(256);
  const hipStream_t st = (hipStream_t)stream;
  switch (dc) {
    case 4:
      hipLaunchKernelGGL(shw::gsw_circular_backward_points_kernel<4>, grid, block, 0, st, xs, xt, thetas, coef_s, coef_t,
                         slice_w, n, dim, slices, theta_pair_stride, r, grad_xs, grad_xt, chunks);
      break;
    case 8:
      hipLaunchKernelGGL(shw::gsw_circular_backward_points_kernel<8>, grid, block, 0, st, xs, xt, thetas, coef_s, coef_t,
                         slice_w, n, dim, slices, theta_pair_stride, r, grad_xs, grad_xt, chunks);
      break;
    default:
      hipLaunchKernelGGL(shw::gsw_circular_backward_points_kernel<16>, grid, block, 0, st, xs, xt, thetas, coef_s, coef_t,
                         slice_w, n, dim, slices, theta_pair_stride, r, grad_xs, grad_xt, chunks);
  }
  return (int)hipGetLastError();
}

int shw_gsw_circular_backward_dirs(const float* xs, const float* xt, const float* thetas, const float* coef_s,
                                   const float* coef_t, const float* slice_w, int pairs, int n, int dim, int slices,
                                   long theta_pair_stride, float r, float* grad_thetas, void* stream) {
  if (!xs || !xt || !thetas || !coef_s || !coef_t || !slice_w || !grad_thetas) return (int)hipErrorInvalidValue;
  if (!shw::gsw_circular_sizes_ok(pairs, n, dim, slices, theta_pair_stride) || pairs > 65535)
    return (int)hipErrorInvalidValue;
  if (pairs == 0 || slices == 0) return 0;
  const int dc = shw::gsw_coord_chunk(dim);
  const dim3 grid(slices, pairs, (dim + dc - 1) / dc), block(256);
  const hipStream_t st = (hipStream_t)stream;
  switch (dc) {
    case 4:
      hipLaunchKernelGGL(shw::gsw_circular_backward_dirs_kernel<4>, grid, block, 0, st, xs, xt, thetas, coef_s, coef_t,
                         slice_w, n, dim, slices, theta_pair_stride, r, grad_thetas);
      break;
    case 8:
      hipLaunchKernelGGL(shw::gsw_circular_backward_dirs_kernel<8>, grid, block, 0, st, xs, xt, thetas, coef_s, coef_t,
                         slice_w, n, dim, slices, theta_pair_stride, r, grad_thetas);
      break;
    default:
      hipLaunchKernelGGL(shw::gsw_circular_backward_dirs_kernel<16>, grid, block, 0, st, xs, xt, thetas, coef_s, coef_t,
                         slice_w, n, dim, slices, theta_pair_stride, r, grad_thetas);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
