// shw_ssw_f64.hip -- float64 path of the spherical sliced-Wasserstein loss for MI355X (gfx950): equal cloud sizes,
// uniform weights, any p >= 1, loss and training form, sliced level and circle level.
//
// Reference being replaced (paths relative to /root/reference/Point_Cloud_Resistration/losses/): the same functions as
// the float32 units -- sliced_cost (max_spherical_sliced_w.py:251-286, _fast.py:258-295), binary_search_circle
// (:117-207), emd1D_circle (:210-247) -- when the caller's tensors are double (`dtype = u_values.dtype`, :153-160).
//
// Weighted and unequal-size double clouds are shw_ssw_f64_general.hip; the device helpers both units use (reductions,
// |d|^p, circle coordinate, searches, the project-and-sort stage of one cloud) are f64_common.hpp.
// This unit shares no kernel with the float32 path: those are tuned to the 32-bit word (registers per key, packed
// (key, index) items, the degree-15 arctangent) and stay as they are.  Here ONE WORKGROUP owns one (pair, slice):
//   1. projection (a, b) = U^T x as an FMA chain from +0 and coord = (atan2(-b, -a) + pi) / (2 pi) with the device
//      library's double atan2 (an all-zero point gives atan2(-0, -0) = -pi, coordinate 0, as in the reference :274-279);
//   2. each cloud sorted in LDS into the total order (ascending coordinate, ties by original index), the 16-bit index
//      array travelling beside the 64-bit keys: a distribution sort over P equal bins of [0, 1] (count with integer
//      LDS counters, scan, scatter, then every bin put in order by insertion -- the result is the total order whatever
//      order the counters served the atoms in); a cloud with more than 24 atoms in one bin (bunched or duplicated
//      points) is sorted by a bitonic network over (coordinate, index) instead;
//   3. p != 1 (and binary_search_circle at p = 1): min over |k| <= n of c(k) = (1/n) sum_i |u_(i) - v_ext(i + k)|^p by
//      the convex search of solve_shift (ssw_common.hpp): start at round(sum u - sum v), gallop, bisect;
//      p == 1 at the sliced level and emd1D_circle: the level-median formula with the reference's omitted wrap segment,
//      levels kept as exact integers (#u - #v, n = m), every atom placed in the other cloud by binary search;
//   4. training form: d cost / d coordinate, written to the row of the slice at the ORIGINAL point index.
// Every sum runs in a fixed order (per-thread strided partial sums, a butterfly over the lanes, the waves in order):
// results are bit-identical from run to run.  No floating-point atomics.
//
// LDS per workgroup, P = next power of two >= n: two sorted clouds 16 P, their permutations 4 P, one cloud in original
// order 8 P, the bins 4 P, and 840 bytes of scratch: 128.8 KiB at n = 4096 (SHW_MAX_POINTS_F64).  The two sorted clouds
// of 8192 doubles with their permutations alone are exactly 160 KiB, hence the limit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/shw.h"
#include "dispatch.hpp"      // host launch helpers only: no device code is shared with the float32 units
#include "f64_common.hpp"    // reductions, |d|^p, circle coordinate, searches, the project-and-sort stage

namespace shw {
namespace f64 {

constexpr int kItems = 4;            // sorted positions per thread and cloud: the workgroup has max(64, P / 4) threads
constexpr int kFixedLds = 6 * kMaxWaves * 8 + (kMaxWaves + 2) * 4;   // reduction scratch, scan totals, flags

struct Args {
  const double* xs;
  const double* xt;
  const double* dirs;                // NULL: rows of circle coordinates (shw_circle_ot_f64), one double per atom
  double* slice_cost;
  int32_t* slice_aux;                // shift k* or median level, may be NULL
  double* coef_s;                    // both NULL: loss only
  double* coef_t;
  int pairs, n, slices, P;
  long u_pair_stride;
  int pstride;                       // doubles per atom in xs / xt: 3 (points) or 1 (coordinates)
  double p;
  int p_int;                         // p as a small integer (1..8), else 0
};

// v_ext(q) = v[q mod n] + floor(q / n) for q in [-2n, 3n)
__device__ __forceinline__ double target_ext(const double* sv, int q, int n, int* at = nullptr) {
  double turn = 0.0;
  if (q < 0) { q += n; turn -= 1.0; }
  if (q < 0) { q += n; turn -= 1.0; }
  if (q >= n) { q -= n; turn += 1.0; }
  if (q >= n) { q -= n; turn += 1.0; }
  if (at) *at = q;
  return sv[q] + turn;
}

// LEVEL_MEDIAN false: min_k c(k) (any p >= 1).  true: the p = 1 level-median formula.
template <bool LEVEL_MEDIAN>
__global__ __launch_bounds__(1024) void ssw_f64_kernel(Args A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int P = A.P, n = A.n, T = blockDim.x, t = threadIdx.x;
  const int nwaves = T >> 6;
  double* su = reinterpret_cast<double*>(lds_raw);      // sorted source coordinates, then [P, 2P) the target's
  double* sv = su + P;
  double* tmp = sv + P;                                 // a cloud's coordinates in original order
  double* red = tmp + P;                                // 2 x 3 x kMaxWaves
  unsigned* hist = reinterpret_cast<unsigned*>(red + 6 * kMaxWaves);   // P bins: counts, starts, ends
  unsigned* wsum = hist + P;                            // kMaxWaves wave totals of the scan
  unsigned* flags = wsum + kMaxWaves;                   // per cloud: sort with the network
  uint16_t* pu = reinterpret_cast<uint16_t*>(flags + 2);   // original index of every sorted position
  uint16_t* pv = pu + P;
  int turn = 0;

  const long s = blockIdx.x;
  const int b = (int)(s / A.slices), l = (int)(s - (long)b * A.slices);

  // ---- 1. + 2. circle coordinates of a cloud, then its sort, the source first ---------------------------------
  double U[6];
  if (A.dirs) {
    const double* Ul = A.dirs + (long)b * A.u_pair_stride + (long)l * 6;
#pragma unroll
    for (int i = 0; i < 6; ++i) U[i] = Ul[i];
  }
  if (t < 2) flags[t] = 0;
  double acc_u = 0.0, acc_v = 0.0, unused = 0.0;
  for (int which = 0; which < 2; ++which) {
    const double* X = (which ? A.xt : A.xs) + (long)b * n * A.pstride;
    const double acc = project_and_sort(X, n, P, U, A.dirs != nullptr, which ? sv : su, which ? pv : pu, tmp, hist, wsum,
                                        flags + which, t, T);
    if (which) acc_v = acc; else acc_u = acc;
  }

  double* cs = A.coef_s ? A.coef_s + s * n : nullptr;
  double* ct = A.coef_t ? A.coef_t + s * n : nullptr;

  if constexpr (!LEVEL_MEDIAN) {
    // ---- 3a. convex search over the shift --------------------------------------------------------
    block_sum3(acc_u, acc_v, unused, red, turn, nwaves);
    int lo = -n, hi = n;
    double guess = rint(acc_u - acc_v);
    guess = fmin(fmax(guess, (double)lo), (double)hi);
    int k = (guess == guess) ? (int)guess : 0;
    bool lo_tight = false, hi_tight = false;
    int step = 1;
    double cm = 0.0, c0 = 0.0, cp = 0.0;
    // every iteration removes k from [lo, hi]; the cap only guards against non-finite input
    for (int it = 0; it < 64; ++it) {
      cm = 0.0; c0 = 0.0; cp = 0.0;
      for (int i = t; i < n; i += T) {
        const double u = su[i];
        cm += pow_abs(u - target_ext(sv, i + k - 1, n), A.p, A.p_int);
        c0 += pow_abs(u - target_ext(sv, i + k, n), A.p, A.p_int);
        cp += pow_abs(u - target_ext(sv, i + k + 1, n), A.p, A.p_int);
      }
      block_sum3(cm, c0, cp, red, turn, nwaves);
      const bool right = (cp < c0) && (k < hi);
      const bool left = !right && (cm < c0) && (k > lo);
      if (!right && !left) break;
      if (right) {
        lo = k + 1;
        lo_tight = true;
        if (hi_tight) { k = lo + ((hi - lo) >> 1); }
        else { k = min(k + step, hi); step <<= 1; }
      } else {
        hi = k - 1;
        hi_tight = true;
        if (lo_tight) { k = lo + ((hi - lo) >> 1); }
        else { k = max(k - step, lo); step <<= 1; }
      }
    }
    if (t == 0) {
      A.slice_cost[s] = c0 / (double)n;
      if (A.slice_aux) A.slice_aux[s] = k;
    }
    if (cs) {
      const double inv_n = 1.0 / (double)n;
      for (int i = t; i < n; i += T) {
        int q;
        const double d = su[i] - target_ext(sv, i + k, n, &q);
        const double g = dpow_abs(d, A.p, A.p_int) * inv_n;
        // i -> q is a bijection: every row entry written once (the index tests only matter for NaN input, whose order
        // the network does not define: a pad's index must never become an address)
        if (pu[i] < n) cs[pu[i]] = g;
        if (pv[q] < n) ct[pv[q]] = -g;
      }
    }
  } else {
    // ---- 3b. level median (p = 1), n = m: level numerator = #u - #v, level = num / n ----------------
    // index j < kItems: source atom at sorted position t + j T; kItems + j: target atom at that position
    int num[2 * kItems];
    double gap[2 * kItems];
    int lo_num = 0x7fffffff, hi_num = -0x7fffffff;
    double w = 0.0;
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
      const int e = t + j * T;
      const bool live = e < n;
      const int ec = live ? e : 0;
      {  // source atom: successor in the merged order (u before v on equal values) = min(u_(e+1), v_lb)
        const double val = su[ec];
        const int lb = count_below<true>(sv, n, val);
        const double a = (ec + 1 < n) ? su[ec + 1] : __builtin_inf();
        const double bb = (lb < n) ? sv[lb] : __builtin_inf();
        const double nxt = fmin(a, bb);
        gap[j] = live ? ((nxt == __builtin_inf()) ? 1.0 : nxt) - val : 0.0;   // last merged atom: up to 1 (:237)
        num[j] = (ec + 1) - lb;
      }
      {  // target atom
        const double val = sv[ec];
        const int ub = count_below<false>(su, n, val);
        const double a = (ec + 1 < n) ? sv[ec + 1] : __builtin_inf();
        const double bb = (ub < n) ? su[ub] : __builtin_inf();
        const double nxt = fmin(a, bb);
        gap[kItems + j] = live ? ((nxt == __builtin_inf()) ? 1.0 : nxt) - val : 0.0;
        num[kItems + j] = ub - (ec + 1);
      }
      if (live) {
        lo_num = min(lo_num, min(num[j], num[kItems + j]));
        hi_num = max(hi_num, max(num[j], num[kItems + j]));
        w += gap[j];
        w += gap[kItems + j];
      }
    }
    // smallest / largest level over the workgroup (integers: order does not matter), with the total gap weight
    double dlo = (double)lo_num, dhi = -(double)hi_num;
#pragma unroll
    for (int sft = 1; sft < 64; sft <<= 1) {
      dlo = fmin(dlo, __shfl_xor(dlo, sft, 64));
      dhi = fmin(dhi, __shfl_xor(dhi, sft, 64));
    }
    {
      double* r = red + turn * 3 * kMaxWaves;
      turn ^= 1;
      const double ws = wave_sum_d(w);
      if ((t & 63) == 0) { r[t >> 6] = dlo; r[kMaxWaves + (t >> 6)] = dhi; r[2 * kMaxWaves + (t >> 6)] = ws; }
      __syncthreads();
      dlo = r[0]; dhi = r[kMaxWaves]; w = r[2 * kMaxWaves];
      for (int q = 1; q < nwaves; ++q) {
        dlo = fmin(dlo, r[q]); dhi = fmin(dhi, r[kMaxWaves + q]); w += r[2 * kMaxWaves + q];
      }
    }
    // weighted median: smallest level whose cumulated gap weight reaches 0.5 (:239-245); if the total never does,
    // the reference's argmin over an all-inf row is index 0, the smallest level
    int lo = (int)dlo, hi = (int)(-dhi);
    if (!(w >= 0.5)) hi = lo;
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      double below = 0.0, z1 = 0.0, z2 = 0.0;
#pragma unroll
      for (int j = 0; j < 2 * kItems; ++j) below += (num[j] <= mid) ? gap[j] : 0.0;
      block_sum3(below, z1, z2, red, turn, nwaves);
      if (below >= 0.5) hi = mid; else lo = mid + 1;
    }
    const int med = lo;
    double acc = 0.0, z1 = 0.0, z2 = 0.0;
#pragma unroll
    for (int j = 0; j < 2 * kItems; ++j) acc += gap[j] * (double)abs(num[j] - med);
    block_sum3(acc, z1, z2, red, turn, nwaves);
    if (t == 0) {
      A.slice_cost[s] = acc / (double)n;
      if (A.slice_aux) A.slice_aux[s] = med;
    }
    if (cs) {
      // d cost / d coordinate = (|level before the atom's own weight - med| - |level - med|) / n; the first merged
      // atom has no gap before it
#pragma unroll
      for (int j = 0; j < kItems; ++j) {
        const int e = t + j * T;
        if (e < n) {
          {
            const int lb = (e + 1) - num[j];
            const bool first = (e == 0) && (lb == 0);
            const double before = first ? 0.0 : (double)abs(num[j] - 1 - med);
            if (pu[e] < n) cs[pu[e]] = (before - (double)abs(num[j] - med)) / (double)n;
          }
          {
            const int ub = num[kItems + j] + (e + 1);
            const bool first = (e == 0) && (ub == 0);
            const double before = first ? 0.0 : (double)abs(num[kItems + j] + 1 - med);
            if (pv[e] < n) ct[pv[e]] = (before - (double)abs(num[kItems + j] - med)) / (double)n;
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Point gradients: grad[b, i, :] = scale * (pair_w[b] + total_w[0]) * sum_l coef[b, l, i] * d coord / d x, the double
// form of ssw_backward_points_kernel: 64 points per workgroup, four waves split the slices (wave w takes l = w, w + 4,
// ... in order), their partial sums are added in wave order.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ssw_f64_backward_points_kernel(
    const double* __restrict__ xs, const double* __restrict__ xt, const double* __restrict__ dirs,
    const double* __restrict__ coef_s, const double* __restrict__ coef_t, int n, int slices, long u_pair_stride,
    double scale, const double* __restrict__ pair_w, const double* __restrict__ total_w, double* __restrict__ grad_xs,
    double* __restrict__ grad_xt, int chunks, int pair0) {
  __shared__ double part[3][4][64];
  const int b = pair0 + blockIdx.y;
  const bool is_t = (int)blockIdx.x >= chunks;
  const int chunk = is_t ? blockIdx.x - chunks : blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = chunk * 64 + lane;
  const int ic = min(i, n - 1);
  const double* X = (is_t ? xt : xs) + (long)b * n * 3;
  const double* C = (is_t ? coef_t : coef_s) + (long)b * slices * n;
  double* G = (is_t ? grad_xt : grad_xs) + (long)b * n * 3;
  const double* Ub = dirs + (long)b * u_pair_stride;
  const double px = X[3 * ic], py = X[3 * ic + 1], pz = X[3 * ic + 2];
  const double kTwoPi = 6.283185307179586;
  double gx = 0.0, gy = 0.0, gz = 0.0;
  for (int l = wave; l < slices; l += 4) {
    const double* U = Ub + (long)l * 6;
    const double c = C[(long)l * n + ic];
    const double a = fma(pz, U[4], fma(py, U[2], fma(px, U[0], 0.0)));
    const double bb = fma(pz, U[5], fma(py, U[3], fma(px, U[1], 0.0)));
    // a projection of exactly (0, 0) has no angle: zero gradient, as the reference's autograd gives (the float32
    // kernel's rule)
    const double r2 = fma(a, a, bb * bb);
    const double w = r2 > 0.0 ? c / (kTwoPi * r2) : 0.0;
    gx = fma(w, fma(a, U[1], -bb * U[0]), gx);
    gy = fma(w, fma(a, U[3], -bb * U[2]), gy);
    gz = fma(w, fma(a, U[5], -bb * U[4]), gz);
  }
  part[0][wave][lane] = gx;
  part[1][wave][lane] = gy;
  part[2][wave][lane] = gz;
  __syncthreads();
  if (wave == 0 && i < n) {
    double up = (pair_w || total_w) ? 0.0 : 1.0;
    if (pair_w) up += pair_w[b];
    if (total_w) up += total_w[0];
    const double sc = scale * up;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      double acc = part[d][0][lane];
#pragma unroll
      for (int w = 1; w < 4; ++w) acc += part[d][w][lane];
      G[3 * i + d] = acc * sc;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Reductions: one wavefront per pair (lane j adds slices j, j + 64, ... in order, then the butterfly), then one
// wavefront over the pairs.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void ssw_f64_reduce_pairs_kernel(const double* __restrict__ slice_cost, int slices,
                                                                  double scale, double* __restrict__ pair_loss) {
  const double* row = slice_cost + (long)blockIdx.x * slices;
  double acc = 0.0;
  for (int l = threadIdx.x; l < slices; l += 64) acc += row[l];
  acc = wave_sum_d(acc);
  if (threadIdx.x == 0) pair_loss[blockIdx.x] = acc * scale;
}

__global__ __launch_bounds__(64) void ssw_f64_reduce_total_kernel(const double* __restrict__ pair_loss, int pairs,
                                                                  double* __restrict__ total) {
  double acc = 0.0;
  for (int b = threadIdx.x; b < pairs; b += 64) acc += pair_loss[b];
  acc = wave_sum_d(acc);
  if (threadIdx.x == 0) {
    total[0] = acc;
    total[1] = acc / (double)pairs;
  }
}

// ---------------------------------------------------------------------------------------------
// Orthonormal 2-frames from Gaussian 3x2 matrices in double: stiefel_frames_kernel (shw_capi.hip) step for step --
// LAPACK's dgeqr2 + dorg2r, beta = -sign(alpha) * norm -- one thread per matrix.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void householder(double alpha, double x1, double x2, bool two, double& beta, double& tau,
                                            double& v1, double& v2) {
  const double xnorm = two ? sqrt(x1 * x1 + x2 * x2) : fabs(x1);
  if (xnorm == 0.0) { beta = alpha; tau = 0.0; v1 = 0.0; v2 = 0.0; return; }
  beta = -copysign(sqrt(alpha * alpha + xnorm * xnorm), alpha);
  tau = (beta - alpha) / beta;
  const double scale = 1.0 / (alpha - beta);
  v1 = x1 * scale;
  v2 = two ? x2 * scale : 0.0;
}

__global__ __launch_bounds__(256) void stiefel_frames_f64_kernel(const double* __restrict__ z, int count,
                                                                 double* __restrict__ u) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const double* Z = z + (long)i * 6;
  double a11 = Z[0], a12 = Z[1], a21 = Z[2], a22 = Z[3], a31 = Z[4], a32 = Z[5];
  double beta1, tau1, v1, v2;
  householder(a11, a21, a31, true, beta1, tau1, v1, v2);
  {
    const double w = a12 + v1 * a22 + v2 * a32;
    a12 -= tau1 * w;
    a22 -= tau1 * w * v1;
    a32 -= tau1 * w * v2;
  }
  double beta2, tau2, w1, unused;
  householder(a22, a32, 0.0, false, beta2, tau2, w1, unused);
  double q2x = 0.0, q2y = 1.0 - tau2, q2z = -tau2 * w1;
  {
    const double w = q2x + v1 * q2y + v2 * q2z;
    q2x -= tau1 * w;
    q2y -= tau1 * w * v1;
    q2z -= tau1 * w * v2;
  }
  double* U = u + (long)i * 6;
  U[0] = 1.0 - tau1; U[1] = q2x;
  U[2] = -tau1 * v1; U[3] = q2y;
  U[4] = -tau1 * v2; U[5] = q2z;
}

// problems = pairs * slices workgroups; level_median selects the p = 1 formula
static int launch(Args& A, bool level_median, hipStream_t stream) {
  int problems;
  if (!problem_groups(A.pairs, A.slices, 1, problems)) return (int)hipErrorInvalidValue;
  A.P = next_pow2(A.n);
  A.p_int = small_integer_power(A.p);
  int threads = A.P / kItems;
  threads = threads < 64 ? 64 : (threads > 1024 ? 1024 : threads);
  const size_t lds = (size_t)A.P * 32 + kFixedLds;
  auto kern = level_median ? ssw_f64_kernel<true> : ssw_f64_kernel<false>;
  if (const hipError_t e = level_median ? raise_dynamic_lds<ssw_f64_kernel<true>>(lds) : raise_dynamic_lds<ssw_f64_kernel<false>>(lds))
    return (int)e;
  hipLaunchKernelGGL(kern, dim3((unsigned)problems), dim3(threads), lds, stream, A);
  return (int)hipGetLastError();
}

}  // namespace f64
}  // namespace shw

extern "C" {

int shw_max_points_f64(void) { return SHW_MAX_POINTS_F64; }

int shw_stiefel_frames_f64(const double* z, long count, double* u, void* stream) {
  if (!z || !u || count < 0 || count > 0x7fffffffL) return (int)hipErrorInvalidValue;
  if (count == 0) return 0;
  hipLaunchKernelGGL(shw::f64::stiefel_frames_f64_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, z, (int)count, u);
  return (int)hipGetLastError();
}

int shw_ssw_forward_f64(const double* xs, const double* xt, const double* dirs, int pairs, int n, int m, int slices,
                        long u_pair_stride, double p, double* slice_cost, int32_t* slice_shift, double* coef_s,
                        double* coef_t, void* stream) {
  if (!xs || !xt || !dirs || !slice_cost) return (int)hipErrorInvalidValue;
  if ((coef_s == nullptr) != (coef_t == nullptr)) return (int)hipErrorInvalidValue;
  if (pairs < 0 || slices < 0 || n < 1 || n != m || n > SHW_MAX_POINTS_F64) return (int)hipErrorInvalidValue;
  if (!(p >= 1.0)) return (int)hipErrorInvalidValue;
  if (u_pair_stride != 0 && u_pair_stride < (long)slices * 6) return (int)hipErrorInvalidValue;
  if (pairs == 0 || slices == 0) return 0;
  shw::f64::Args A{};
  A.xs = xs; A.xt = xt; A.dirs = dirs; A.slice_cost = slice_cost; A.slice_aux = slice_shift;
  A.coef_s = coef_s; A.coef_t = coef_t;
  A.pairs = pairs; A.n = n; A.slices = slices; A.u_pair_stride = u_pair_stride; A.pstride = 3; A.p = p;
  return shw::f64::launch(A, p == 1.0, (hipStream_t)stream);
}

int shw_ssw_backward_points_f64(const double* xs, const double* xt, const double* dirs, const double* coef_s,
                                const double* coef_t, int pairs, int n, int m, int slices, long u_pair_stride,
                                double scale, const double* pair_w, const double* total_w, double* grad_xs,
                                double* grad_xt, void* stream) {
  if (!xs || !xt || !dirs || !coef_s || !coef_t || !grad_xs || !grad_xt) return (int)hipErrorInvalidValue;
  if (pairs < 0 || slices < 0 || n < 1 || n != m || n > SHW_MAX_POINTS_F64) return (int)hipErrorInvalidValue;
  if (u_pair_stride != 0 && u_pair_stride < (long)slices * 6) return (int)hipErrorInvalidValue;
  if (pairs == 0) return 0;
  const int chunks = (n + 63) / 64;
  for (int b0 = 0; b0 < pairs; b0 += 65535) {            // pairs ride on gridDim.y
    const int nb = pairs - b0 < 65535 ? pairs - b0 : 65535;
    hipLaunchKernelGGL(shw::f64::ssw_f64_backward_points_kernel, dim3(2 * chunks, nb), dim3(256), 0,
                       (hipStream_t)stream, xs, xt, dirs, coef_s, coef_t, n, slices, u_pair_stride, scale, pair_w,
                       total_w, grad_xs, grad_xt, chunks, b0);
  }
  return (int)hipGetLastError();
}

int shw_ssw_reduce_f64(const double* slice_cost, int pairs, int slices, double scale, double* pair_loss, double* total,
                       void* stream) {
  if (!slice_cost || !pair_loss || pairs < 0 || slices < 0) return (int)hipErrorInvalidValue;
  if (pairs == 0) return 0;
  hipLaunchKernelGGL(shw::f64::ssw_f64_reduce_pairs_kernel, dim3(pairs), dim3(64), 0, (hipStream_t)stream, slice_cost,
                     slices, scale, pair_loss);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  if (total) {
    hipLaunchKernelGGL(shw::f64::ssw_f64_reduce_total_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, pair_loss,
                       pairs, total);
    rc = (int)hipGetLastError();
  }
  return rc;
}

int shw_circle_ot_f64(const double* u, const double* v, int rows, int n, int m, double p, int method, double* cost,
                      int32_t* aux, double* grad_u, double* grad_v, void* stream) {
  if (!u || !v || !cost) return (int)hipErrorInvalidValue;
  if (method != SHW_CIRCLE_AS_SLICED && method != SHW_CIRCLE_BISECTION && method != SHW_CIRCLE_LEVEL_MEDIAN) return (int)hipErrorInvalidValue;
  if (method == SHW_CIRCLE_LEVEL_MEDIAN && p != 1.0) return (int)hipErrorInvalidValue;
  if ((grad_u == nullptr) != (grad_v == nullptr)) return (int)hipErrorInvalidValue;
  if (rows < 0 || n < 1 || n != m || n > SHW_MAX_POINTS_F64 || !(p >= 1.0)) return (int)hipErrorInvalidValue;
  if (rows == 0) return 0;
  // a row is a "pair" with ONE slice whose atoms already are circle coordinates
  shw::f64::Args A{};
  A.xs = u; A.xt = v; A.dirs = nullptr; A.slice_cost = cost; A.slice_aux = aux;
  A.coef_s = grad_u; A.coef_t = grad_v;
  A.pairs = rows; A.n = n; A.slices = 1; A.u_pair_stride = 0; A.pstride = 1; A.p = p;
  const bool level_median = p == 1.0 && method != SHW_CIRCLE_BISECTION;
  return shw::f64::launch(A, level_median, (hipStream_t)stream);
}

}  // extern "C"
