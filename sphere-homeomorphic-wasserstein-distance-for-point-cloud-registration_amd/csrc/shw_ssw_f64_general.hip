// shw_ssw_f64_general.hip -- float64 general circular OT for MI355X (gfx950): weighted and / or unequal-size clouds,
// any p >= 1, loss and training form, sliced level and circle level.
//
// Reference being replaced (paths relative to /root/reference/Point_Cloud_Resistration/losses/): sliced_cost
// (max_spherical_sliced_w.py:251-286, _fast.py:258-295), binary_search_circle (:117-207) with dCost (:25-65) and Cost
// (:68-113), emd1D_circle (:210-247), on double tensors (`dtype = u_values.dtype`, :153-160) with n != m and / or
// u_weights / v_weights.
//
// ONE WORKGROUP owns one (pair, slice):
//   1. + 2. projection, circle coordinate and sort of both clouds: project_and_sort of f64_common.hpp, shared with
//      shw_ssw_f64.hip;
//   3. both CDFs by a fixed-order scan of the weights gathered through the permutation (1/n, 1/m when absent);
//   4a. p != 1 at the sliced level, binary_search_circle for every p: min over the cut theta in [-1, 1] of Cost(theta),
//      the reference's quantile-merge integral.  Cost is convex and piecewise linear in theta, so the minimum sits on a
//      kink.  Search: six bisection steps on the signs of the one-sided slopes (dCost), then tangent intersection --
//      cross the right tangent at lo with the left tangent at hi, evaluate Cost and slopes at the crossing t, stop when
//      Cost(t) exceeds the tangents' value at t (a lower bound of the minimum over the bracket) by no more than
//      1e-15 Cost, or when the slopes at t straddle zero; else t replaces the end whose slope sign it shares.  Finite
//      because the function is piecewise linear; capped at kMaxRounds so that non-finite input cannot hang it.  The
//      smallest Cost seen and its cut are what is returned.
//      One evaluation: every source atom walks its own merge segments (the target levels inside its CDF step, two
//      binary searches over the rotated target CDF to find them), every target level evaluates both one-sided slope
//      terms (two binary searches over the source CDF); three workgroup sums.
//   4b. p == 1 at the sliced level and emd1D_circle: the level-median formula with the reference's omitted wrap segment
//      (SURVEY A7): every atom is placed in the other cloud by binary search, its level is the difference of the two
//      CDFs there, its gap the distance to its successor in the merge; the weighted median at threshold 0.5 is found by
//      bisection over the ordered bit patterns of the levels (at most 64 workgroup sums, no sort of the levels);
//   5. training form: d Cost(theta*) / d coordinate with the cut detached (:207), owner-computed -- every source atom
//      sums width * p |D|^(p-1) sgn D over its own segments, every target atom over its own -- and written to the row
//      of the slice at the ORIGINAL point index.
// Every sum runs in a fixed order; no floating-point atomics: results are bit-identical from run to run.
//
// LDS per workgroup, Pn / Pm = next power of two >= n / m, Pmax the larger: sorted values and CDFs of both clouds
// 16 (Pn + Pm), permutations 2 (Pn + Pm), scratch of the sort 12 Pmax (4a) or levels and gaps 16 (Pn + Pm) (4b), and
// 968 bytes fixed.  At n = m = 2048 (SHW_MAX_POINTS_F64_GENERAL): 64 KiB + 8 KiB + 24 KiB = 97 KiB for the cut search,
// 64 + 8 + 64 = 137 KiB for the level median, inside the 160 KiB.  4096 points would need 272 KiB for the level median.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/shw.h"
#include "dispatch.hpp"      // host launch helpers only
#include "f64_common.hpp"

namespace shw {
namespace f64 {

constexpr int kBisections = 6;       // slope-sign bisection steps before the tangent rounds
constexpr int kMaxRounds = 64;       // measured need: 13-17 rounds at 256 x 200, 21-22 at 1200 x 1000 weighted
constexpr int kGeneralFixedLds = 6 * kMaxWaves * 8 + kMaxWaves * 8 + (kMaxWaves + 2) * 4;

struct GeneralArgs {
  const double* xs;
  const double* xt;
  const double* dirs;                // NULL: rows of circle coordinates, one double per atom
  const double* wu;                  // NULL: uniform
  const double* wv;
  long wu_stride, wv_stride;         // doubles between the weight rows of consecutive pairs, 0 = shared
  double* slice_cost;
  double* slice_theta;               // cut theta* or median level, may be NULL
  double* coef_s;                    // both NULL: loss only
  double* coef_t;
  int pairs, n, m, slices, Pn, Pm;
  long u_pair_stride;
  double p;
  int p_int;
};

// cdf[i] = w[perm[0]] + ... + w[perm[i]] (1 / cnt each when w is NULL), i < cnt: thread t owns a run of consecutive
// positions, the runs are joined by a wave scan and the wave totals in order.  Ends with a barrier.
__device__ __forceinline__ void cdf_scan(const double* w, const uint16_t* perm, int cnt, double* cdf, double* wtot,
                                         int t, int T) {
  const int per = (cnt + T - 1) / T, first = t * per;
  const double uniform = 1.0 / (double)cnt;
  // (a permutation entry can only name a pad, >= cnt, on NaN input, whose order the network does not define: a pad's
  //  index must never become an address)
  auto weight = [&](int pos) -> double {
    if (!w) return uniform;
    const int at = perm[pos];
    return at < cnt ? w[at] : 0.0;
  };
  double local = 0.0;
  for (int j = 0; j < per; ++j)
    if (first + j < cnt) local += weight(first + j);
  double incl = local;
#pragma unroll
  for (int sft = 1; sft < 64; sft <<= 1) {
    const double up = __shfl_up(incl, sft, 64);
    if ((t & 63) >= sft) incl += up;
  }
  double run = __shfl_up(incl, 1, 64);
  if ((t & 63) == 0) run = 0.0;
  if ((t & 63) == 63) wtot[t >> 6] = incl;
  __syncthreads();
  double base = 0.0;
  for (int q = 0; q < (t >> 6); ++q) base += wtot[q];
  run += base;
  for (int j = 0; j < per; ++j) {
    if (first + j < cnt) {
      run += weight(first + j);
      cdf[first + j] = run;
    }
  }
  __syncthreads();
}

// The target after moving mass theta around the circle (:31-48): position k = 0..m-1 of the rotated order is sorted
// atom j = (first + k) mod m, `first` the first atom whose shifted CDF is not negative.
struct Rotation {
  const double* sv;
  const double* cv;
  int m, first, nwrap;               // atoms j < nwrap wrapped (shifted CDF below 0)
  double frac, turns;

  __device__ __forceinline__ int atom_of(int k) const {
    const int j = k + first;
    return j >= m ? j - m : j;
  }
  __device__ __forceinline__ double level(int k) const {             // re-based CDF, ascending in k
    const int j = atom_of(k);
    const double s = cv[j] - frac;
    return j < nwrap ? s + 1.0 : s;
  }
  __device__ __forceinline__ double atom(int k) const {              // k in [0, m]: position m is atom 0 one turn on
    const int j = k == m ? first : atom_of(k);
    const double a = sv[j] + (turns + (j < nwrap ? 1.0 : 0.0));
    return k == m ? a + 1.0 : a;
  }
  // number of levels < val (STRICT) or <= val
  template <bool STRICT>
  __device__ __forceinline__ int count(double val) const {
    int lo = 0, hi = m;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const double probe = level(mid);
      const bool go = STRICT ? (probe < val) : (probe <= val);
      if (go) lo = mid + 1; else hi = mid;
    }
    return lo;
  }
};

__device__ __forceinline__ Rotation rotate(double theta, const double* sv, const double* cv, int m) {
  Rotation R;
  R.sv = sv; R.cv = cv; R.m = m;
  R.turns = floor(theta);
  R.frac = theta - R.turns;
  R.nwrap = count_below<true>(cv, m, R.frac);          // cv[j] - frac < 0
  R.first = R.nwrap == m ? 0 : R.nwrap;                // all wrapped: the reference's argmin over an all-inf row is 0
  return R;
}

// The merge segments of source atom i at the rotation R, in merge order (:94-113: a grid point g belongs to the first
// source atom whose CDF reaches g, the last atom also takes what lies above its CDF; equal levels give zero widths).
// f(width, D) is called once per segment, D = source coordinate - target position.
template <class F>
__device__ __forceinline__ void source_segments(const Rotation& R, const double* su, const double* cu, int n, int i,
                                                F f) {
  const double own = cu[i], ui = su[i];
  double prev = i > 0 ? cu[i - 1] : 0.0;
  const int kstart = i > 0 ? R.count<false>(prev) : 0;
  const int kend = R.count<true>(own);
  for (int k = kstart; k < kend; ++k) {
    const double lv = R.level(k);
    f(lv - prev, ui - R.atom(k));
    prev = lv;
  }
  f(own - prev, ui - R.atom(kend));
  if (i == n - 1) {
    prev = own;
    for (int k = max(kstart, kend); k < R.m; ++k) {
      const double lv = R.level(k);
      f(lv - prev, ui - R.atom(k));
      prev = lv;
    }
  }
}

// The merge segments of the target atom at rotated position k: the source CDF levels in (level(k-1), level(k)] and its
// own level; position 0 also owns what lies above the last level, one turn on (`tail`).
template <class F>
__device__ __forceinline__ void target_segments(const Rotation& R, const double* su, const double* cu, int n, int k,
                                                F f) {
  const double own = R.level(k), ak = R.atom(k);
  double prev = k > 0 ? R.level(k - 1) : 0.0;
  const int istart = k > 0 ? count_below<false>(cu, n, prev) : 0;
  const int iend = count_below<false>(cu, n, own);
  for (int i = istart; i < iend; ++i) {
    f(cu[i] - prev, su[i] - ak);
    prev = cu[i];
  }
  f(own - prev, su[min(iend, n - 1)] - ak);
  if (k == 0) {
    prev = R.level(R.m - 1);
    const double am = R.atom(R.m);
    for (int i = count_below<false>(cu, n, prev); i < n; ++i) {
      f(cu[i] - prev, su[i] - am);
      prev = cu[i];
    }
  }
}

// Cost(theta) and its right / left derivative (dCost, :25-65), the same bits in every thread.
__device__ __forceinline__ void evaluate_cut(double theta, const double* su, const double* sv, const double* cu,
                                             const double* cv, int n, int m, double p, int p_int, double* red,
                                             int& turn, int t, int T, double& cost, double& d_plus, double& d_minus) {
  const Rotation R = rotate(theta, sv, cv, m);
  cost = 0.0; d_plus = 0.0; d_minus = 0.0;
  for (int i = t; i < n; i += T) {
    double acc = 0.0;
    source_segments(R, su, cu, n, i, [&](double width, double d) { acc += width * pow_abs(d, p, p_int); });
    cost += acc;
  }
  for (int k = t; k < m; k += T) {
    const double lv = R.level(k), cur = R.atom(k), nxt = R.atom(k + 1);
    const double left = su[min(count_below<true>(cu, n, lv), n - 1)];      // source quantile, left-continuous
    const int at = count_below<false>(cu, n, lv);                           // right-continuous, one wrapped atom (:54-57)
    const double right = at < n ? su[at] : su[0] + 1.0;
    d_plus += pow_abs(left - nxt, p, p_int) - pow_abs(left - cur, p, p_int);
    d_minus += pow_abs(right - nxt, p, p_int) - pow_abs(right - cur, p, p_int);
  }
  block_sum3(cost, d_plus, d_minus, red, turn, T >> 6);
}

// LEVEL_MEDIAN false: min over the cut (any p >= 1).  true: the p = 1 level-median formula.
template <bool LEVEL_MEDIAN>
__global__ __launch_bounds__(1024) void ssw_f64_general_kernel(GeneralArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int n = A.n, m = A.m, Pn = A.Pn, Pm = A.Pm, T = blockDim.x, t = threadIdx.x;
  const int Pmax = max(Pn, Pm);
  const int nwaves = T >> 6;
  double* su = reinterpret_cast<double*>(lds_raw);      // sorted source coordinates
  double* sv = su + Pn;                                 // sorted target coordinates
  double* cu = sv + Pm;                                 // source CDF
  double* cv = cu + Pn;                                 // target CDF
  double* red = cv + Pm;                                // 2 x 3 x kMaxWaves
  double* wtot = red + 6 * kMaxWaves;                   // kMaxWaves wave totals of the CDF scan
  unsigned* wsum = reinterpret_cast<unsigned*>(wtot + kMaxWaves);
  unsigned* flags = wsum + kMaxWaves;
  uint16_t* pu = reinterpret_cast<uint16_t*>(flags + 2);
  uint16_t* pv = pu + Pn;
  // (Pn + Pm) * 2 bytes of permutations: a multiple of 8, the scratch behind them is aligned for doubles
  double* scratch = reinterpret_cast<double*>(pv + Pm);
  double* tmp = scratch;                                // sort: a cloud's coordinates in original order, Pmax
  unsigned* hist = reinterpret_cast<unsigned*>(tmp + Pmax);   // sort: Pmax bins
  int turn = 0;

  const long s = blockIdx.x;
  const int b = (int)(s / A.slices), l = (int)(s - (long)b * A.slices);

  double U[6];
  if (A.dirs) {
    const double* Ul = A.dirs + (long)b * A.u_pair_stride + (long)l * 6;
#pragma unroll
    for (int i = 0; i < 6; ++i) U[i] = Ul[i];
  }
  if (t < 2) flags[t] = 0;
  const int pstride = A.dirs ? 3 : 1;
  project_and_sort(A.xs + (long)b * n * pstride, n, Pn, U, A.dirs != nullptr, su, pu, tmp, hist, wsum, flags, t, T);
  project_and_sort(A.xt + (long)b * m * pstride, m, Pm, U, A.dirs != nullptr, sv, pv, tmp, hist, wsum, flags + 1, t, T);
  cdf_scan(A.wu ? A.wu + (long)b * A.wu_stride : nullptr, pu, n, cu, wtot, t, T);
  cdf_scan(A.wv ? A.wv + (long)b * A.wv_stride : nullptr, pv, m, cv, wtot, t, T);

  double* cs = A.coef_s ? A.coef_s + s * n : nullptr;
  double* ct = A.coef_t ? A.coef_t + s * m : nullptr;
  const double p = A.p;
  const int p_int = A.p_int;

  if constexpr (!LEVEL_MEDIAN) {
    // ---- 4a. min over the cut ----------------------------------------------------------------------
    double lo = -1.0, hi = 1.0, c_lo, c_hi, dp_lo, dm_hi, dp, dm, c;
    evaluate_cut(lo, su, sv, cu, cv, n, m, p, p_int, red, turn, t, T, c_lo, dp_lo, dm);
    evaluate_cut(hi, su, sv, cu, cv, n, m, p, p_int, red, turn, t, T, c_hi, dp, dm_hi);
    double best = c_lo, best_theta = lo;
    if (c_hi < best) { best = c_hi; best_theta = hi; }
    // the minimum is inside the bracket while the cost falls to the right of lo and rises towards hi
    bool open = dp_lo < 0.0 && dm_hi > 0.0;
    for (int round = 0; open && round < kMaxRounds; ++round) {
      double cut = 0.5 * (lo + hi);
      if (round >= kBisections) {
        const double cross = (c_hi - c_lo + lo * dp_lo - hi * dm_hi) / (dp_lo - dm_hi);
        if (cross > lo && cross < hi) cut = cross;
      }
      if (!(cut > lo && cut < hi)) break;                 // no double left between the ends
      evaluate_cut(cut, su, sv, cu, cv, n, m, p, p_int, red, turn, t, T, c, dp, dm);
      if (c < best) { best = c; best_theta = cut; }
      if (dp * dm <= 0.0) break;                          // the slopes straddle zero: cut is a minimiser
      if (round >= kBisections) {
        const double bound = c_lo + dp_lo * (cut - lo);   // both tangents' value at their crossing
        if (c - bound <= 1e-15 * c) break;
      }
      if (dp < 0.0) { lo = cut; c_lo = c; dp_lo = dp; }
      else { hi = cut; c_hi = c; dm_hi = dm; }
    }
    if (t == 0) {
      A.slice_cost[s] = best;
      if (A.slice_theta) A.slice_theta[s] = best_theta;
    }
    if (cs) {
      const Rotation R = rotate(best_theta, sv, cv, m);
      for (int i = t; i < n; i += T) {
        double g = 0.0;
        source_segments(R, su, cu, n, i, [&](double width, double d) { g += width * dpow_abs(d, p, p_int); });
        if (pu[i] < n) cs[pu[i]] = g;                     // (the index tests only matter for NaN input)
      }
      for (int k = t; k < m; k += T) {
        double g = 0.0;
        target_segments(R, su, cu, n, k, [&](double width, double d) { g += width * dpow_abs(d, p, p_int); });
        const int j = R.atom_of(k);
        if (pv[j] < m) ct[pv[j]] = -g;
      }
    }
  } else {
    // ---- 4b. level median (p = 1) -----------------------------------------------------------------
    __syncthreads();                                      // the sort's scratch becomes levels and gaps
    double* lv = scratch;                                 // n + m levels, the source atoms first
    double* gp = scratch + Pn + Pm;                       // their gaps to the successor in the merge
    const double kInf = __builtin_inf();
    double w = 0.0, lo_lv = kInf, hi_lv = -kInf;
    for (int e = t; e < n + m; e += T) {
      double level, gap;
      if (e < n) {       // source atom: successor in the merged order (u before v on equal values) = min(u_(e+1), v_lb)
        const double val = su[e];
        const int lb = count_below<true>(sv, m, val);
        const double nxt = fmin(e + 1 < n ? su[e + 1] : kInf, lb < m ? sv[lb] : kInf);
        gap = (nxt == kInf ? 1.0 : nxt) - val;            // last merged atom: up to 1 (:237)
        level = cu[e] - (lb > 0 ? cv[lb - 1] : 0.0);
      } else {
        const int j = e - n;
        const double val = sv[j];
        const int ub = count_below<false>(su, n, val);
        const double nxt = fmin(j + 1 < m ? sv[j + 1] : kInf, ub < n ? su[ub] : kInf);
        gap = (nxt == kInf ? 1.0 : nxt) - val;
        level = (ub > 0 ? cu[ub - 1] : 0.0) - cv[j];
      }
      level += 0.0;                                       // -0 -> +0: one bit pattern per value
      lv[e] = level;
      gp[e] = gap;
      w += gap;
      lo_lv = fmin(lo_lv, level);
      hi_lv = fmax(hi_lv, level);
    }
    // smallest / largest level over the workgroup (order does not matter), with the total gap weight
    double neg_hi = -hi_lv;
#pragma unroll
    for (int sft = 1; sft < 64; sft <<= 1) {
      lo_lv = fmin(lo_lv, __shfl_xor(lo_lv, sft, 64));
      neg_hi = fmin(neg_hi, __shfl_xor(neg_hi, sft, 64));
    }
    {
      double* r = red + turn * 3 * kMaxWaves;
      turn ^= 1;
      const double ws = wave_sum_d(w);
      if ((t & 63) == 0) { r[t >> 6] = lo_lv; r[kMaxWaves + (t >> 6)] = neg_hi; r[2 * kMaxWaves + (t >> 6)] = ws; }
      __syncthreads();
      lo_lv = r[0]; neg_hi = r[kMaxWaves]; w = r[2 * kMaxWaves];
      for (int q = 1; q < nwaves; ++q) {
        lo_lv = fmin(lo_lv, r[q]); neg_hi = fmin(neg_hi, r[kMaxWaves + q]); w += r[2 * kMaxWaves + q];
      }
    }
    // weighted median: smallest level whose cumulated gap weight reaches 0.5 (:239-245); if the total never does, the
    // reference's argmin over an all-inf row is index 0, the smallest level.  Bisection over the ordered keys of the
    // levels: a double's bits, sign-folded, order as the doubles do.
    auto key_of = [](double x) -> unsigned long long {
      const long long bits = __double_as_longlong(x);
      return (unsigned long long)bits ^ (bits < 0 ? ~0ull : 0x8000000000000000ull);
    };
    auto level_of = [](unsigned long long k) -> double {
      const unsigned long long bits = (k & 0x8000000000000000ull) ? k ^ 0x8000000000000000ull : ~k;
      return __longlong_as_double((long long)bits);
    };
    unsigned long long klo = key_of(lo_lv), khi = key_of(-neg_hi);
    if (!(w >= 0.5) || !(klo <= khi)) khi = klo;
    while (klo < khi) {                                   // at most 64 steps
      const unsigned long long mid = klo + ((khi - klo) >> 1);
      double below = 0.0, z1 = 0.0, z2 = 0.0;
      for (int e = t; e < n + m; e += T) below += (key_of(lv[e]) <= mid) ? gp[e] : 0.0;
      block_sum3(below, z1, z2, red, turn, nwaves);
      if (below >= 0.5) khi = mid; else klo = mid + 1;
    }
    const double med = level_of(klo);
    double acc = 0.0, z1 = 0.0, z2 = 0.0;
    for (int e = t; e < n + m; e += T) acc += gp[e] * fabs(lv[e] - med);
    block_sum3(acc, z1, z2, red, turn, nwaves);
    if (t == 0) {
      A.slice_cost[s] = acc;
      if (A.slice_theta) A.slice_theta[s] = med;
    }
    if (cs) {
      // d cost / d coordinate = |level before the atom's own weight - med| - |level - med|; the first merged atom has
      // no gap before it
      for (int e = t; e < n + m; e += T) {
        if (e < n) {
          const int lb = count_below<true>(sv, m, su[e]);
          const double before_lv = (e > 0 ? cu[e - 1] : 0.0) - (lb > 0 ? cv[lb - 1] : 0.0);
          const double before = (e == 0 && lb == 0) ? 0.0 : fabs(before_lv - med);
          if (pu[e] < n) cs[pu[e]] = before - fabs(lv[e] - med);
        } else {
          const int j = e - n;
          const int ub = count_below<false>(su, n, sv[j]);
          const double before_lv = (ub > 0 ? cu[ub - 1] : 0.0) - (j > 0 ? cv[j - 1] : 0.0);
          const double before = (j == 0 && ub == 0) ? 0.0 : fabs(before_lv - med);
          if (pv[j] < m) ct[pv[j]] = before - fabs(lv[e] - med);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Point gradients for two cloud sizes: ssw_f64_backward_points_kernel (shw_ssw_f64.hip) with a count per cloud --
// grad[b, i, :] = scale * (pair_w[b] + total_w[0]) * sum_l coef[b, l, i] * d coord / d x, 64 points per workgroup, four
// waves split the slices (wave w takes l = w, w + 4, ... in order), their partial sums are added in wave order.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ssw_f64_general_backward_points_kernel(
    const double* __restrict__ xs, const double* __restrict__ xt, const double* __restrict__ dirs,
    const double* __restrict__ coef_s, const double* __restrict__ coef_t, int n, int m, int slices, long u_pair_stride,
    double scale, const double* __restrict__ pair_w, const double* __restrict__ total_w, double* __restrict__ grad_xs,
    double* __restrict__ grad_xt, int chunks_s, int pair0) {
  __shared__ double part[3][4][64];
  const int b = pair0 + blockIdx.y;
  const bool is_t = (int)blockIdx.x >= chunks_s;
  const int chunk = is_t ? blockIdx.x - chunks_s : blockIdx.x;
  const int cnt = is_t ? m : n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = chunk * 64 + lane;
  const int ic = min(i, cnt - 1);
  const double* X = (is_t ? xt : xs) + (long)b * cnt * 3;
  const double* C = (is_t ? coef_t : coef_s) + (long)b * slices * cnt;
  double* G = (is_t ? grad_xt : grad_xs) + (long)b * cnt * 3;
  const double* Ub = dirs + (long)b * u_pair_stride;
  const double px = X[3 * ic], py = X[3 * ic + 1], pz = X[3 * ic + 2];
  const double kTwoPi = 6.283185307179586;
  double gx = 0.0, gy = 0.0, gz = 0.0;
  for (int l = wave; l < slices; l += 4) {
    const double* U = Ub + (long)l * 6;
    const double c = C[(long)l * cnt + ic];
    const double a = fma(pz, U[4], fma(py, U[2], fma(px, U[0], 0.0)));
    const double bb = fma(pz, U[5], fma(py, U[3], fma(px, U[1], 0.0)));
    const double r2 = fma(a, a, bb * bb);               // a projection of exactly (0, 0) has no angle: zero gradient
    const double w = r2 > 0.0 ? c / (kTwoPi * r2) : 0.0;
    gx = fma(w, fma(a, U[1], -bb * U[0]), gx);
    gy = fma(w, fma(a, U[3], -bb * U[2]), gy);
    gz = fma(w, fma(a, U[5], -bb * U[4]), gz);
  }
  part[0][wave][lane] = gx;
  part[1][wave][lane] = gy;
  part[2][wave][lane] = gz;
  __syncthreads();
  if (wave == 0 && i < cnt) {
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

static size_t general_lds(int Pn, int Pm, bool level_median) {
  const int Pmax = Pn > Pm ? Pn : Pm;
  const size_t scratch = level_median ? (size_t)16 * (Pn + Pm) : (size_t)12 * Pmax;
  const size_t sort_scratch = (size_t)12 * Pmax;        // the level-median form sorts first, in the same bytes
  return (size_t)18 * (Pn + Pm) + (scratch > sort_scratch ? scratch : sort_scratch) + kGeneralFixedLds;
}

// problems = pairs * slices workgroups; level_median selects the p = 1 formula
static int launch_general(GeneralArgs& A, bool level_median, hipStream_t stream) {
  int problems;
  if (!problem_groups(A.pairs, A.slices, 1, problems)) return (int)hipErrorInvalidValue;
  A.Pn = next_pow2(A.n < 4 ? 4 : A.n);                 // at least 4: the permutations stay a multiple of 8 bytes
  A.Pm = next_pow2(A.m < 4 ? 4 : A.m);
  A.p_int = small_integer_power(A.p);
  int threads = (A.Pn > A.Pm ? A.Pn : A.Pm) / 2;
  threads = threads < 64 ? 64 : (threads > 1024 ? 1024 : threads);
  const size_t lds = general_lds(A.Pn, A.Pm, level_median);
  auto kern = level_median ? ssw_f64_general_kernel<true> : ssw_f64_general_kernel<false>;
  if (const hipError_t e = level_median ? raise_dynamic_lds<ssw_f64_general_kernel<true>>(lds)
                                        : raise_dynamic_lds<ssw_f64_general_kernel<false>>(lds))
    return (int)e;
  hipLaunchKernelGGL(kern, dim3((unsigned)problems), dim3(threads), lds, stream, A);
  return (int)hipGetLastError();
}

static bool sizes_ok(int n, int m) {
  return n >= 1 && m >= 1 && n <= SHW_MAX_POINTS_F64_GENERAL && m <= SHW_MAX_POINTS_F64_GENERAL;
}

}  // namespace f64
}  // namespace shw

extern "C" {

int shw_max_points_f64_general(void) { return SHW_MAX_POINTS_F64_GENERAL; }

int shw_ssw_forward_general_f64(const double* xs, const double* xt, const double* dirs, const double* wu,
                                const double* wv, long wu_pair_stride, long wv_pair_stride, int pairs, int n, int m,
                                int slices, long u_pair_stride, double p, double* slice_cost, double* slice_theta,
                                double* coef_s, double* coef_t, void* stream) {
  if (!xs || !xt || !dirs || !slice_cost) return (int)hipErrorInvalidValue;
  if ((coef_s == nullptr) != (coef_t == nullptr)) return (int)hipErrorInvalidValue;
  if (pairs < 0 || slices < 0 || !shw::f64::sizes_ok(n, m)) return (int)hipErrorInvalidValue;
  if (!(p >= 1.0)) return (int)hipErrorInvalidValue;
  if (u_pair_stride != 0 && u_pair_stride < (long)slices * 6) return (int)hipErrorInvalidValue;
  if (wu_pair_stride < 0 || wv_pair_stride < 0) return (int)hipErrorInvalidValue;
  if (pairs == 0 || slices == 0) return 0;
  shw::f64::GeneralArgs A{};
  A.xs = xs; A.xt = xt; A.dirs = dirs; A.wu = wu; A.wv = wv; A.wu_stride = wu_pair_stride; A.wv_stride = wv_pair_stride;
  A.slice_cost = slice_cost; A.slice_theta = slice_theta; A.coef_s = coef_s; A.coef_t = coef_t;
  A.pairs = pairs; A.n = n; A.m = m; A.slices = slices; A.u_pair_stride = u_pair_stride; A.p = p;
  return shw::f64::launch_general(A, p == 1.0, (hipStream_t)stream);
}

int shw_ssw_backward_points_general_f64(const double* xs, const double* xt, const double* dirs, const double* coef_s,
                                        const double* coef_t, int pairs, int n, int m, int slices, long u_pair_stride,
                                        double scale, const double* pair_w, const double* total_w, double* grad_xs,
                                        double* grad_xt, void* stream) {
  if (!xs || !xt || !dirs || !coef_s || !coef_t || !grad_xs || !grad_xt) return (int)hipErrorInvalidValue;
  if (pairs < 0 || slices < 0 || !shw::f64::sizes_ok(n, m)) return (int)hipErrorInvalidValue;
  if (u_pair_stride != 0 && u_pair_stride < (long)slices * 6) return (int)hipErrorInvalidValue;
  if (pairs == 0) return 0;
  const int chunks_s = (n + 63) / 64, chunks_t = (m + 63) / 64;
  for (int b0 = 0; b0 < pairs; b0 += 65535) {            // pairs ride on gridDim.y
    const int nb = pairs - b0 < 65535 ? pairs - b0 : 65535;
    hipLaunchKernelGGL(shw::f64::ssw_f64_general_backward_points_kernel, dim3(chunks_s + chunks_t, nb), dim3(256), 0,
                       (hipStream_t)stream, xs, xt, dirs, coef_s, coef_t, n, m, slices, u_pair_stride, scale, pair_w,
                       total_w, grad_xs, grad_xt, chunks_s, b0);
  }
  return (int)hipGetLastError();
}

int shw_circle_ot_general_f64(const double* u, const double* v, const double* wu, const double* wv, long wu_row_stride,
                              long wv_row_stride, int rows, int n, int m, double p, int method, double* cost,
                              double* aux, double* grad_u, double* grad_v, void* stream) {
  if (!u || !v || !cost) return (int)hipErrorInvalidValue;
  if (method != SHW_CIRCLE_AS_SLICED && method != SHW_CIRCLE_BISECTION && method != SHW_CIRCLE_LEVEL_MEDIAN) return (int)hipErrorInvalidValue;
  if (method == SHW_CIRCLE_LEVEL_MEDIAN && p != 1.0) return (int)hipErrorInvalidValue;
  if ((grad_u == nullptr) != (grad_v == nullptr)) return (int)hipErrorInvalidValue;
  if (rows < 0 || !shw::f64::sizes_ok(n, m) || !(p >= 1.0)) return (int)hipErrorInvalidValue;
  if (wu_row_stride < 0 || wv_row_stride < 0) return (int)hipErrorInvalidValue;
  if (rows == 0) return 0;
  // a row is a "pair" with ONE slice whose atoms already are circle coordinates
  shw::f64::GeneralArgs A{};
  A.xs = u; A.xt = v; A.dirs = nullptr; A.wu = wu; A.wv = wv; A.wu_stride = wu_row_stride; A.wv_stride = wv_row_stride;
  A.slice_cost = cost; A.slice_theta = aux; A.coef_s = grad_u; A.coef_t = grad_v;
  A.pairs = rows; A.n = n; A.m = m; A.slices = 1; A.u_pair_stride = 0; A.p = p;
  const bool level_median = p == 1.0 && method != SHW_CIRCLE_BISECTION;
  return shw::f64::launch_general(A, level_median, (hipStream_t)stream);
}

}  // extern "C"
