// shw_ssw_weights.hip -- spherical sliced-W: the gradient of a slice's circular OT cost with respect to the WEIGHTS of the
// two clouds, for the forms that take weights: (b) the cut search (every p >= 1) and (c) the p = 1 level
// median.  One workgroup of four waves per (pair, slice) or per row of circle coordinates; the clouds come through the
// loaders of the general kernels (prepare_one: R^3 projection or coordinate rows, the same sorted values and float32 CDFs
// as the solve), the cut is the one the solve launch left.  The solve is not repeated; where its cut is not on the
// minimising kink the window of the two-sided evaluation is moved onto it (see the polish loop of the cut kernel).
//
// Form (b).  W(a, b) = min over the cut of Cost(cut; a, b), and the minimiser sits on a kink: a source level A_r meets a
// rotated target level C_j = B_j - cut (mod 1).  The fixed-cut derivatives are suffix sums of the jumps of the cost at the
// CDF ends,
//     source level A_r (r < n-1):  c(u_r, y) - c(u_(r+1), y),   y the rotated target atom active at A_r
//     target level C_j          :  c(x, v_j) - c(x, v_next(j)), x the source atom active at C_j, next(j) the next atom
//                                   around the circle (the first rotated atom's copy one turn later after the last)
// summed over r >= i resp. over j >= k in the ORIGINAL sorted order of the target (a target weight moves the levels of the
// atoms at or after it there, wherever the cut puts them).  The slope in the cut is minus the sum of all target jumps.
// The gradient of W is the mix  G = lambda G+ + (1 - lambda) G-  of the fixed-cut derivatives on the two sides of the kink
// with the weight that cancels the slope, lambda = -s- / (s+ - s-), clipped to [0, 1] (0.5 when both slopes are 0).  The
// solve's float32 cut is within rounding of the kink at best, so the two sides are evaluated at t - eta and t + eta
// (kEta, a few float32 ulps of a level; levels compared in double): every level pair the cut is tied with, or nearly, falls
// on the source-first side in one evaluation and on the target-first side in the other.  t starts at the solve's cut.
// Form (c).  In merged order: gaps g_k, levels, the median level_(k*), sigma_k = sign(level_k - median),
// H_k = sum_(t >= k) g_t sigma_t, S = H_0; the derivative with respect to the signed weight at k is H_k - S [k <= k*].
//
// Jumps are differences of float32 costs, summed in double in a fixed order over the workgroup's threads (no atomics:
// the same bits on every run).  Output rows are centred (sum_i a_i G_i = 0: the gradient of the cost composed with
// w -> w / sum w), a side of one atom is exactly 0, un-permuted through LDS and stored coalesced.
#include "general_cut.hpp"
#include "general_p1.hpp"

namespace shw {

struct WeightPotArgs {
  GeneralArgs G;          // clouds, frames, weights (prepare_one)
  const float* cut;       // (pairs * slices) the solve's cut; form (c): unused
  float* pot_u;           // (pairs * slices, n) or NULL
  float* pot_v;           // (pairs * slices, m) or NULL
};

constexpr int kPotThreads = 256;
constexpr double kEta = 3e-7;                                // half-width of the two-sided evaluation around the cut
constexpr double kEtaMin = 1e-9;                              // ... and the narrowest window the polish goes down to
constexpr int kPolishEvals = 48;                             // evaluations a row may spend on moving the window onto the kink

// index of element i of an array that threads walk in contiguous chunks: one pad word per 32 keeps the chunks of
// neighbouring threads on different banks
__device__ __forceinline__ int pad32(int i) { return i + (i >> 5); }
constexpr int padded_floats(int count) { return count + (count >> 5) + 1; }

// sum over the workgroup in thread order; every thread gets the same bits.  Two barriers: `red` is free again on return.
__device__ __forceinline__ double block_sum(double v, double* red, int tid) {
  red[tid] = v;
  __syncthreads();
  double acc = 0.0;
  for (int q = 0; q < kPotThreads; ++q) acc += red[q];
  __syncthreads();
  return acc;
}

__device__ __forceinline__ double block_min(double v, double* red, int tid) {
  red[tid] = v;
  __syncthreads();
  double acc = red[0];
  for (int q = 1; q < kPotThreads; ++q) acc = fmin(acc, red[q]);
  __syncthreads();
  return acc;
}

// arr[pad32(i)] <- sum_(t >= i) arr[pad32(t)], i < count: chunks of consecutive entries per thread, the chunks' totals
// added from the last one down, all in double
__device__ __forceinline__ void block_suffix_sum(float* arr, int count, double* red, int tid) {
  const int ch = (count + kPotThreads - 1) / kPotThreads;
  const int b = min(tid * ch, count), e = min(b + ch, count);
  double tot = 0.0;
  for (int i = b; i < e; ++i) tot += (double)arr[pad32(i)];
  red[tid] = tot;
  __syncthreads();
  double run = 0.0;
  for (int q = kPotThreads - 1; q > tid; --q) run += red[q];
  for (int i = e - 1; i >= b; --i) {
    run += (double)arr[pad32(i)];
    arr[pad32(i)] = (float)run;
  }
  __syncthreads();
}

// number of the first `count` entries of an ascending array (lds_slot layout) below `key`, or not above it
template <int EPT>
__device__ __forceinline__ int count_below(const float* arr, int count, double key, bool inclusive) {
  int lo = 0, hi = count;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const double x = (double)arr[lds_slot<EPT>(mid)];
    const bool go = inclusive ? (x <= key) : (x < key);
    lo = go ? mid + 1 : lo;
    hi = go ? hi : mid;
  }
  return lo;
}

// LDS of both kernels: the four rows of the sorted clouds, four padded rows of jumps / merged-order arrays, the two
// sorted -> original index maps (16 bit) and the reduction slots
template <int EPT>
constexpr size_t weight_pot_lds_bytes() {
  return (size_t)(4 * EPT * kWave + 4 * padded_floats(EPT * kWave)) * sizeof(float) + (size_t)2 * EPT * kWave * sizeof(unsigned short) +
         (size_t)kPotThreads * sizeof(double);
}

template <int EPT>
struct WeightPotLds {
  float *s_val, *s_cdf, *t_val, *t_cdf, *work;
  unsigned short *idx_s, *idx_t;
  double* red;
  __device__ __forceinline__ explicit WeightPotLds(float* lds) {
    constexpr int ROW = EPT * kWave;
    red = reinterpret_cast<double*>(lds);                    // (first: 8-byte aligned)
    float* f = lds + 2 * kPotThreads;
    s_val = f; s_cdf = f + ROW; t_val = f + 2 * ROW; t_cdf = f + 3 * ROW;
    work = f + 4 * ROW;
    idx_s = reinterpret_cast<unsigned short*>(work + 4 * padded_floats(ROW));
    idx_t = idx_s + ROW;
  }
};

// sort both clouds of slice s (wave 0: the source, wave 1: the target) and leave the index maps in LDS
template <int EPT>
__device__ __forceinline__ void load_sorted_sides(const GeneralArgs& G, int s, int wave, int lane, const WeightPotLds<EPT>& L) {
  if (wave < 2) {
    const int which = 1 - wave;
    float* dval = which == 0 ? L.t_val : L.s_val;
    float* dcdf = which == 0 ? L.t_cdf : L.s_cdf;
    unsigned short* didx = which == 0 ? L.idx_t : L.idx_s;
    const int count = which == 0 ? G.base.m : G.base.n;
    int idx[EPT];
    float mean_unused;
    prepare_one<EPT, false>(G, s, lane, which, dval, dcdf, dval, reinterpret_cast<unsigned*>(dcdf), idx, mean_unused);
#pragma unroll
    for (int r = 0; r < EPT; ++r) {
      const int e = lane * EPT + r;
      if (e < count) didx[e] = (unsigned short)idx[r];
    }
  }
  __syncthreads();
}

// centre one side's potentials (sorted order, arr[pad32(e)]) against its weights, un-permute through `by_index` and store
__device__ __forceinline__ void centre_and_store(const float* arr, int count, const unsigned short* idx, const float* w,
                                                 float sign, float* by_index, float* out, double* red, int tid) {
  double aw = 0.0, ag = 0.0;
  for (int e = tid; e < count; e += kPotThreads) {
    const double a = (double)w[idx[e]];
    aw += a;
    ag += a * (double)(sign * arr[pad32(e)]);
  }
  const double total = block_sum(aw, red, tid);
  const double mean = block_sum(ag, red, tid) / total;
  for (int e = tid; e < count; e += kPotThreads)
    by_index[idx[e]] = count == 1 ? 0.f : (float)(((double)(sign * arr[pad32(e)]) - mean) / total);
  __syncthreads();
  for (int i = tid; i < count; i += kPotThreads) out[i] = by_index[i];
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------
// form (b): the cut search's value, every p >= 1
// ---------------------------------------------------------------------------------------------
template <int EPT, int PMODE>
__global__ __launch_bounds__(kPotThreads) void ssw_weight_pot_cut_kernel(WeightPotArgs P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int ROW = EPT * kWave;
  constexpr int PROW = padded_floats(ROW);
  const GeneralArgs& G = P.G;
  const SswArgs& A = G.base;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const WeightPotLds<EPT> L(lds);
  const int s = xcd_contiguous_id(blockIdx.x, A.num_groups);
  if (s >= A.pairs * A.slices) return;                       // (uniform over the workgroup)
  const int n = A.n, m = A.m;
  load_sorted_sides<EPT>(G, s, wave, lane, L);
  const Side<EPT> S{L.s_val, L.s_cdf, n}, T{L.t_val, L.t_cdf, m};
  const float p = A.p;
  const int p_int = A.p_int;
  const float theta = P.cut[s];

  // the jumps and the slope on the two sides of the cut t: slope0 at t - eta, ties source first; slope1 at t + eta, target
  // first; kinks: source levels that a target level crosses inside the window (the rank of the first pass rides in the
  // second pass's jump slot until that pass overwrites it -- the same thread owns the level in both)
  double slope0 = 0.0, slope1 = 0.0, kinks = 0.0, eta = kEta;
  auto evaluate = [&](double t) {
    double crossed = 0.0;
#pragma nounroll
    for (int ev = 0; ev < 2; ++ev) {
      float* ja = L.work + ev * 2 * PROW;
      float* jb = ja + PROW;
      int* rank0 = reinterpret_cast<int*>(L.work + 2 * PROW);
      const double td = t + (ev ? eta : -eta);
      const double turns_d = floor(td);
      const double fr = td - turns_d;
      const float turns = (float)turns_d;
      const int nw = count_below<EPT>(T.cdf, m, fr, false);  // wrapped atoms: B_j - fr < 0
      const int start = nw >= m ? 0 : nw;                    // first atom of the rotated order
      for (int r = tid; r < n; r += kPotThreads) {
        float jump = 0.f;                                    // (the last level is 1 whatever the weights: no jump)
        if (r < n - 1) {
          const double key = (double)S.c(r) + fr;            // C_j < A_r  <=>  B_j < A_r + fr (- 1 for a wrapped atom)
          const int c1 = count_below<EPT>(T.cdf, m, key, ev == 1);
          const int c2 = count_below<EPT>(T.cdf, m, key - 1.0, ev == 1);
          const int rho = max(c1 - nw, 0) + min(c2, nw);     // rotated target levels before A_r: 0..m
          int j = rho + start;
          j = j >= m ? j - m : j;
          float pos = T.v(j) + (turns + (((double)T.c(j) < fr) ? 1.f : 0.f));
          pos += rho >= m ? 1.f : 0.f;                       // the appended copy of the first rotated atom
          jump = powp<PMODE>(S.v(r) - pos, p, p_int) - powp<PMODE>(S.v(r + 1) - pos, p, p_int);
          // (the rotation's start moves with the cut: compare ranks as atoms of the target's own order)
          if (ev == 0) rank0[pad32(r)] = j + (rho >= m ? m : 0);
          else crossed += rank0[pad32(r)] != j + (rho >= m ? m : 0) ? 1.0 : 0.0;
        }
        ja[pad32(r)] = jump;
      }
      double part = 0.0;
      for (int j = tid; j < m; j += kPotThreads) {
        const double sh = (double)T.c(j) - fr;
        const bool wrapped = sh < 0.0;
        const double level = wrapped ? sh + 1.0 : sh;
        // the source atom active at the level; the last source level is 1 whatever its float32 sum says
        const int i = min(count_below<EPT>(S.cdf, n - 1, level, ev == 0), n - 1);
        const int jn = j + 1 == m ? 0 : j + 1;
        const float pos = T.v(j) + (turns + (wrapped ? 1.f : 0.f));
        const float posn = T.v(jn) + (turns + (((double)T.c(jn) < fr) ? 1.f : 0.f)) + (jn == start ? 1.f : 0.f);
        const float u = S.v(i);
        const float jump = powp<PMODE>(u - pos, p, p_int) - powp<PMODE>(u - posn, p, p_int);
        jb[pad32(j)] = jump;
        part += (double)jump;
      }
      const double sl = -block_sum(part, L.red, tid);        // (also the barrier that publishes ja, jb)
      if (ev == 0) slope0 = sl; else slope1 = sl;
    }
    kinks = block_sum(crossed, L.red, tid);
  };
  // The solve's cut is within float32 rounding of the minimising kink when the solve ended ON a kink; its other exit
  // (an end of the bracket once nothing is left to gain in the COST) can leave it many kinks away, where the potentials
  // are another piece's.  Both slopes of one sign say so, and which way the minimum lies: step out from the cut until the
  // sign changes (first step: Newton at curvature 2), then close in -- secant and midpoint in turns -- until the window
  // holds the minimum.  A window that holds it together with other kinks (dense clouds: n m kinks per turn) is quartered
  // and moved again, until one kink is left, the count stops falling (exactly tied levels) or the window is 1e-9 wide.
  // Slopes and counts are sums in double in a fixed order, uniform over the workgroup: so is every decision.
  double t = (double)theta, lo = 0.0, hi = 0.0, f_lo = 0.0, f_hi = 0.0, step = 0.0, kinks_before = -1.0;
  bool has_lo = false, has_hi = false;
  for (int it = 0; it < kPolishEvals; ++it) {
    evaluate(t);
    const bool last = it + 1 == kPolishEvals;
    if (slope0 <= 0.0 && slope1 >= 0.0) {                    // the window holds the minimum
      if (kinks <= 1.0 || kinks == kinks_before || eta <= kEtaMin || last || slope0 == 0.0 || slope1 == 0.0) break;
      kinks_before = kinks;
      lo = t - eta; f_lo = slope0; hi = t + eta; f_hi = slope1;
      has_lo = has_hi = true;
      eta = fmax(0.25 * eta, kEtaMin);
    } else {
      const bool left = slope0 > 0.0, right = slope1 < 0.0;  // ... lies to the left / to the right of the window
      if (!(left || right) || last) break;                   // (non-finite input)
      if (left) { hi = t; f_hi = slope0; has_hi = true; }
      else { lo = t; f_lo = slope1; has_lo = true; }
    }
    if (has_lo && has_hi) {
      const double secant = lo + (hi - lo) * (-f_lo) / (f_hi - f_lo);
      t = (it & 1) ? secant : 0.5 * (lo + hi);
      t = fmin(fmax(t, lo + eta), hi - eta);
      if (!(t > lo && t < hi)) t = 0.5 * (lo + hi);
    } else {
      step = step == 0.0 ? fmax(0.75 * fabs(has_hi ? f_hi : f_lo), 4.0 * eta) : 2.0 * step;
      t = has_hi ? t - step : t + step;
    }
  }
  // the mix that cancels the slope
  double lambda;
  if (slope0 == 0.0 && slope1 == 0.0) lambda = 0.5;
  else if (slope0 >= 0.0) lambda = 0.0;                      // the window is not left of the minimum: the lower side alone
  else if (slope1 <= 0.0) lambda = 1.0;
  else lambda = -slope0 / (slope1 - slope0);
  if (!(lambda >= 0.0 && lambda <= 1.0)) lambda = 0.5;       // non-finite input
  float* ja = L.work;
  float* jb = L.work + PROW;
  for (int i = tid; i < max(n, m); i += kPotThreads) {
    if (i < n) {
      const double lo = (double)ja[pad32(i)], hi = (double)ja[2 * PROW + pad32(i)];
      ja[pad32(i)] = (float)(lo + lambda * (hi - lo));
    }
    if (i < m) {
      const double lo = (double)jb[pad32(i)], hi = (double)jb[2 * PROW + pad32(i)];
      jb[pad32(i)] = (float)(lo + lambda * (hi - lo));
    }
  }
  __syncthreads();
  const int b = s / A.slices;
  if (P.pot_u) {
    block_suffix_sum(ja, n, L.red, tid);
    centre_and_store(ja, n, L.idx_s, G.wu + (long)b * G.wu_pair_stride, 1.f, L.s_val, P.pot_u + (long)s * n, L.red, tid);
  }
  if (P.pot_v) {
    block_suffix_sum(jb, m, L.red, tid);
    centre_and_store(jb, m, L.idx_t, G.wv + (long)b * G.wv_pair_stride, 1.f, L.t_val, P.pot_v + (long)s * m, L.red, tid);
  }
}

// ---------------------------------------------------------------------------------------------
// form (c): the p = 1 level median
// ---------------------------------------------------------------------------------------------
// merged position, level and gap of source atom e (source before target on equal values), as ssw_general_p1_kernel
template <int EPT>
__device__ __forceinline__ void merged_source(const Side<EPT>& S, const Side<EPT>& T, int e, int& k, float& lev, float& gap) {
  const int n = S.count, m = T.count;
  const float val = S.v(e);
  const int lb = T.values_below(val, true);
  k = e + lb;
  lev = S.c(e) - (lb > 0 ? T.c(lb - 1) : 0.f);
  const float nxt = fminf(e + 1 < n ? S.v(e + 1) : __builtin_inff(), lb < m ? T.v(lb) : __builtin_inff());
  gap = (nxt == __builtin_inff() ? 1.f : nxt) - val;
}

template <int EPT>
__device__ __forceinline__ void merged_target(const Side<EPT>& S, const Side<EPT>& T, int e, int& k, float& lev, float& gap) {
  const int n = S.count, m = T.count;
  const float val = T.v(e);
  const int ub = S.values_below(val, false);
  k = e + ub;
  lev = (ub > 0 ? S.c(ub - 1) : 0.f) - T.c(e);
  const float nxt = fminf(e + 1 < m ? T.v(e + 1) : __builtin_inff(), ub < n ? S.v(ub) : __builtin_inff());
  gap = (nxt == __builtin_inff() ? 1.f : nxt) - val;
}

template <int EPT>
__global__ __launch_bounds__(kPotThreads) void ssw_weight_pot_median_kernel(WeightPotArgs P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int ROW = EPT * kWave;
  constexpr int PROW = padded_floats(ROW);
  const GeneralArgs& G = P.G;
  const SswArgs& A = G.base;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const WeightPotLds<EPT> L(lds);
  const int s = xcd_contiguous_id(blockIdx.x, A.num_groups);
  if (s >= A.pairs * A.slices) return;                       // (uniform over the workgroup)
  const int n = A.n, m = A.m, total = n + m;
  load_sorted_sides<EPT>(G, s, wave, lane, L);
  const Side<EPT> S{L.s_val, L.s_cdf, n}, T{L.t_val, L.t_cdf, m};
  float* lev_k = L.work;                                     // n + m <= 2 ROW entries each, merged order
  float* gap_k = L.work + 2 * PROW;
  double lo_lev = (double)__builtin_inff(), hi_lev = -(double)__builtin_inff();
  for (int e = tid; e < max(n, m); e += kPotThreads) {
    int k;
    float lev, gap;
    if (e < n) {
      merged_source<EPT>(S, T, e, k, lev, gap);
      lev_k[pad32(k)] = lev; gap_k[pad32(k)] = gap;
      lo_lev = fmin(lo_lev, (double)lev); hi_lev = fmax(hi_lev, (double)lev);
    }
    if (e < m) {
      merged_target<EPT>(S, T, e, k, lev, gap);
      lev_k[pad32(k)] = lev; gap_k[pad32(k)] = gap;
      lo_lev = fmin(lo_lev, (double)lev); hi_lev = fmax(hi_lev, (double)lev);
    }
  }
  lo_lev = block_min(lo_lev, L.red, tid);                    // (also the barrier that publishes the merged arrays)
  hi_lev = -block_min(-hi_lev, L.red, tid);
  // the median: the smallest level whose cumulated gap weight reaches 0.5 (the smallest level if the total never does)
  auto weight_below = [&](float t) -> double {
    double w = 0.0;
    for (int k = tid; k < total; k += kPotThreads) w += lev_k[pad32(k)] <= t ? (double)gap_k[pad32(k)] : 0.0;
    return block_sum(w, L.red, tid);
  };
  float med = (float)lo_lev;
  if (weight_below((float)hi_lev) >= 0.5) {
    float lo = (float)lo_lev - 1.f, hi = (float)hi_lev;
    for (int it = 0; it < 48 && lo < hi; ++it) {
      const float mid = lo + (hi - lo) * 0.5f;
      if (!(mid > lo && mid < hi)) break;                    // bracket exhausted at fp32 resolution
      if (weight_below(mid) >= 0.5) hi = mid; else lo = mid;
    }
    double best = (double)__builtin_inff();                  // smallest level above the bracket's lower end
    for (int k = tid; k < total; k += kPotThreads) {
      const float l = lev_k[pad32(k)];
      best = l > lo ? fmin(best, (double)l) : best;
    }
    med = (float)block_min(best, L.red, tid);
  }
  double kfirst = (double)total;                             // k*: the first merged position on the median level
  for (int k = tid; k < total; k += kPotThreads) kfirst = lev_k[pad32(k)] == med ? fmin(kfirst, (double)k) : kfirst;
  const int kstar = (int)block_min(kfirst, L.red, tid);
  // g sigma in place of the gaps, then H by a suffix sum; S = H_0
  double part = 0.0;
  for (int k = tid; k < total; k += kPotThreads) {
    const float l = lev_k[pad32(k)];
    const float c = l > med ? gap_k[pad32(k)] : (l < med ? -gap_k[pad32(k)] : 0.f);
    gap_k[pad32(k)] = c;
    part += (double)c;
  }
  const double S0 = block_sum(part, L.red, tid);
  block_suffix_sum(gap_k, total, L.red, tid);
  // every atom's derivative, by sorted position, into the level rows (dead: the loop reads the clouds and H only)
  float* du = L.work;
  float* dv = L.work + PROW;
  for (int e = tid; e < max(n, m); e += kPotThreads) {
    int k;
    float lev, gap;
    if (e < n) {
      merged_source<EPT>(S, T, e, k, lev, gap);
      du[pad32(e)] = (float)((double)gap_k[pad32(k)] - (k <= kstar ? S0 : 0.0));
    }
    if (e < m) {
      merged_target<EPT>(S, T, e, k, lev, gap);
      dv[pad32(e)] = (float)((double)gap_k[pad32(k)] - (k <= kstar ? S0 : 0.0));
    }
  }
  __syncthreads();
  const int b = s / A.slices;
  if (P.pot_u)
    centre_and_store(du, n, L.idx_s, G.wu + (long)b * G.wu_pair_stride, 1.f, L.s_val, P.pot_u + (long)s * n, L.red, tid);
  if (P.pot_v)
    centre_and_store(dv, m, L.idx_t, G.wv + (long)b * G.wv_pair_stride, -1.f, L.t_val, P.pot_v + (long)s * m, L.red, tid);
}

template <int EPT>
static int launch_weight_pot_class(WeightPotArgs& P, bool median, hipStream_t stream) {
  SswArgs& A = P.G.base;
  if (!problem_groups(A.pairs, A.slices, 1, A.num_groups)) return (int)hipErrorInvalidValue;
  constexpr size_t lds = weight_pot_lds_bytes<EPT>();
  static_assert(lds <= 160 * 1024, "one workgroup's LDS fits a CU");
  const dim3 grid((unsigned)A.num_groups), block(kPotThreads);
  if (median) hipLaunchKernelGGL((ssw_weight_pot_median_kernel<EPT>), grid, block, lds, stream, P);
  else with_pmode(A.p_int, [&](auto pm) {
    hipLaunchKernelGGL((ssw_weight_pot_cut_kernel<EPT, decltype(pm)::value>), grid, block, lds, stream, P);
  });
  return (int)hipGetLastError();
}

static int launch_weight_pot(WeightPotArgs& P, bool median, hipStream_t stream) {
  switch (ept_for(P.G.base.n, P.G.base.m)) {
    case 1: return launch_weight_pot_class<1>(P, median, stream);
    case 2: return launch_weight_pot_class<2>(P, median, stream);
    case 4: return launch_weight_pot_class<4>(P, median, stream);
    case 8: return launch_weight_pot_class<8>(P, median, stream);
    case 16: return launch_weight_pot_class<16>(P, median, stream);
    case 32: return launch_weight_pot_class<32>(P, median, stream);
    case 64: return launch_weight_pot_class<64>(P, median, stream);
    default: return (int)hipErrorInvalidValue;               // > 4096 points
  }
}

static int weight_pot_entry(const float* xs, const float* xt, const float* dirs, int pstride, const float* wu, const float* wv,
                            long wu_stride, long wv_stride, int pairs, int n, int m, int slices, long u_pair_stride, float p,
                            bool median, const float* cut, float* pot_u, float* pot_v, void* stream) {
  if (!xs || !xt || (!pot_u && !pot_v)) return (int)hipErrorInvalidValue;
  if ((pot_u && !wu) || (pot_v && !wv)) return (int)hipErrorInvalidValue;      // a potential row needs its side's weights
  if (pairs < 0 || slices < 0 || n < 1 || m < 1 || n > 4096 || m > 4096 || !(p >= 1.f)) return (int)hipErrorInvalidValue;
  if (median ? p != 1.f : cut == nullptr) return (int)hipErrorInvalidValue;
  if ((wu_stride != 0 && wu_stride < n) || (wv_stride != 0 && wv_stride < m)) return (int)hipErrorInvalidValue;
  if (pairs == 0 || slices == 0) return 0;
  WeightPotArgs P{};
  SswArgs& A = P.G.base;
  A.xs = xs; A.xt = xt; A.dirs = dirs;
  A.pairs = pairs; A.n = n; A.m = m; A.slices = slices; A.u_pair_stride = u_pair_stride; A.pstride = pstride;
  A.p = p; A.p_int = small_integer_power(p);
  P.G.wu = wu; P.G.wv = wv; P.G.wu_pair_stride = wu_stride; P.G.wv_pair_stride = wv_stride;
  P.cut = cut; P.pot_u = pot_u; P.pot_v = pot_v;
  return launch_weight_pot(P, median, (hipStream_t)stream);
}

}  // namespace shw

extern "C" {

int shw_ssw_weight_potentials(const float* xs, const float* xt, const float* dirs, const float* wu, const float* wv,
                              long wu_pair_stride, long wv_pair_stride, int pairs, int n, int m, int slices,
                              long u_pair_stride, float p, const float* slice_cut, float* pot_u, float* pot_v, void* stream) {
  if (!dirs || (u_pair_stride != 0 && u_pair_stride < (long)slices * 6)) return (int)hipErrorInvalidValue;
  return shw::weight_pot_entry(xs, xt, dirs, 3, wu, wv, wu_pair_stride, wv_pair_stride, pairs, n, m, slices, u_pair_stride,
                               p, p == 1.f, slice_cut, pot_u, pot_v, stream);
}

int shw_circle_weight_potentials(const float* u, const float* v, const float* wu, const float* wv, long wu_row_stride,
                                 long wv_row_stride, int rows, int n, int m, float p, int method, const float* cut,
                                 float* pot_u, float* pot_v, void* stream) {
  if (method != SHW_CIRCLE_AS_SLICED && method != SHW_CIRCLE_BISECTION && method != SHW_CIRCLE_LEVEL_MEDIAN) return (int)hipErrorInvalidValue;
  if (method == SHW_CIRCLE_LEVEL_MEDIAN && p != 1.f) return (int)hipErrorInvalidValue;
  const bool median = p == 1.f && method != SHW_CIRCLE_BISECTION;
  return shw::weight_pot_entry(u, v, nullptr, 1, wu, wv, wu_row_stride, wv_row_stride, rows, n, m, 1, 0, p, median, cut,
                               pot_u, pot_v, stream);
}

}  // extern "C"
