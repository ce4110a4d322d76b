// general_grid.hpp -- general circular OT, solver (a) of general_common.hpp: no weights, n != m, p != 1.
#pragma once
#include "general_common.hpp"

namespace shw {

// ---------------------------------------------------------------------------------------------
// No weights, n != m (round 3): the solve on the INTEGER grid of lcm(n, m).
//
// With masses 1/n and 1/m every CDF level is a multiple of 1/G, G = lcm(n, m) = a n = b m.  Cut the unit of mass into G
// cells: cell q belongs to source atom q / a, and -- after moving mass k / G around the circle -- to the extended target
// atom (q + k) / b (floor division; vx(t) = v[t mod m] + floor(t / m)).  The reference's Cost (:68-113) at theta = k / G is
//     c(k) = (1/G) sum_q | u[q / a] - vx((q + k) / b) |^p ,
// it is linear between grid points (both quantile functions are step functions whose steps sit on the grid), so the
// bisection of binary_search_circle (:117-207) converges to  min_k c(k),  a convex sequence -- the same statement as row
// A8 of SURVEY 8a, which is its special case a = b = 1.  Everything here is exact integer index arithmetic: no CDF
// arrays, no searches, no rounding questions about coinciding levels (round 2 evaluated the same thing with closed-form
// float ranks: ~100 VALU per atom and evaluation, a divergent tie path for every third atom when n and m share a factor).
//   * slope:  c(k+1) - c(k) = (1/G) sum over the m cells q = t b - k - 1 whose target atom changes, of
//             |u[q/a] - vx(t)|^p - |u[q/a] - vx(t-1)|^p   (the reference's dCost, :59-63).  One pass gives the forward
//             difference dp at k, the backward difference dm (= dp at k - 1) and how far k can move either way before
//             any term's source atom changes (the distance to the next kink of the sequence).
//   * search: secant / Illinois on the slope from k0 = round(G (mean u - mean v)) (exact for p = 2 and evenly spread
//             targets), every evaluation moving the bracket at least to the next kink; ends when dm <= 0 <= dp.
//   * cost and gradient at k*: every source atom walks the <= a/b + 2 target atoms that share cells with it (and every
//             target atom its sources): each coefficient is accumulated by its owner and written once.
// ---------------------------------------------------------------------------------------------
// q = floor(x / d), r = x - q d for 0 <= x < 2^24, 1 <= d, quotient < 2^13 (indices of atoms): the fp32 quotient is
// within one of the answer (x is exact in fp32, the quotient's error is < 2^13 * 2^-22), one correction each way
__device__ __forceinline__ void div_small(int x, int d, float inv_d, int& q, int& r) {
  q = (int)((float)x * inv_d);
  r = x - q * d;
  if (r < 0) { r += d; --q; }
  if (r >= d) { r -= d; ++q; }
}

// k = q d + r with 0 <= r < d for |k| < 2^24 (floor division)
__device__ __forceinline__ void floor_divmod(int k, int d, float inv_d, int& q, int& r) {
  int qa, ra;
  div_small(k < 0 ? -k : k, d, inv_d, qa, ra);
  q = k < 0 ? -qa - (ra > 0 ? 1 : 0) : qa;
  r = (k < 0 && ra > 0) ? d - ra : ra;
}

__device__ __forceinline__ int floor_div_m(int x, int m) {          // x in [-m, 2m)
  return x < 0 ? -1 : (x >= m ? 1 : 0);
}

struct Grid {
  int n, m, G, a, b;
  float inv_a, inv_b;
};

// forward / backward differences of G c(k) at k and the distances to the neighbouring kinks; uniform over the slice
template <int EPT, int PMODE, int W>
__device__ void grid_slopes(const float* s_val, const float* t_val, const Grid& gr, int k, int lane, int tid, float p, int p_int,
                            SliceTeam<W>& team, float& dm, float& dp, int& gap_left, int& gap_right) {
  constexpr int AP = EPT / W;
  const int a = gr.a, b = gr.b, n = gr.n, m = gr.m;
  int kb, krem;                                                    // k = kb b + krem, 0 <= krem < b
  floor_divmod(k, b, gr.inv_b, kb, krem);
  const int s1 = krem == 0 ? 1 : 0;                                // dp's cells sit one target atom further when b | k
  const int t_base = krem == 0 ? kb : kb + 1;                      // ceil(k / b)
  const int j0 = tid * AP;
  // atom j: t = t_base + j;  dm's cell q1 = t b - k,  dp's cell q2 = (t + s1) b - k - 1;  0 <= q < G for j < m
  const int q1 = min((t_base + j0) * b - k, gr.G - 1);             // (threads past the last atom: clamped, masked below)
  int i1, r1, i2, r2, bh, bl;
  div_small(q1, a, gr.inv_a, i1, r1);
  div_small(max(q1 + s1 * b - 1, 0), a, gr.inv_a, i2, r2);
  div_small(b, a, gr.inv_a, bh, bl);
  float vm = target_unrolled<EPT>(t_val, min(t_base + j0 - 1, 3 * m - 1), m);
  float v0 = target_unrolled<EPT>(t_val, min(t_base + j0, 3 * m - 1), m);
  float sm = 0.f, sp = 0.f;
  int gl = 0x7fffffff, grt = 0x7fffffff;
#pragma unroll 4
  for (int r = 0; r < AP; ++r) {
    const bool live = (j0 + r) < m;
    const float vp = target_unrolled<EPT>(t_val, min(t_base + j0 + r + 1, 3 * m - 1), m);
    const float um = s_val[lds_slot<EPT>(min(i1, n - 1))];
    const float up = s_val[lds_slot<EPT>(min(i2, n - 1))];
    const float hi = s1 ? vp : v0, lo = s1 ? v0 : vm;
    const float tm = powp<PMODE>(um - v0, p, p_int) - powp<PMODE>(um - vm, p, p_int);
    const float tp = powp<PMODE>(up - hi, p, p_int) - powp<PMODE>(up - lo, p, p_int);
    sm += live ? tm : 0.f;
    sp += live ? tp : 0.f;
    gl = live ? min(gl, a - r1) : gl;
    grt = live ? min(grt, r2 + 1) : grt;
    vm = v0; v0 = vp;
    r1 += bl; i1 += bh;
    if (r1 >= a) { r1 -= a; ++i1; }
    r2 += bl; i2 += bh;
    if (r2 >= a) { r2 -= a; ++i2; }
  }
  float sums[2] = {wave_sum_uniform(sm, lane), wave_sum_uniform(sp, lane)};
  // (distances are <= max(a, b) <= 4096: exact in fp32)
  float mins[2] = {-wave_max(-(float)min(gl, 1 << 23), lane), -wave_max(-(float)min(grt, 1 << 23), lane)};
  mins[0] = as_f(__builtin_amdgcn_readfirstlane(as_i(mins[0])));
  mins[1] = as_f(__builtin_amdgcn_readfirstlane(as_i(mins[1])));
  team.sum2_min2(sums, mins, lane);
  dm = sums[0];
  dp = sums[1];
  gap_left = (int)mins[0];
  gap_right = (int)mins[1];
}

// minimiser k* of the convex sequence c(k), |k| <= G (theta in [-1, 1], :174-177); uniform over the slice
// (evals: the evaluations spent.  No caller reads it, but the loss-only kernels compile to other code without the
//  counter -- profiles/r11_general_split.txt -- and their bytes are the proof that this unit computes what it did.)
template <int EPT, int PMODE, int W>
__device__ int grid_solve(const float* s_val, const float* t_val, const Grid& gr, float mean_s, float mean_t, int lane, int tid,
                          float p, int p_int, SliceTeam<W>& team, int& evals) {
  const float Gf = (float)gr.G;
  int lo = -gr.G, hi = gr.G;
  float guess = rintf((mean_s - mean_t) * Gf);
  if (!(guess >= (float)lo)) guess = (float)lo;                     // (also non-finite input)
  if (!(guess <= (float)hi)) guess = (float)hi;
  int k = __builtin_amdgcn_readfirstlane((int)guess);
  int k_neg = 0, k_pos = 0, k_prev = 0, last_side = 0, secant_steps = 0;
  float f_neg = 0.f, f_pos = 0.f, f_prev = 0.f, step = 1.f;
  bool have_neg = false, have_pos = false, have_prev = false;
  evals = 0;
  for (int it = 0; it < kMaxEvals; ++it) {
    float dm, dp;
    int gl, grt;
    grid_slopes<EPT, PMODE, W>(s_val, t_val, gr, k, lane, tid, p, p_int, team, dm, dp, gl, grt);
    ++evals;
    const bool right = (dp < 0.f) && (k < hi);
    const bool left = !right && (dm > 0.f) && (k > lo);
    if (!right && !left) break;                                    // dm <= 0 <= dp: k is a minimiser (:186-187)
    const float f = right ? dp : dm;
    if (right) {
      lo = min(k + max(grt, 1), hi);                               // the slope cannot change before the next kink
      k_neg = k; f_neg = dp; have_neg = true;
      if (last_side > 0 && have_pos) f_pos *= 0.5f;                // Illinois: the end that stays put loses weight
      last_side = 1;
    } else {
      hi = max(k - max(gl, 1), lo);
      k_pos = k; f_pos = dm; have_pos = true;
      if (last_side < 0 && have_neg) f_neg *= 0.5f;
      last_side = -1;
    }
    if (lo >= hi) { k = lo; break; }                               // one candidate left: the minimiser
    float next;
    if (have_neg && have_pos) {
      const float w = (float)(k_pos - k_neg);
      next = (float)k_neg + rintf(w * (-f_neg) / (f_pos - f_neg));
      if (!(next >= (float)lo && next <= (float)hi) || ++secant_steps > 24) next = (float)(lo + ((hi - lo) >> 1));
    } else {
      // p = 2: G c is ~quadratic in theta = k / G with curvature ~2 for clouds spread around the circle
      if (PMODE == 2 && !have_prev) step = fmaxf(step, 0.5f * fabsf(f) * Gf);
      next = (float)k + (right ? step : -step);
      if (have_prev && (f - f_prev) * (float)(k - k_prev) > 0.f) {
        const float root = (float)k - f * (float)(k - k_prev) / (f - f_prev);
        const float over = (float)k + 1.25f * (root - (float)k);
        next = right ? fmaxf(next, over) : fminf(next, over);
      }
      step *= 2.f;
    }
    next = fminf(fmaxf(rintf(next), (float)lo), (float)hi);
    k_prev = k; f_prev = f; have_prev = true;
    k = __builtin_amdgcn_readfirstlane((int)next);
  }
  return k;
}

// G * Cost at the shift k, the thread's share (sum over its source atoms); GRAD: G * d Cost / d (sorted source atom) into gs
template <int EPT, int PMODE, bool GRAD, int W>
__device__ float grid_cost_source(const float* s_val, const float* t_val, const Grid& gr, int k, int tid, float p, int p_int,
                                  float* gs) {
  constexpr int AP = EPT / W;
  const int a = gr.a, b = gr.b, n = gr.n, m = gr.m;
  const int trips = (a + b - 2) / b + 1;                           // a source atom's a cells meet at most this many targets
  float cost = 0.f;
  int e = tid * AP;
  // cells [e a, (e+1) a): the first one belongs to target t = floor((e a + k) / b), rb cells into it
  int kb, krem, t, rb, ah, al;
  floor_divmod(k, b, gr.inv_b, kb, krem);
  div_small(min(e, n - 1) * a + krem, b, gr.inv_b, t, rb);         // (< G + b <= 2^24)
  t += kb;
  div_small(a, b, gr.inv_b, ah, al);
#pragma nounroll
  for (int r = 0; r < AP; ++r, ++e) {
    const bool live = e < n;
    const float u = s_val[lds_slot<EPT>(min(e, n - 1))];
    float acc = 0.f, part = 0.f;
    int left = a, tt = t, off = rb;
    for (int s = 0; s < trips; ++s) {
      const int len = min(left, b - off);                          // cells shared with target tt (0 once the atom is used up)
      const float d = u - target_unrolled<EPT>(t_val, min(tt, 3 * m - 1), m);
      part = fmaf((float)len, powp<PMODE>(d, p, p_int), part);
      if constexpr (GRAD) acc = fmaf((float)len, dpow_abs<PMODE>(d, p, p_int), acc);
      left -= len;
      off = 0;
      ++tt;
    }
    cost += live ? part : 0.f;
    if constexpr (GRAD) {
      if (live) gs[lds_slot<EPT>(e)] = acc;
    }
    rb += al; t += ah;
    if (rb >= b) { rb -= b; ++t; }
  }
  return cost;
}

// GRAD: G * d Cost / d (sorted target atom) into gt.  Thread tid owns the extended target atoms T0 + [tid AP, (tid+1) AP),
// T0 = floor(k / b); when b does not divide k the first of them holds only part of its cells and the rest sit one turn
// later at T0 + m -- the owner of the last atom walks that instance too and hands its sum over in *tail (it belongs to
// sorted atom T0 mod m, which adds it to its own part: a fixed order).
template <int EPT, int PMODE, int W>
__device__ void grid_grad_target(const float* s_val, const float* t_val, const Grid& gr, int k, int tid, float p, int p_int,
                                 float* gt, float* tail) {
  constexpr int AP = EPT / W;
  const int a = gr.a, b = gr.b, n = gr.n, m = gr.m, G = gr.G;
  const int trips = (a + b - 2) / a + 1;                           // a target atom's b cells meet at most this many sources
  int T0, krem;
  floor_divmod(k, b, gr.inv_b, T0, krem);                          // T0 = floor(k / b)
  const int rho0 = tid * AP;
  const bool owns_tail = rho0 < m && rho0 + AP >= m;               // owner of the last extended atom
  const int rho_end = owns_tail ? m + 1 : min(rho0 + AP, m);
  int j = T0 + rho0;                                               // sorted atom of instance rho: (T0 + rho) mod m
  j += j < 0 ? m : 0;
  j -= j >= m ? m : 0;
  j -= j >= m ? m : 0;
#pragma nounroll
  for (int rho = rho0; rho < rho_end; ++rho) {
    const int t = T0 + rho;
    const float v = target_unrolled<EPT>(t_val, t, m);             // t in [-m, 2m]
    const int q_lo = max(t * b - k, 0);
    const int q_hi = min((t + 1) * b - k, G);                      // (rho = m with b | k: no cells, the sum is 0)
    int i, ra;
    div_small(min(q_lo, G - 1), a, gr.inv_a, i, ra);
    int left = max(q_hi - q_lo, 0);
    float acc = 0.f;
    for (int s = 0; s < trips; ++s) {
      const int len = min(left, a - ra);
      const float d = s_val[lds_slot<EPT>(min(i, n - 1))] - v;
      acc = fmaf((float)len, dpow_abs<PMODE>(d, p, p_int), acc);
      left -= len;
      ra = 0;
      ++i;
    }
    if (rho < m) gt[lds_slot<EPT>(j)] = -acc;
    else *tail = -acc;
    ++j;
    j -= j >= m ? m : 0;
  }
}

}  // namespace shw
