// general_p1.hpp -- general circular OT, solver (c) of general_common.hpp: p == 1 with weights and / or n != m.
#pragma once
#include "general_common.hpp"

namespace shw {

// ---------------------------------------------------------------------------------------------
// p == 1 with weights: the reference's level-median formula (emd1D_circle, :210-247) on weighted atoms.
// level = CDF difference after the atom in merged-by-value order (source before target on equal values),
// gap = distance to the merged successor (the last atom: 1 - value; [0, first atom) is not integrated),
// median = smallest level whose cumulated gap weight reaches 0.5 (the smallest level if the total never does),
// cost = sum gap * |level - median|.  Levels are floats here, so the median is a float bisection followed by a
// snap to the smallest level above the bracket.  Coefficients (GRAD): |level_before - med| - |level - med|,
// the first merged atom -|level - med|.
// ---------------------------------------------------------------------------------------------
template <int EPT, bool GRAD>
__global__ __launch_bounds__(64) void ssw_general_p1_kernel(GeneralArgs G) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int ROW = EPT * kWave;
  const SswArgs& A = G.base;
  const int lane = threadIdx.x & 63;
  float* s_val = lds;
  float* s_cdf = lds + ROW;
  float* t_val = lds + 2 * ROW;
  float* t_cdf = lds + 3 * ROW;
  float* scratch = lds + 4 * ROW;
  float* lev_s = lds + 4 * ROW;                              // reuses scratch once the sorts are done
  float* gap_s = lds + 5 * ROW;
  float* lev_t = lds + 6 * ROW;
  float* gap_t = lds + 7 * ROW;

  const int s = xcd_contiguous_id(blockIdx.x, A.num_groups);
  if (s >= A.pairs * A.slices) return;
  const int n = A.n, m = A.m;
  int sidx[EPT], tidx[EPT];
  float mean_s_unused = 0.f, mean_t_unused = 0.f;
  prepare_sides<EPT>(G, s, lane, s_val, s_cdf, t_val, t_cdf, scratch, sidx, tidx, mean_s_unused, mean_t_unused);
  Side<EPT> S{s_val, s_cdf, n}, T{t_val, t_cdf, m};

  float lo_lev = __builtin_inff(), hi_lev = -__builtin_inff(), total = 0.f;
  constexpr int NA = EPT < 4 ? EPT : 4;                      // atoms searched together (see lower_bounds2)
#pragma nounroll
  for (int r0 = 0; r0 < EPT; r0 += NA) {
    float su[NA], sv[NA];
    int lt_u[NA], le_u[NA], lt_v[NA], le_v[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      su[a] = S.v(min(lane * EPT + r0 + a, n - 1));
      sv[a] = T.v(min(lane * EPT + r0 + a, m - 1));
    }
    lower_bounds2_arr<EPT, NA>(t_val, m, su, lt_u, le_u);    // source atom: target values <  it
    lower_bounds2_arr<EPT, NA>(s_val, n, sv, lt_v, le_v);    // target atom: source values <= it
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const int r = r0 + a, e = lane * EPT + r;
      if (e < n) {                                           // source atom e
        const float val = su[a];
        const int lb = lt_u[a];
        const float lev = S.c(e) - (lb > 0 ? T.c(lb - 1) : 0.f);
        const float nxt = fminf(e + 1 < n ? S.v(e + 1) : __builtin_inff(), lb < m ? T.v(lb) : __builtin_inff());
        const float gap = (nxt == __builtin_inff() ? 1.f : nxt) - val;
        lev_s[r * kWave + lane] = lev;
        gap_s[r * kWave + lane] = gap;
        lo_lev = fminf(lo_lev, lev); hi_lev = fmaxf(hi_lev, lev); total += gap;
      }
      if (e < m) {                                           // target atom e
        const float val = sv[a];
        const int ub = le_v[a];
        const float lev = (ub > 0 ? S.c(ub - 1) : 0.f) - T.c(e);
        const float nxt = fminf(e + 1 < m ? T.v(e + 1) : __builtin_inff(), ub < n ? S.v(ub) : __builtin_inff());
        const float gap = (nxt == __builtin_inff() ? 1.f : nxt) - val;
        lev_t[r * kWave + lane] = lev;
        gap_t[r * kWave + lane] = gap;
        lo_lev = fminf(lo_lev, lev); hi_lev = fmaxf(hi_lev, lev); total += gap;
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
  lo_lev = as_f(__builtin_amdgcn_readfirstlane(as_i(-wave_max(-lo_lev, lane))));
  hi_lev = as_f(__builtin_amdgcn_readfirstlane(as_i(wave_max(hi_lev, lane))));
  total = wave_sum_uniform(total, lane);

  auto weight_below = [&](float t) -> float {               // sum of gaps of atoms with level <= t
    float w = 0.f;
#pragma nounroll
    for (int r = 0; r < EPT; ++r) {
      const int e = lane * EPT + r;
      if (e < n && lev_s[r * kWave + lane] <= t) w += gap_s[r * kWave + lane];
      if (e < m && lev_t[r * kWave + lane] <= t) w += gap_t[r * kWave + lane];
    }
    return wave_sum_uniform(w, lane);
  };
  float med = lo_lev;
  if (total >= 0.5f) {
    float lo = lo_lev - 1.f, hi = hi_lev;                    // W(lo) = 0 < 0.5 <= W(hi) = total
    for (int it = 0; it < 48 && lo < hi; ++it) {
      const float mid = lo + (hi - lo) * 0.5f;
      if (!(mid > lo && mid < hi)) break;                    // bracket exhausted at fp32 resolution
      if (weight_below(mid) >= 0.5f) hi = mid; else lo = mid;
    }
    float best = __builtin_inff();                           // smallest level above the bracket's lower end
#pragma nounroll
    for (int r = 0; r < EPT; ++r) {
      const int e = lane * EPT + r;
      if (e < n) { const float l = lev_s[r * kWave + lane]; best = (l > lo) ? fminf(best, l) : best; }
      if (e < m) { const float l = lev_t[r * kWave + lane]; best = (l > lo) ? fminf(best, l) : best; }
    }
    med = as_f(__builtin_amdgcn_readfirstlane(as_i(-wave_max(-best, lane))));
  }

  float acc = 0.f;
  float* cs = GRAD ? A.coef_s + (long)s * n : nullptr;
  float* ct = GRAD ? A.coef_t + (long)s * m : nullptr;
#pragma unroll
  for (int r = 0; r < EPT; ++r) {
    const int e = lane * EPT + r;
    if (e < n) {
      const float lev = lev_s[r * kWave + lane], here = fabsf(lev - med);
      acc += gap_s[r * kWave + lane] * here;
      if constexpr (GRAD) {
        const float own = S.c(e) - (e > 0 ? S.c(e - 1) : 0.f);
        const bool first = (e == 0) && (T.values_below(S.v(0), true) == 0);
        cs[sidx[r]] = (first ? 0.f : fabsf(lev - own - med)) - here;
      }
    }
    if (e < m) {
      const float lev = lev_t[r * kWave + lane], here = fabsf(lev - med);
      acc += gap_t[r * kWave + lane] * here;
      if constexpr (GRAD) {
        const float own = T.c(e) - (e > 0 ? T.c(e - 1) : 0.f);
        const bool first = (e == 0) && (S.values_below(T.v(0), false) == 0);
        ct[tidx[r]] = (first ? 0.f : fabsf(lev + own - med)) - here;
      }
    }
  }
  const float cost = wave_sum_uniform(acc, lane);
  if (lane == 0) {
    A.slice_cost[s] = cost;
    if (G.slice_theta) G.slice_theta[s] = med;
  }
}

// ---------------------------------------------------------------------------------------------
// p == 1 with weights, >= 8 atoms per lane: the same formula as ssw_general_p1_kernel with
//   * the two cross searches (target values below a source atom, source values not above a target atom) done by
//     walking (walk_window: the lane's atoms ascend, so do their ranks in the other cloud's values; round 2);
//   * levels and gaps in REGISTERS: the median bisection reads no LDS;
//   * TWO waves per slice (round 3): wave 0 owns the source cloud, wave 1 the target -- its sort (at the same time as the
//     other's), the levels and gaps of its atoms (one walk each, at the same time, straight into registers: the loop over a
//     lane's atoms is unrolled), its share of every masked sum of the median bisection (added in wave order through LDS, one
//     barrier per step) and its coefficient row.  Round 2's one-wave kernel kept the levels and gaps of BOTH clouds in
//     registers (256 VGPRs + AGPRs, one wave per SIMD, three slices per CU): 3.3 -> 1.6 ms per loss, 3.8 -> 2.4 per
//     training step at B = 64, n = m = 2048, L = 512; the loss-only form needs no staging rows (4 slices per CU);
//   * coefficients un-permuted through LDS and stored coalesced.
// ---------------------------------------------------------------------------------------------
template <int EPT, int C, bool SRC>
__device__ __forceinline__ int p1_levels_walk_regs(const Side<EPT>& O, const Side<EPT>& X, int lane, float (&lev_out)[EPT],
                                                   float (&gap_out)[EPT]) {
  constexpr int P = EPT * kWave;
  constexpr int LEN = EPT / C;
  const int no = O.count, nx = X.count;
  const float inf = __builtin_inff();
  int ptr[C];
  float prev[C], own_v[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int e0 = lane * EPT + c * LEN;
    own_v[c] = O.val[lds_slot<EPT>(min(e0, P - 1))];
    prev[c] = O.val[lds_slot<EPT>(min(e0, no - 1))];
    ptr[c] = lower_bound_arr<EPT>(X.val, nx, prev[c]);
  }
  int first_rank = 0;
#pragma unroll
  for (int i = 0; i < LEN; ++i) {
    float k[C], val[C], nxt_own[C];
    bool live[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int e = lane * EPT + c * LEN + i;
      live[c] = e < no;
      val[c] = own_v[c];
      own_v[c] = e + 1 < P ? O.val[lds_slot<EPT>(min(e + 1, P - 1))] : inf;   // dead values are +inf in the row
      nxt_own[c] = own_v[c];
      k[c] = live[c] ? val[c] : prev[c];
      prev[c] = k[c];
    }
    int le[C];
    walk_window<EPT, C>(X.val, nx, k, ptr, le);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int e = lane * EPT + c * LEN + i;
      const int rank = SRC ? ptr[c] : le[c];
      if (i == 0 && c == 0) first_rank = rank;
      const float below = rank > 0 ? X.c(rank - 1) : 0.f;
      const float mine = O.c(min(e, no - 1));
      const float lev = SRC ? mine - below : below - mine;
      const float cross = rank < nx ? X.v(min(rank, P - 1)) : inf;
      const float nxt = fminf(nxt_own[c], cross);
      const float gap = (nxt == inf ? 1.f : nxt) - val[c];
      lev_out[c * LEN + i] = live[c] ? lev : inf;
      gap_out[c * LEN + i] = live[c] ? gap : 0.f;
    }
  }
  return first_rank;
}

template <int EPT, bool GRAD>
__global__ __launch_bounds__(128, 2) void ssw_general_p1_walk2_kernel(GeneralArgs G) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int ROW = EPT * kWave, EXT = kWalkExt * kWave;
  constexpr int C = 2;
  const SswArgs& A = G.base;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float* s_val = lds;                                        // each value row with its window rows
  float* t_val = s_val + ROW + EXT;
  float* s_cdf = t_val + ROW + EXT;
  float* t_cdf = s_cdf + ROW;
  float* stage = t_cdf + ROW;                                // GRAD only: [2][ROW] coefficients by original index
  float* team_mem = stage + (GRAD ? 2 * ROW : 0);
  SliceTeam<2> team{team_mem, wave, 0};
  float* shared = team_mem + 16;                             // [0..3] minima / maxima of the two waves

  const int s = xcd_contiguous_id(blockIdx.x, A.num_groups);
  if (s >= A.pairs * A.slices) return;
  const int n = A.n, m = A.m;
  const bool src = wave == 0;                                // wave 0: the source cloud, wave 1: the target
  int oidx[EPT];
  {
    float mean_unused;
    float* dval = src ? s_val : t_val;
    float* dcdf = src ? s_cdf : t_cdf;
    // the wave's own rows serve as its sort scratch (see ssw_general_kernel)
    prepare_one<EPT, false>(G, s, lane, src ? 1 : 0, dval, dcdf, dval, reinterpret_cast<unsigned*>(dcdf), oidx, mean_unused);
    fill_walk_ext<EPT>(dval, lane);
  }
  __syncthreads();
  Side<EPT> S{s_val, s_cdf, n}, T{t_val, t_cdf, m};
  const Side<EPT>& O = src ? S : T;                          // own cloud
  const int no = src ? n : m;

  float lev[EPT], gap[EPT];
  int rank0;
  if (src) rank0 = p1_levels_walk_regs<EPT, C, true>(S, T, lane, lev, gap);
  else rank0 = p1_levels_walk_regs<EPT, C, false>(T, S, lane, lev, gap);

  const float inf = __builtin_inff();
  float lo_lev = inf, hi_lev = -inf, total = 0.f;
#pragma unroll
  for (int r = 0; r < EPT; ++r) {
    lo_lev = fminf(lo_lev, lev[r]);
    hi_lev = fmaxf(hi_lev, lev[r] < inf ? lev[r] : -inf);
    total += gap[r];
  }
  lo_lev = -wave_max(-lo_lev, lane);
  hi_lev = wave_max(hi_lev, lane);
  if (lane == 0) { shared[wave] = lo_lev; shared[2 + wave] = hi_lev; }
  float sums[1] = {wave_sum_uniform(total, lane)};
  team.sum(sums, lane);                                      // (its barrier also publishes the minima / maxima)
  total = sums[0];
  lo_lev = as_f(__builtin_amdgcn_readfirstlane(as_i(fminf(shared[0], shared[1]))));
  hi_lev = as_f(__builtin_amdgcn_readfirstlane(as_i(fmaxf(shared[2], shared[3]))));

  auto weight_below = [&](float t) -> float {               // sum of gaps of the slice's atoms with level <= t
    float w = 0.f;
#pragma unroll
    for (int r = 0; r < EPT; ++r) w += (lev[r] <= t) ? gap[r] : 0.f;
    float sw[1] = {wave_sum_uniform(w, lane)};
    team.sum(sw, lane);
    return sw[0];
  };
  float med = lo_lev;
  if (total >= 0.5f) {
    float lo = lo_lev - 1.f, hi = hi_lev;                    // W(lo) = 0 < 0.5 <= W(hi) = total
    for (int it = 0; it < 48 && lo < hi; ++it) {
      const float mid = lo + (hi - lo) * 0.5f;
      if (!(mid > lo && mid < hi)) break;                    // bracket exhausted at fp32 resolution
      if (weight_below(mid) >= 0.5f) hi = mid; else lo = mid;
    }
    float best = inf;                                        // smallest level above the bracket's lower end
#pragma unroll
    for (int r = 0; r < EPT; ++r) best = (lev[r] > lo) ? fminf(best, lev[r]) : best;
    best = -wave_max(-best, lane);
    __syncthreads();                                         // (everyone has read the minima of the first exchange)
    if (lane == 0) shared[wave] = best;
    __syncthreads();
    med = as_f(__builtin_amdgcn_readfirstlane(as_i(fminf(shared[0], shared[1]))));
  }

  float acc = 0.f;
#pragma unroll
  for (int r = 0; r < EPT; ++r) {
    const int e = lane * EPT + r;
    if (e < no) {
      const float here = fabsf(lev[r] - med);
      acc += gap[r] * here;
      if constexpr (GRAD) {
        const float own = O.c(e) - (e > 0 ? O.c(e - 1) : 0.f);
        const bool first = (e == 0) && (rank0 == 0);         // no atom of the other cloud before (source) / at or before it
        // source: the level before the atom's own weight is lev - own; target: lev + own
        const float before = src ? lev[r] - own : lev[r] + own;
        stage[(src ? 0 : ROW) + oidx[r]] = (first ? 0.f : fabsf(before - med)) - here;
      }
    }
  }
  float cs1[1] = {wave_sum_uniform(acc, lane)};
  team.sum(cs1, lane);                                       // (GRAD: its barrier also publishes the staging rows)
  if (threadIdx.x == 0) {
    A.slice_cost[s] = cs1[0];
    if (G.slice_theta) G.slice_theta[s] = med;
  }
  if constexpr (GRAD) {
    float* cs = A.coef_s + (long)s * n;
    float* ct = A.coef_t + (long)s * m;
    for (int i = (int)threadIdx.x; i < max(n, m); i += 128) {
      if (i < n) cs[i] = stage[i];
      if (i < m) ct[i] = stage[ROW + i];
    }
  }
}

}  // namespace shw
