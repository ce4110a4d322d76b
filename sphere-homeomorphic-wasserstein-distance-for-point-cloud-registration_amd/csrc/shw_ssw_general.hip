// shw_ssw_general.hip -- general circular OT for p != 1: different sizes (n != m) and/or non-uniform
// weights.  One wavefront per (pair, slice), like the fast kernels, but the solve follows the
// reference's algorithm step for step instead of the equal-size shortcut:
//
//   binary_search_circle (max_spherical_sliced_w.py:117-207): bisection over the cut theta in [-1, 1]
//   on the sign of the one-sided derivatives dCost (:25-65); exit when dC+ * dC- <= 0 or, once the
//   bracket is narrower than eps/L = 1e-7, through the tangent intersection (:189-200); the value is
//   Cost(theta) (:68-113), whose gradient w.r.t. the atoms is the loss gradient (theta is detached).
//
// Both sorted clouds live in LDS as (value, CDF) arrays.  The reference materialises the rotated
// target arrays, a merged CDF grid and a 2N sort per Cost call; here every atom locates itself in the
// other cloud's CDF by binary search (the rotated target CDF is evaluated on the fly, with the same
// fp32 operations the reference applies to v_cdf: subtract frac(theta), add 1 where negative), so one
// Cost / dCost evaluation is n + 2m independent searches and nothing is re-sorted.
//
// This is the compatibility path (~10x the work of the equal-size kernel): the trainers' "different
// source / target density" option (train_W_COS.py:292-293,334-336) and the u_weights / v_weights
// arguments (:289) land here.
//
// Round 3: W wavefronts of one workgroup share a slice (W = 2 from 1024 points on, 4 at 4096).  The LDS arrays are the
// slice's, so W waves per slice put W times the waves on a CU without another byte of LDS (round 2 ran ONE wave per
// SIMD at n = 2048 with weights: 7.5 clocks per instruction of a dependent chain).  Wave 0 sorts the source while wave 1
// sorts the target; every evaluation of the solve is split by atoms (thread t of the slice owns sorted atoms
// [t AP, (t+1) AP), AP = EPT / W) and its partial sums are added in wave order through LDS, so all waves take the same
// decisions.  Gradients are OWNER-COMPUTED: every sorted atom's coefficient is accumulated in registers by one thread
// that walks the merged CDF grid over the atom's own mass interval, and written once -- no zero fill, no float
// atomics, bit-identical from run to run like the reference's autograd on the CPU.
//
// The three solvers are headers of this unit (general_common.hpp lists them); here: the kernel of forms (a) and (b), and
// the launches of all three.
#include "general_grid.hpp"
#include "general_cut.hpp"
#include "general_p1.hpp"

namespace shw {

template <int EPT, int PMODE, bool GRAD, bool UNIFORM, int W>
__global__ __launch_bounds__(64 * W, W > 1 ? (UNIFORM ? SHW_GENERAL_MINW_UNIFORM : 2) : 1) void ssw_general_kernel(GeneralArgs G) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int ROW = EPT * kWave;
  constexpr int AP = EPT / W;                                // sorted atoms per thread in the evaluations
  static_assert(EPT % W == 0 && AP >= 1, "atoms split evenly over the slice's threads");
  const SswArgs& A = G.base;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int tid = wave * kWave + lane;                       // thread of the slice: owns sorted atoms [tid AP, (tid+1) AP)
  // rows: sorted values of both clouds, their CDFs (weighted only), coordinates by original index (later the
  // source gradient row), target gradient row (GRAD only)
  float* s_val = lds;
  float* t_val = lds + ROW;
  constexpr int EXT = (UNIFORM ? 0 : general_ext_floats<EPT>());     // window rows under the source CDF (fill_walk_ext)
  float* s_cdf = UNIFORM ? nullptr : lds + 2 * ROW;
  float* t_cdf = UNIFORM ? nullptr : lds + 3 * ROW + EXT;
  float* grad_rows = lds + (UNIFORM ? 2 : 4) * ROW + EXT;    // GRAD only: two rows of coefficients by sorted position
  float* gs = grad_rows;
  float* gt = grad_rows + ROW;
  float* team_mem = lds + ((UNIFORM ? 2 : 4) + (GRAD ? 2 : 0)) * ROW + EXT;
  SliceTeam<W> team{team_mem, wave, 0};
  float* shared = team_mem + 8 * W;                          // [0], [1]: the two mean coordinates; [2]: the tail coefficient

  const int s = xcd_contiguous_id(blockIdx.x, A.num_groups);
  if (s >= A.pairs * A.slices) return;                       // (uniform over the workgroup)
  const int n = A.n, m = A.m;
  // sorted -> original index maps.  One wave per slice: [0] target, [1] source.  W waves: wave 0 sorts the source and
  // wave 1 the target at the same time, each keeps its own cloud's map in [0].
  constexpr int NI = W == 1 ? 2 : 1;
  int oidx[NI][EPT];
  float mean_s = 0.f, mean_t = 0.f;
  float handed_cut = 0.f;
  const bool from_indices = GRAD && UNIFORM && G.idx_handoff;
  if (from_indices) handed_cut = A.coef_t[(long)s * m + (m - 1)];   // read before the rows are reused
  if constexpr (W == 1) {
    if (from_indices) {
      prepare_one_from_indices<EPT>(G, s, lane, 0, t_val, oidx[0]);
      prepare_one_from_indices<EPT>(G, s, lane, 1, s_val, oidx[NI - 1]);
    } else {
      // sort counters (32 EPT words, weighted only): the source CDF row, which is written after both sorts' scatters;
      // loss only: the coordinates-by-original-index row of the sorts shares the source row
      unsigned* counters = reinterpret_cast<unsigned*>(s_cdf);
      float* scratch = GRAD ? gs : s_val;
#pragma nounroll
      for (int which = 0; which < 2; ++which) {
        float mean;
        int idx[EPT];
        prepare_one<EPT, UNIFORM>(G, s, lane, which, which == 0 ? t_val : s_val, which == 0 ? t_cdf : s_cdf, scratch,
                                  counters, idx, mean);
        if (which == 0) {
          mean_t = mean;
#pragma unroll
          for (int r = 0; r < EPT; ++r) oidx[0][r] = idx[r];
        } else {
          mean_s = mean;
#pragma unroll
          for (int r = 0; r < EPT; ++r) oidx[NI - 1][r] = idx[r];
        }
      }
    }
  } else {
    if (wave < 2) {
      const int which = 1 - wave;                            // wave 0: source, wave 1: target
      float* dval = which == 0 ? t_val : s_val;
      float* dcdf = which == 0 ? t_cdf : s_cdf;
      if (from_indices) {
        prepare_one_from_indices<EPT>(G, s, lane, which, dval, oidx[0]);
      } else {
        float mean;
        // each wave's own rows serve as its sort scratch: the value row takes the coordinates by original index, the
        // CDF row the counters; both are written with their final contents after the wave's gather
        // (without weights the sorts stay on the network: the distribution sort with indices needs half a row of counters
        //  per cloud -- 24 instead of 16 KB per slice -- and measured 2.06 against 1.79 ms at 2048 vs 1536 points)
        prepare_one<EPT, UNIFORM>(G, s, lane, which, dval, dcdf, dval, reinterpret_cast<unsigned*>(dcdf), oidx[0], mean);
        if (lane == 0) shared[which == 0 ? 1 : 0] = mean;
      }
    }
    __syncthreads();
    mean_s = shared[0];
    mean_t = shared[1];
  }
  if (!GRAD && G.idx_handoff) {                              // solve launch: leave the permutations for the gradient launch
    unsigned short* ps = reinterpret_cast<unsigned short*>(G.cut_scratch + (long)s * n);
    unsigned short* pt = reinterpret_cast<unsigned short*>(G.cut_scratch_t + (long)s * m);
    if (W == 1 || wave < 2) {
#pragma unroll
      for (int r = 0; r < EPT; ++r) {
        const int e = lane * EPT + r;
        if constexpr (W == 1) {
          if (e < n) ps[e] = (unsigned short)oidx[NI - 1][r];
          if (e < m) pt[e] = (unsigned short)oidx[0][r];
        } else {
          if (wave == 0 && e < n) ps[e] = (unsigned short)oidx[0][r];
          if (wave == 1 && e < m) pt[e] = (unsigned short)oidx[0][r];
        }
      }
    }
  }

  if constexpr (UNIFORM) {
    // ---- no weights: the solve on the integer grid of lcm(n, m) (grid_* above) ------------------------------------
    const Grid gr{n, m, G.lcm, G.lcm_a, G.lcm_b, 1.f / (float)G.lcm_a, 1.f / (float)G.lcm_b};
    const float inv_G = 1.f / (float)gr.G;
    int k;
    if constexpr (GRAD) {
      // (the gradient launch never solves: launch_general runs the loss-only kernel first, which hands the shift over as
      //  the bits of an int in the slice's own coefficient row)
      k = __float_as_int(G.idx_handoff ? handed_cut : G.cut_scratch[(long)s * G.cut_stride]);
    } else {
      int evals;                                             // (unread: see grid_solve)
      k = grid_solve<EPT, PMODE, W>(s_val, t_val, gr, mean_s, mean_t, lane, tid, A.p, A.p_int, team, evals);
      // (index hand-off: the 16-bit permutation takes the first half of the target row, the shift its last word; m >= 2)
      if (G.idx_handoff) { if (tid == 0) G.cut_scratch_t[(long)s * m + (m - 1)] = __int_as_float(k); }
      else if (G.cut_scratch && tid == 0) G.cut_scratch[(long)s * G.cut_stride] = __int_as_float(k);
    }
    float sums[1] = {wave_sum_uniform(grid_cost_source<EPT, PMODE, GRAD, W>(s_val, t_val, gr, k, tid, A.p, A.p_int, gs), lane)};
    if constexpr (GRAD) grid_grad_target<EPT, PMODE, W>(s_val, t_val, gr, k, tid, A.p, A.p_int, gt, shared + 2);
    team.sum(sums, lane);                                    // (W > 1: also the barrier that publishes gs, gt, tail)
    if (tid == 0) {
      A.slice_cost[s] = sums[0] * inv_G;
      if (G.slice_theta) G.slice_theta[s] = (float)k * inv_G;
    }
    if constexpr (GRAD) {
      if constexpr (W == 1) __builtin_amdgcn_wave_barrier();
      // un-permute through LDS (the value rows are dead now -- every wave is past its loops) and store coalesced
      const float tail = shared[2];
      int jstart, unused;
      floor_divmod(k, gr.b, gr.inv_b, jstart, unused);        // floor(k / b): its atom owns the tail
      jstart -= floor_div_m(jstart, m) * m;
      float* by_index_s = s_val;
      float* by_index_t = t_val;
      if (W == 1 || wave == 0) {
#pragma unroll
        for (int r = 0; r < EPT; ++r) {
          const int e = lane * EPT + r;
          if (e < n) by_index_s[oidx[NI - 1][r]] = gs[r * kWave + lane] * inv_G;
        }
      }
      if (W == 1 || wave == 1) {
#pragma unroll
        for (int r = 0; r < EPT; ++r) {
          const int e = lane * EPT + r;
          // (the atom of the first extended instance also owns the cells one turn later: own part first, then the tail)
          if (e < m) by_index_t[oidx[0][r]] = (gt[r * kWave + lane] + (e == jstart ? tail : 0.f)) * inv_G;
        }
      }
      if constexpr (W > 1) __syncthreads(); else __builtin_amdgcn_wave_barrier();
      float* cs = A.coef_s + (long)s * n;
      float* ct = A.coef_t + (long)s * m;
      for (int i = tid; i < max(n, m); i += kWave * W) {
        if (i < n) cs[i] = by_index_s[i];
        if (i < m) ct[i] = by_index_t[i];
      }
    }
  } else {
  Side<EPT> S{s_val, s_cdf, n}, T{t_val, t_cdf, m};
  if constexpr (general_walks<EPT>()) {
    if (wave == 0) fill_walk_ext<EPT>(s_cdf, lane);
    if constexpr (W > 1) __syncthreads(); else __builtin_amdgcn_wave_barrier();
  }

  // ---- the cut: minimiser of the convex, piecewise LINEAR cost over theta in [-1, 1] -------------------
  // The reference bisects [-1, 1] from theta = 0 on the sign of dCost until the bracket is below eps/L = 1e-7,
  // then intersects the two end tangents (:174-205): ~27 derivative evaluations.  Same exits here (kink:
  // dC+ * dC- <= 0; tangent intersection), but the bracket is grown around a first guess instead of halved
  // from [-1, 1]: moving the cut by theta moves every target atom by theta, so for p = 2 the optimum is the
  // difference of the mean coordinates (up to the kink spacing) and for other p it is near it; the search
  // steps out from there (doubling) until dCost changes sign, then bisects.  Both quantile functions are step
  // functions, so the cost is linear between kinks, and once the bracket is narrower than the smallest kink
  // spacing (G.min_width: the reference's eps/L = 1e-7) it holds at most one kink and the tangent intersection IS the
  // minimiser.  (Clouds without weights do not come here: the integer grid above.)
  float t_mid = 0.f;
  if constexpr (GRAD) {
    // the gradient launch never solves: launch_general always runs the loss-only kernel first and hands the cut over
    // (cut_given = 1) -- keeping the search out of this instantiation keeps its registers for the walks
    t_mid = G.idx_handoff ? handed_cut : G.cut_scratch[(long)s * G.cut_stride];
  } else {
    float t_lo = -1.f, t_hi = 1.f;
    t_mid = fminf(fmaxf(mean_s - mean_t, -1.f), 1.f);
    if (!(t_mid >= -1.f)) t_mid = 0.f;                         // non-finite input
    bool lo_tight = false, hi_tight = false;
    float step = G.first_step, dp_lo = 0.f, dm_hi = 0.f;
    float f_lo = 0.f, f_hi = 0.f, t_prev = 0.f, f_prev = 0.f;  // secant state (weighted clouds)
    constexpr int kChains = AP >= SHW_GENERAL_CHAINS ? SHW_GENERAL_CHAINS : AP;
    int anchors[kChains] = {};                                 // first ranks of the previous evaluation (cut_slopes_walk)
    float cost_scale = 0.f;                                    // size of the cost (cut_slopes_walk)
    int last_side = 0, secant_steps = 0;
    bool have_prev = false;
    for (int it = 0; it < kMaxEvals; ++it) {                   // <= ~25 doublings + ~25 halvings
      float dp, dm;
      if constexpr (!general_walks<EPT>()) {
        cut_slopes<EPT, PMODE, W>(S, T, t_mid, lane, tid, A.p, A.p_int, team, dp, dm);
      } else {
        cut_slopes_walk<EPT, PMODE, kChains, W>(S, T, t_mid, lane, tid, A.p, A.p_int, team, dp, dm, anchors, it > 0, cost_scale);
      }
      if (dp * dm <= 0.f) break;                               // settled on a kink / flat piece (:186-187)
      if (!(dp * dm > 0.f)) break;                             // non-finite input: stop
      if (dp < 0.f) { t_lo = t_mid; lo_tight = true; dp_lo = dp; }
      else { t_hi = t_mid; hi_tight = true; dm_hi = dm; }
      {
        // by convexity an end of the bracket is within  width * |slope at that end|  of the minimum
        // COST.  Below one fp32 ulp of the cost (and below 1e-12 in any case) nothing is left to gain and the end is the
        // answer: with ~n*m micro-kinks the slope near the optimum is a noisy ~1e-6 and the search would spend its
        // last evaluations inside that noise; this ends it a few halvings before eps/L, and without the three cost
        // evaluations of the reference's finish, which resolve nothing at that scale.  Coinciding levels (equal
        // weights given explicitly: few, large kinks) keep large slopes on both sides and take the reference's exit.
        const float kGain = fmaxf(1e-12f, 1.2e-7f * cost_scale);
        if (lo_tight && hi_tight) {
          const float w = t_hi - t_lo;
          const float g_lo = -w * dp_lo, g_hi = w * dm_hi;
          if (fminf(g_lo, g_hi) < kGain) { t_mid = g_lo < g_hi ? t_lo : t_hi; break; }
        }
      }
      if ((t_hi - t_lo) < G.min_width) {                       // :189-200
        float unused;
        if (!lo_tight) cut_slopes<EPT, PMODE, W>(S, T, t_lo, lane, tid, A.p, A.p_int, team, dp_lo, unused);
        if (!hi_tight) cut_slopes<EPT, PMODE, W>(S, T, t_hi, lane, tid, A.p, A.p_int, team, unused, dm_hi);
        const float c_lo = cut_cost<EPT, PMODE, W>(S, T, t_lo, lane, tid, A.p, A.p_int, team);
        const float c_hi = cut_cost<EPT, PMODE, W>(S, T, t_hi, lane, tid, A.p, A.p_int, team);
        float t_c = (t_lo + t_hi) * 0.5f;
        if (fabsf(dp_lo - dm_hi) > 1e-3f) {                    // tangent intersection, :198-199 (written relative to
          // t_lo: the reference's form cancels terms of size theta * slope against each other)
          const float t_x = t_lo + (c_hi - c_lo - dm_hi * (t_hi - t_lo)) / (dp_lo - dm_hi);
          if (t_x == t_x) t_c = fminf(fmaxf(t_x, t_lo), t_hi);
        }
        // never end above a bracket end: an evaluation that lands within rounding of a kink can put that kink
        // ON an end, and the candidate then sits on the wrong side of it
        const float c_c = cut_cost<EPT, PMODE, W>(S, T, t_c, lane, tid, A.p, A.p_int, team);
        t_mid = t_c;
        float best = c_c;
        if (c_lo < best) { best = c_lo; t_mid = t_lo; }
        if (c_hi < best) { best = c_hi; t_mid = t_hi; }
        break;
      }
      {
        // Weighted clouds (round 2).  The cost has n*m kinks (every coincidence of a source level with a target
        // level), ~2.4e-7 apart at 2048 points: its one-sided slope is, at every scale above that, a smooth increasing
        // function -- exactly linear for p = 2 with the masses fixed.  Halving the bracket down to eps/L = 1e-7 as
        // the reference does takes ~17 evaluations after ~6 doublings; a secant on the slope gets there in 3-5:
        //   * no bracket yet: the line through the last two evaluations, over-stepped by a quarter (at least `step`);
        //   * bracket: regula falsi with the Illinois rule (an end that stays put twice has its slope halved, which
        //     throws the next point across the root) so that BOTH ends close in; the midpoint when the secant point
        //     is not strictly inside, and plain halving after kSecant steps.
        // The exit (width < eps/L, then the reference's tangent intersection) is unchanged.
        constexpr int kSecant = 24;
        const float f = dp < 0.f ? dp : dm;
        const int side = dp < 0.f ? -1 : 1;
        if (side < 0) { f_lo = f; if (last_side < 0 && hi_tight) f_hi *= 0.5f; }
        else { f_hi = f; if (last_side > 0 && lo_tight) f_lo *= 0.5f; }
        float t_next;
        if (lo_tight && hi_tight) {
          const float w = t_hi - t_lo;
          t_next = t_lo + w * (-f_lo) / (f_hi - f_lo);
          if (!(t_next > t_lo && t_next < t_hi) || ++secant_steps > kSecant) t_next = t_lo + 0.5f * w;
        } else {
          // p = 2: the cost is ~quadratic in the cut with curvature ~2 for clouds spread around the circle
          if (PMODE == 2 && !have_prev) step = fmaxf(step, SHW_GENERAL_FIRST_GAIN * fabsf(f));
          t_next = t_mid - (float)side * step;
          if (have_prev && (f - f_prev) * (t_mid - t_prev) > 0.f) {
            const float root = t_mid - f * (t_mid - t_prev) / (f - f_prev);
            const float over = t_mid + 1.25f * (root - t_mid);
            t_next = side < 0 ? fmaxf(t_next, over) : fminf(t_next, over);
          }
          t_next = fminf(fmaxf(t_next, t_lo), t_hi);
          step *= 2.f;
        }
        t_prev = t_mid; f_prev = f; have_prev = true; last_side = side;
        t_mid = t_next;
      }
    }
    if (G.cut_scratch && tid == 0) G.cut_scratch[(long)s * G.cut_stride] = t_mid;   // training: the gradient launch reads it
  }

  float cost;
  if constexpr (GRAD) {
    // Cost and its gradient at the cut: every atom's coefficient by its owner, once (walk_source_atoms)
    Rotated<EPT> R;
    R.set(T, t_mid, lane);
    const float part = walk_source_atoms<EPT, PMODE, W>(S, R, tid, A.p, A.p_int, gs);
    float sums[1] = {wave_sum_uniform(part, lane)};
    walk_target_atoms<EPT, PMODE, W>(S, R, tid, A.p, A.p_int, gt, shared + 2);
    team.sum(sums, lane);                                    // (W > 1: also the barrier that publishes gs, gt, tail)
    cost = sums[0];
    if constexpr (W == 1) __builtin_amdgcn_wave_barrier();
    // un-permute through LDS (the value rows are dead now -- every wave is past its walks) and store coalesced: a
    // direct scatter writes one 4-byte word per cache line -- 2.3 ms per launch at n=2048, m=1536
    const float tail = shared[2];
    float* by_index_s = s_val;
    float* by_index_t = t_val;
    if (W == 1 || wave == 0) {
#pragma unroll
      for (int r = 0; r < EPT; ++r) {
        const int e = lane * EPT + r;
        if (e < n) by_index_s[oidx[NI - 1][r]] = gs[r * kWave + lane];
      }
    }
    if (W == 1 || wave == 1) {
#pragma unroll
      for (int r = 0; r < EPT; ++r) {
        const int e = lane * EPT + r;
        // (the first rotated atom also owns the coefficient of its copy one turn later: own part first, then the tail)
        if (e < m) by_index_t[oidx[0][r]] = gt[r * kWave + lane] + (e == R.start ? tail : 0.f);
      }
    }
    if constexpr (W > 1) __syncthreads(); else __builtin_amdgcn_wave_barrier();
    float* cs = A.coef_s + (long)s * n;
    float* ct = A.coef_t + (long)s * m;
    for (int i = tid; i < max(n, m); i += kWave * W) {
      if (i < n) cs[i] = by_index_s[i];
      if (i < m) ct[i] = by_index_t[i];
    }
  } else {
    cost = cut_cost<EPT, PMODE, W>(S, T, t_mid, lane, tid, A.p, A.p_int, team);
  }
  if (tid == 0) {
    A.slice_cost[s] = cost;
    if (G.slice_theta) G.slice_theta[s] = t_mid;
  }
  }   // weighted clouds
}

template <int EPT>
static int launch_general_class(GeneralArgs& G, hipStream_t stream) {
  SswArgs& A = G.base;
  if (!problem_groups(A.pairs, A.slices, 1, A.num_groups)) return (int)hipErrorInvalidValue;
  const bool grad = A.coef_s != nullptr;
  const dim3 grid((unsigned)A.num_groups), block(64);
  if (A.p == 1.f && !A.bisect_p1) {
    if constexpr (EPT >= 8) {
      const size_t lds2 = ((size_t)(grad ? 6 : 4) * EPT * kWave + 2 * kWalkExt * kWave + kTeamFloats) * sizeof(float);
      if (lds2 > 160 * 1024) return (int)hipErrorInvalidValue;
      if (grad) hipLaunchKernelGGL((ssw_general_p1_walk2_kernel<EPT, true>), grid, dim3(128), lds2, stream, G);
      else hipLaunchKernelGGL((ssw_general_p1_walk2_kernel<EPT, false>), grid, dim3(128), lds2, stream, G);
    } else {
      const size_t lds1 = (size_t)8 * EPT * kWave * sizeof(float);
      if (grad) hipLaunchKernelGGL((ssw_general_p1_kernel<EPT, true>), grid, block, lds1, stream, G);
      else hipLaunchKernelGGL((ssw_general_p1_kernel<EPT, false>), grid, block, lds1, stream, G);
    }
    return (int)hipGetLastError();
  }
  const bool uniform = G.wu == nullptr && G.wv == nullptr;   // no weights: CDFs in closed form, no searches
  constexpr int W = general_waves(EPT);                      // waves per slice
  const dim3 wblock(64 * W);
  const auto launch = [&](auto pm, auto gr, GeneralArgs& args) {
    constexpr int PM = decltype(pm)::value;
    constexpr bool GR = decltype(gr)::value;
    const size_t lds = ((size_t)((uniform ? 2 : 4) + (GR ? 2 : 0)) * EPT * kWave + kTeamFloats +
                        (uniform ? 0 : general_ext_floats<EPT>())) * sizeof(float);
    if (uniform) hipLaunchKernelGGL((ssw_general_kernel<EPT, PM, GR, true, W>), grid, wblock, lds, stream, args);
    else hipLaunchKernelGGL((ssw_general_kernel<EPT, PM, GR, false, W>), grid, wblock, lds, stream, args);
  };
  if (!grad) {
    with_pmode(A.p_int, [&](auto pm) { launch(pm, std::false_type{}, G); });
    return (int)hipGetLastError();
  }
  GeneralArgs solve, eval;                                   // training: two launches
  training_launches(G, uniform, solve, eval);
  with_pmode(A.p_int, [&](auto pm) { launch(pm, std::false_type{}, solve); launch(pm, std::true_type{}, eval); });
  return (int)hipGetLastError();
}

int launch_general(SswArgs& A, const Plan& P, const float* wu, const float* wv, long wu_pair_stride, long wv_pair_stride,
                   float* slice_theta, hipStream_t stream) {
  GeneralArgs G{A, wu, wv, wu_pair_stride, wv_pair_stride, slice_theta, 0.f, 0.f, 0, 0, 0, nullptr, nullptr, 0, 0, 0};
  if (wu == nullptr && wv == nullptr) {                      // no weights: the integer grid of lcm(n, m)
    const long lcm = (long)A.n / gcd(A.n, A.m) * (long)A.m;
    G.lcm = (int)lcm;                                        // n, m <= 4096: < 2^24
    G.lcm_a = G.lcm / A.n;
    G.lcm_b = G.lcm / A.m;
  } else {
    G.first_step = 0.25f / (float)(A.n + A.m);
    G.min_width = 1e-7f;                                     // eps / L, :189
  }
  switch (P.kpl) {
#ifdef SHW_DEV_ONLY_EPT
    case SHW_DEV_ONLY_EPT: return launch_general_class<SHW_DEV_ONLY_EPT>(G, stream);
#else
    case 1: return launch_general_class<1>(G, stream);
    case 2: return launch_general_class<2>(G, stream);
    case 4: return launch_general_class<4>(G, stream);
    case 8: return launch_general_class<8>(G, stream);
    case 16: return launch_general_class<16>(G, stream);
    case 32: return launch_general_class<32>(G, stream);
    case 64: return launch_general_class<64>(G, stream);
#endif
    default: return (int)hipErrorInvalidValue;               // > 4096 points: not built for this path
  }
}

}  // namespace shw
