// general_common.hpp -- what the three solvers of general circular OT (n != m and / or weights) share: the kernel
// argument, the waves of a slice, a sorted cloud in LDS and the searches over it, and the sorts of a slice's clouds.
//   (a) no weights, n != m : the integer grid of lcm(n, m)      general_grid.hpp
//   (b) weights, p != 1    : the cut search on dCost            general_cut.hpp
//   (c) weights, p == 1    : the weighted level median          general_p1.hpp (its own two kernels)
// shw_ssw_general.hip includes the three, holds ssw_general_kernel (forms a and b) and launches all of them.
#pragma once
#include "bin_sort_idx.hpp"
#include "ssw_common.hpp"

namespace shw {

struct GeneralArgs {
  SswArgs base;
  const float* wu;        // (n) or (pairs, n) source weights, NULL = uniform 1/n
  const float* wv;        // (m) or (pairs, m) target weights, NULL = uniform 1/m
  long wu_pair_stride;    // 0 = shared by all pairs
  long wv_pair_stride;
  float* slice_theta;     // optional: the cut the solve ended on
  float first_step;       // weights: first step of the bracket search around the mean-difference guess
  float min_width;        // weights: bracket width below which the tangent intersection finishes the solve
  int lcm, lcm_a, lcm_b;  // no weights: lcm(n, m), lcm / n, lcm / m  (n, m <= 4096: lcm < 2^24) -- the integer grid
  // training runs as TWO launches: the solve at the loss-only kernel's occupancy (it leaves the cut of slice s in
  // cut_scratch[s * cut_stride] -- the first word of the slice's own coefficient row), then the gradient kernel
  // with cut_given = 1, which skips the solve and evaluates Cost and its gradient at that cut.
  float* cut_scratch;
  float* cut_scratch_t;   // index hand-off only: the target coefficient rows
  long cut_stride;
  int cut_given;
  // index hand-off (no weights, n, m >= 2): the solve launch also leaves the sort permutations of slice s in the
  // slice's coefficient rows (16-bit original indices by sorted position; the cut then goes to the LAST word of the
  // target row), and the gradient launch rebuilds the sorted coordinates from them -- a gather and a projection
  // instead of a second pair of sorts at the gradient kernel's low occupancy.
  int idx_handoff;
};

// The W waves of the workgroup that owns a slice.  sum(): wave-uniform partial sums -> sums over the slice, added in wave
// order (every wave gets the same bits, so control flow that depends on them stays uniform over the workgroup).  One
// barrier per call: the slots alternate between two parities, and a wave can only be one call ahead of another.
template <int W>
struct SliceTeam {
  float* red;               // [2 parities][W][4] floats
  int wave;
  int parity;
  // the slot of this call; the next call takes the other parity
  __device__ __forceinline__ float* next_slot() {
    float* slot = red + parity * (4 * W);
    parity ^= 1;
    return slot;
  }
  template <int K>
  __device__ __forceinline__ void sum(float (&v)[K], int lane) {
    static_assert(K <= 4, "four sums per call");
    if constexpr (W > 1) {
      float* slot = next_slot();
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) slot[wave * 4 + k] = v[k];
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < K; ++k) {
        float acc = 0.f;
#pragma unroll
        for (int q = 0; q < W; ++q) acc += slot[q * 4 + k];
        v[k] = as_f(__builtin_amdgcn_readfirstlane(as_i(acc)));
      }
    }
  }
  // two sums and two minima in one call
  __device__ __forceinline__ void sum2_min2(float (&sums)[2], float (&mins)[2], int lane) {
    if constexpr (W > 1) {
      float* slot = next_slot();
      if (lane == 0) { slot[wave * 4] = sums[0]; slot[wave * 4 + 1] = sums[1]; slot[wave * 4 + 2] = mins[0]; slot[wave * 4 + 3] = mins[1]; }
      __syncthreads();
      float a0 = 0.f, a1 = 0.f, m0 = __builtin_inff(), m1 = __builtin_inff();
#pragma unroll
      for (int q = 0; q < W; ++q) {
        a0 += slot[q * 4]; a1 += slot[q * 4 + 1];
        m0 = fminf(m0, slot[q * 4 + 2]); m1 = fminf(m1, slot[q * 4 + 3]);
      }
      sums[0] = as_f(__builtin_amdgcn_readfirstlane(as_i(a0)));
      sums[1] = as_f(__builtin_amdgcn_readfirstlane(as_i(a1)));
      mins[0] = as_f(__builtin_amdgcn_readfirstlane(as_i(m0)));
      mins[1] = as_f(__builtin_amdgcn_readfirstlane(as_i(m1)));
    }
  }
};
constexpr int kTeamFloats = 48;   // two parities of four waves' sums + the means and the tail coefficient

// waves per slice by size class: the evaluations split by atoms, the two sorts take one wave each
#ifndef SHW_GENERAL_W32
#define SHW_GENERAL_W32 2       // waves per slice at 1025..2048 points
#endif
#ifndef SHW_GENERAL_MINW_UNIFORM
#define SHW_GENERAL_MINW_UNIFORM 3   // waves per SIMD asked of the register allocator, kernels without weights
#endif
constexpr int general_waves(int ept) { return ept >= 64 ? 4 : (ept == 32 ? SHW_GENERAL_W32 : (ept >= 16 ? 2 : 1)); }
// one cloud as the solver sees it (weights given): ascending atom values and their inclusive CDF, lds_slot layout.
// (Clouds WITHOUT weights never get here: their CDFs are (i+1)/count and the solve runs on the integer grid of lcm(n, m),
//  shw_ssw_general_grid.hip.)
template <int EPT>
struct Side {
  const float* val;
  const float* cdf;
  int count;
  __device__ __forceinline__ float v(int i) const { return val[lds_slot<EPT>(i)]; }
  __device__ __forceinline__ float c(int i) const { return cdf[lds_slot<EPT>(i)]; }
  // number of atom VALUES < key (strict) or <= key (the p = 1 formula merges by value, not by CDF level)
  __device__ __forceinline__ int values_below(float key, bool strict) const {
    int lo = 0, hi = count;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const float x = v(mid);
      const bool go = strict ? (x < key) : (x <= key);
      lo = go ? mid + 1 : lo;
      hi = go ? hi : mid;
    }
    return lo;
  }
  // number of CDF entries < key (strict) or <= key  == torch.searchsorted(cdf, key, right = !strict)
  __device__ __forceinline__ int below(float key, bool strict) const {
    int lo = 0, hi = count;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const float x = c(mid);
      const bool go = strict ? (x < key) : (x <= key);
      lo = go ? mid + 1 : lo;
      hi = go ? hi : mid;
    }
    return lo;
  }
};

// ---------------------------------------------------------------------------------------------
// Batched, branch-free binary searches.  The searches of one atom are a chain of dependent LDS reads (12 probes
// at 2048 atoms); a lane owns up to 64 atoms and the first version ran their searches one after the other with
// data-dependent loops: ~1 500 dependent LDS round trips per lane per evaluation, 25 evaluations per slice,
// 51 ms per loss at config-3 sizes.  Here NB atoms are searched TOGETHER with a fixed trip count, so that each
// level issues NB (or 2 NB) independent reads.
// lower_bounds2: for every key, the number of entries < key (lt) and <= key (le) among the first `count`
// entries of an ascending array in lds_slot layout  (= torch.searchsorted(..., right=False / True)).
// ---------------------------------------------------------------------------------------------
template <int EPT, int NB>
__device__ __forceinline__ void lower_bounds2_arr(const float* arr, int count, const float (&key)[NB], int (&lt)[NB],
                                                  int (&le)[NB]) {
  constexpr int P = EPT * kWave;
  // one fixed-trip search for #{< key}; #{<= key} then differs only by the entries EQUAL to key, which two more
  // probes count in all but degenerate inputs (three or more equal entries: a second full search, rare branch)
#pragma unroll
  for (int b = 0; b < NB; ++b) lt[b] = 0;
#pragma unroll
  for (int st = P / 2; st >= 1; st >>= 1) {
    float x[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) x[b] = arr[lds_slot<EPT>(lt[b] + st - 1)];
#pragma unroll
    for (int b = 0; b < NB; ++b) lt[b] += ((lt[b] + st - 1 < count) && (x[b] < key[b])) ? st : 0;
  }
  bool again = false;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const float x = arr[lds_slot<EPT>(min(lt[b], P - 1))];
    lt[b] += ((lt[b] < count) && (x < key[b])) ? 1 : 0;
    const float e0 = arr[lds_slot<EPT>(min(lt[b], P - 1))];
    const float e1 = arr[lds_slot<EPT>(min(lt[b] + 1, P - 1))];
    const float e2 = arr[lds_slot<EPT>(min(lt[b] + 2, P - 1))];
    const bool q0 = (lt[b] < count) && (e0 == key[b]);
    const bool q1 = q0 && (lt[b] + 1 < count) && (e1 == key[b]);
    const bool q2 = q1 && (lt[b] + 2 < count) && (e2 == key[b]);
    le[b] = lt[b] + (q0 ? 1 : 0) + (q1 ? 1 : 0);
    again |= q2;
  }
  if (again) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      int pos = 0;
#pragma unroll
      for (int st = P / 2; st >= 1; st >>= 1) {
        const float y = arr[lds_slot<EPT>(pos + st - 1)];
        pos += ((pos + st - 1 < count) && (y <= key[b])) ? st : 0;
      }
      const float y = arr[lds_slot<EPT>(min(pos, P - 1))];
      le[b] = pos + (((pos < count) && (y <= key[b])) ? 1 : 0);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Walking searches (round 2, weighted clouds).  A lane's atoms are CONSECUTIVE sorted atoms, so their CDF levels
// ascend and so do their ranks in the other cloud's CDF: after one binary search for the lane's first atom the rank
// of every further atom is found by WALKING forward from its predecessor's -- four entries are read at once and the
// entries below the key counted; with weights of comparable size the walk advances ~1 entry per atom and one round
// of four reads settles it (the rare lane that needs more loops, wave-uniformly; a walk longer than kWalkRounds
// rounds falls back to the binary search).  The ranks are the binary search's, entry for entry: #{< key} is monotone
// in the key.  12 + 4 probes per atom become 4 + 3, and the chain of dependent reads per evaluation 32 instead
// of 4 x 15.  `prev` (the previous key) detects the one place where the keys of a lane do not ascend -- the rotated
// target's wrap from level ~1 to level ~0 -- and restarts the walk at entry 0.
// ---------------------------------------------------------------------------------------------
constexpr int kWalkRounds = 6;
// Window reads at constant offsets: an array in lds_slot layout ([r][lane], entry i at row i % EPT, column i / EPT)
// keeps entries i, i+1, ... of one column one row (256 bytes) apart -- until the column ends.  kWalkExt extra rows
// under the array repeat the first kWalkExt rows one column to the left (ext[r][c] = arr[r - EPT][c + 1], +inf past the
// last column), so that the kWalkExt entries from ANY index are base + q * 256 bytes: one address, kWalkExt reads.
constexpr int kWalkExt = 6;

// weighted clouds with >= 8 atoms per lane evaluate their slopes by walking (cut_slopes_walk)
template <int EPT>
constexpr bool general_walks() { return EPT >= 8; }
template <int EPT>
constexpr int general_ext_floats() { return general_walks<EPT>() ? kWalkExt * kWave : 0; }


template <int EPT>
__device__ __forceinline__ void fill_walk_ext(float* arr, int lane) {
#pragma unroll
  for (int q = 0; q < kWalkExt; ++q) {
    const float x = arr[q * kWave + min(lane + 1, kWave - 1)];
    arr[(EPT + q) * kWave + lane] = lane + 1 < kWave ? x : __builtin_inff();
  }
}

template <int EPT>
__device__ __forceinline__ int upper_bound_arr(const float* arr, int count, float key) {
  constexpr int P = EPT * kWave;
  int le = 0;
#pragma unroll
  for (int st = P / 2; st >= 1; st >>= 1) {
    const float x = arr[lds_slot<EPT>(le + st - 1)];
    le += ((le + st - 1 < count) && (x <= key)) ? st : 0;
  }
  const float x = arr[lds_slot<EPT>(min(le, P - 1))];
  return le + (((le < count) && (x <= key)) ? 1 : 0);
}

template <int EPT>
__device__ __forceinline__ int lower_bound_arr(const float* arr, int count, float key) {
  constexpr int P = EPT * kWave;
  int lt = 0;
#pragma unroll
  for (int st = P / 2; st >= 1; st >>= 1) {
    const float x = arr[lds_slot<EPT>(lt + st - 1)];
    lt += ((lt + st - 1 < count) && (x < key)) ? st : 0;
  }
  const float x = arr[lds_slot<EPT>(min(lt, P - 1))];
  return lt + (((lt < count) && (x < key)) ? 1 : 0);
}

// #{entries < key} for ONE key common to the wave: two rounds of 64 probes instead of 12 dependent ones
template <int EPT>
__device__ __forceinline__ int wave_lower_bound_arr(const float* arr, int count, float key, int lane) {
  static_assert(EPT <= kWave, "one probe per lane covers a block of EPT entries");
  const int i1 = lane * EPT + EPT - 1;                       // last entry of block `lane`
  const bool b1 = (i1 < count) && (arr[lds_slot<EPT>(i1)] < key);
  const int blk = __builtin_popcountll(__builtin_amdgcn_ballot_w64(b1));   // blocks entirely below the key
  const int i2 = min(blk, kWave - 1) * EPT + min(lane, EPT - 1);
  const bool b2 = (blk < kWave) && (lane < EPT) && (i2 < count) && (arr[lds_slot<EPT>(i2)] < key);
  return blk * EPT + __builtin_popcountll(__builtin_amdgcn_ballot_w64(b2));
}

// ranks #{< k} (ptr, updated) and #{<= k} (le) of C ascending key chains in `arr` (lds_slot layout with the
// fill_walk_ext rows, dead entries +inf), each from its chain's previous rank on: both are counted among the kWalkExt
// entries from ptr on and are settled unless all of those are <= k (then another round, wave-uniformly; binary
// searches after kWalkRounds rounds).
template <int EPT, int C>
__device__ __forceinline__ void walk_window(const float* arr, int count, const float (&k)[C], int (&ptr)[C],
                                            int (&le)[C]) {
  constexpr int P = EPT * kWave;
  int rounds = 0;
  for (;;) {
    bool more = false;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float* w = arr + lds_slot<EPT>(min(ptr[c], P - 1));
      int lta = 0, lea = 0;
#pragma unroll
      for (int q = 0; q < kWalkExt; ++q) {
        const float x = w[q * kWave];
        lta += (x < k[c]) ? 1 : 0;
        lea += (x <= k[c]) ? 1 : 0;
      }
      const bool inside = ptr[c] < P;                        // ptr == P (every entry below the key): nothing to read
      lta = inside ? lta : 0;
      lea = inside ? lea : 0;
      le[c] = ptr[c] + lea;
      ptr[c] += lta;
      more |= lea == kWalkExt;
    }
    if (__builtin_amdgcn_ballot_w64(more) == 0) break;
    if (++rounds >= kWalkRounds) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        ptr[c] = lower_bound_arr<EPT>(arr, count, k[c]);
        le[c] = upper_bound_arr<EPT>(arr, count, k[c]);
      }
      break;
    }
  }
}

// ranks of NA keys that ascend (except where key < prev: restart).  ptr: in, a rank not above key[0]'s unless the
// keys restart; out, the rank of the last key.  Dead keys (live[a] false) are not searched: they take the running rank.
template <int EPT, int NA>
__device__ __forceinline__ void walk_lower_bounds2(const float* arr, int count, const float (&key)[NA],
                                                   const bool (&live)[NA], float& prev, int& ptr, int (&lt)[NA],
                                                   int (&le)[NA]) {
  constexpr int P = EPT * kWave;
  bool again = false;
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const float k = live[a] ? key[a] : prev;
    ptr = k < prev ? 0 : ptr;
    prev = k;
    int rounds = 0;
    for (;;) {
      float x[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) x[q] = arr[lds_slot<EPT>(min(ptr + q, P - 1))];
      int adv = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) adv += ((ptr + q < count) && (x[q] < k)) ? 1 : 0;
      ptr += adv;
      if (__builtin_amdgcn_ballot_w64(adv == 4) == 0) break;
      if (++rounds >= kWalkRounds) { ptr = lower_bound_arr<EPT>(arr, count, k); break; }
    }
    lt[a] = ptr;
    const float e0 = arr[lds_slot<EPT>(min(ptr, P - 1))];
    const float e1 = arr[lds_slot<EPT>(min(ptr + 1, P - 1))];
    const float e2 = arr[lds_slot<EPT>(min(ptr + 2, P - 1))];
    const bool q0 = (ptr < count) && (e0 == k);
    const bool q1 = q0 && (ptr + 1 < count) && (e1 == k);
    const bool q2 = q1 && (ptr + 2 < count) && (e2 == k);
    le[a] = ptr + (q0 ? 1 : 0) + (q1 ? 1 : 0);
    again |= q2;
  }
  if (again) {                                               // three or more equal entries: degenerate weights
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const float k = live[a] ? key[a] : prev;
      int pos = 0;
#pragma unroll
      for (int st = P / 2; st >= 1; st >>= 1) {
        const float y = arr[lds_slot<EPT>(pos + st - 1)];
        pos += ((pos + st - 1 < count) && (y <= k)) ? st : 0;
      }
      const float y = arr[lds_slot<EPT>(min(pos, P - 1))];
      le[a] = live[a] ? pos + (((pos < count) && (y <= k)) ? 1 : 0) : le[a];
    }
  }
}

template <int PMODE>
__device__ __forceinline__ float powp(float d, float p, int p_int) { return pow_abs<PMODE>(d, p, p_int); }

// inclusive prefix sum over the wave's sorted positions lane*EPT + r  (the CDF, :169-170)
template <int EPT>
__device__ __forceinline__ void sorted_cdf(float (&w)[EPT], int lane) {
  float run = 0.f;
#pragma unroll
  for (int r = 0; r < EPT; ++r) { run += w[r]; w[r] = run; }
  float incl = run;                                          // inclusive scan of the lane totals
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float up = as_f(__builtin_amdgcn_ds_bpermute(max(lane - d, 0) << 2, as_i(incl)));
    incl += (lane >= d) ? up : 0.f;
  }
  const float offset = incl - run;
#pragma unroll
  for (int r = 0; r < EPT; ++r) w[r] += offset;
}

// project, sort (with indices), gather weights and build the CDF of ONE cloud of slice s (which = 0: target, 1: source);
// leaves the sorted values / CDF in LDS (dval, dcdf) and the sorted->original index map in registers.  `scratch` is a row
// for the coordinates by original index (it may be dval itself: the gather out of it is complete before the sorted values
// are written, LDS operations of a wave execute in order), `counters` 32 EPT words for the distribution sort.
template <int EPT, bool UNIFORM = false>
__device__ __forceinline__ void prepare_one(const GeneralArgs& G, int s, int lane, int which, float* dval, float* dcdf,
                                            float* scratch, unsigned* counters, int (&idx)[EPT], float& mean_out) {
  const SswArgs& A = G.base;
  const int b = s / A.slices, l = s - b * A.slices;
  const int n = A.n, m = A.m;
  float U[6];
  load_frame(A.dirs, (long)b * A.u_pair_stride + (long)l * 6, U);   // (3,2) row-major: U[2*d + k]
  const float* X = which == 0 ? A.xt + (long)b * m * A.pstride : A.xs + (long)b * n * A.pstride;
  const int count = which == 0 ? m : n;
  const float* Wt = which == 0 ? G.wv : G.wu;
  const long wstride = which == 0 ? G.wv_pair_stride : G.wu_pair_stride;
  int ln = lane;
  asm volatile("" : "+v"(ln));
  float val[EPT];
  // weighted, >= 8 atoms per lane: the distribution sort of bin_sort_idx.hpp (32 EPT counters beside the staging
  // row).  Without weights the one-wave kernel ran two waves per SIMD on 248 registers and the distribution sort's extra
  // live words spilled (measured in round 2: 2.1 -> 3.3 ms at n = 2048, m = 1536): it keeps the network.
  float part;
  if constexpr (EPT >= 8 && !UNIFORM) part = sorted_with_indices_binned<EPT, false, false>(X, count, ln, U, counters, scratch, val, idx);
  else part = sorted_with_indices<EPT>(X, count, ln, U, scratch, val, idx);
  float mean = 0.f;                                        // mass-weighted mean coordinate (first guess of the cut)
  if constexpr (UNIFORM) {
    mean = wave_sum_uniform(part, lane) / (float)count;                                 // CDF = (i+1)/count in closed form: no array
#pragma unroll
    for (int r = 0; r < EPT; ++r) dval[r * kWave + lane] = val[r];
  } else {
    float w[EPT];
#pragma unroll
    for (int r = 0; r < EPT; ++r) {
      const int e = lane * EPT + r;
      const bool live = e < count;
      w[r] = !live ? 0.f : (Wt ? Wt[(long)b * wstride + idx[r]] : 1.f / (float)count);
      mean += live ? w[r] * val[r] : 0.f;
    }
    mean = wave_sum_uniform(mean, lane);
    sorted_cdf<EPT>(w, lane);
#pragma unroll
    for (int r = 0; r < EPT; ++r) {                        // sorted position lane*EPT + r -> slot r*64 + lane
      dval[r * kWave + lane] = val[r];
      dcdf[r * kWave + lane] = (lane * EPT + r < count) ? w[r] : __builtin_inff();   // (window reads count on it)
    }
  }
  mean_out = mean;
  __builtin_amdgcn_wave_barrier();
}

// both clouds by ONE wave, the target first (the p = 1 kernels and the classes below 1024 points)
template <int EPT, bool UNIFORM = false>
__device__ __forceinline__ void prepare_sides(const GeneralArgs& G, int s, int lane, float* s_val, float* s_cdf,
                                              float* t_val, float* t_cdf, float* scratch, int (&sidx)[EPT],
                                              int (&tidx)[EPT], float& mean_s, float& mean_t,
                                              unsigned* counters = nullptr) {
  int idx[EPT];
#pragma nounroll
  for (int which = 0; which < 2; ++which) {                  // 0: target, 1: source
    float mean;
    prepare_one<EPT, UNIFORM>(G, s, lane, which, which == 0 ? t_val : s_val, which == 0 ? t_cdf : s_cdf, scratch, counters,
                              idx, mean);
    if (which == 0) {
      mean_t = mean;
#pragma unroll
      for (int r = 0; r < EPT; ++r) tidx[r] = idx[r];
    } else {
      mean_s = mean;
#pragma unroll
      for (int r = 0; r < EPT; ++r) sidx[r] = idx[r];
    }
  }
}

// gradient launch with index hand-off: sorted coordinates of one cloud (which = 0: target, 1: source) from the permutation
// the solve launch left in the coefficient rows (same projection arithmetic as load_coords, so the values are
// bit-identical to the ones that were sorted)
template <int EPT>
__device__ __forceinline__ void prepare_one_from_indices(const GeneralArgs& G, int s, int lane, int which, float* dval,
                                                         int (&idx)[EPT]) {
  const SswArgs& A = G.base;
  const int b = s / A.slices, l = s - b * A.slices;
  float U[6];
  load_frame(A.dirs, (long)b * A.u_pair_stride + (long)l * 6, U);   // (3,2) row-major: U[2*d + k]
  const int count = which == 0 ? A.m : A.n;
  const float* X = which == 0 ? A.xt + (long)b * count * A.pstride : A.xs + (long)b * count * A.pstride;
  const unsigned short* perm = reinterpret_cast<const unsigned short*>(
      which == 0 ? A.coef_t + (long)s * A.m : A.coef_s + (long)s * A.n);
#pragma unroll
  for (int r = 0; r < EPT; ++r) {
    const int e = lane * EPT + r;
    idx[r] = e < count ? (int)perm[min(e, count - 1)] : 0;
  }
#pragma unroll
  for (int r = 0; r < EPT; ++r) {
    const int e = lane * EPT + r;
    const float px = X[3 * idx[r]], py = X[3 * idx[r] + 1], pz = X[3 * idx[r] + 2];
    const float a = fmaf(pz, U[4], fmaf(py, U[2], fmaf(px, U[0], 0.f)));
    const float bb = fmaf(pz, U[5], fmaf(py, U[3], fmaf(px, U[1], 0.f)));
    dval[r * kWave + lane] = e < count ? circle_coord(a, bb) : __builtin_inff();
  }
  __builtin_amdgcn_wave_barrier();
}

constexpr int kMaxEvals = 96;   // evaluations of the slope a solve may spend (grid_solve, the cut search of ssw_general_kernel)

// Training with solvers (a) and (b) runs as two launches (GeneralArgs::cut_scratch): the solve with the loss-only kernel
// (fewer LDS rows, twice the waves per CU), then one gradient evaluation at the cut it left.
inline void training_launches(const GeneralArgs& G, bool uniform, GeneralArgs& solve, GeneralArgs& eval) {
  const SswArgs& A = G.base;
  solve = eval = G;
  solve.base.coef_s = solve.base.coef_t = nullptr;
  solve.cut_scratch = eval.cut_scratch = A.coef_s;           // first word of each slice's own coefficient row
  solve.cut_scratch_t = eval.cut_scratch_t = A.coef_t;
  solve.cut_stride = eval.cut_stride = A.n;
  eval.cut_given = 1;
  // (coordinate-row mode re-sorts in the gradient launch: the hand-off re-projects gathered POINTS)
  solve.idx_handoff = eval.idx_handoff = (uniform && A.n >= 2 && A.m >= 2 && A.pstride == 3) ? 1 : 0;
}

}  // namespace shw
