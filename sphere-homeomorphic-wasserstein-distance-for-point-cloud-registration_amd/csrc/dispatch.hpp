// dispatch.hpp -- host side of the float32 loss: which kernel family and size class serves a call.  Host only: no
// device code, and no HIP call outside the launch helpers at the end.
//
// A call is planned once (plan_*: pure functions of the sizes, the problem count and the knobs) and then launched by
// the unit that owns the planned family (launch_*: the unit's one entry, a switch from the size class to its template
// instantiation).  The C entry points of shw_capi.hip join the two.  tests/test_dispatch_cpu.py records, without a
// GPU, the kernel, grid, block and LDS request of every entry point over the sizes where a rule below changes.
//
// Environment knobs (diagnostics and A/B runs; read once per process, on the first call):
//   name                  values                   default  used by                 forced by
//   SHW_FORWARD_KERNEL    onewave | twowave |      (rule)   plan_forward            test_dispatch_cpu
//                         network | coop
//   SHW_GRAD_KERNEL       onewave                  (rule)   plan_forward_grad       test_r2_gpu (cooperative training
//                                                                                   kernel against the one-wave kernels)
//   SHW_SMALL_GRID        problem count, 0 = never 1024     plan_forward,           test_r3_gpu (small-grid kernels against
//                                                           plan_forward_grad       the throughput kernels)
//   SHW_KPL_CLASSES       0 = powers of two only   1        kpl_for, coop_kpl_for,  test_r3_gpu (keys-per-lane classes)
//                                                           level_median_coop_class
//   SHW_P1_SEARCH_KERNEL  1 = one-wave search      0        plan_level_median       test_r2_gpu (search kernel against the
//                         kernel at every size                                      merge and cooperative kernels)
//   SHW_P1_KERNEL         coop | merge             (rule)   plan_level_median       test_r2_gpu
//   SHW_BWD_WIDE          0 = never, 2 = whenever  1        plan_backward_points    test_r3_gpu (wide backward kernel)
//                         sizes and alignment allow
// (every setting is also recorded by test_dispatch_cpu.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <type_traits>

namespace shw {

struct SswArgs;   // ssw_common.hpp

struct Knobs {
  enum Forward { kRule, kNetwork, kCoop, kTwoWave, kOneWave };
  enum P1 { kP1Rule, kP1Coop, kP1Merge };
  Forward forward_kernel;
  bool grad_onewave;
  long small_grid;      // launches with at most this many (pair, slice) problems take the small-grid kernels
  bool kpl_classes;
  bool p1_search;
  P1 p1_kernel;
  int bwd_wide;
};

inline const Knobs& knobs() {
  static const Knobs k = [] {
    const auto first = [](const char* name) { const char* v = getenv(name); return v ? v[0] : '\0'; };
    Knobs r;
    const char f = first("SHW_FORWARD_KERNEL");
    r.forward_kernel = f == 'n' ? Knobs::kNetwork : f == 'c' ? Knobs::kCoop : f == 't' ? Knobs::kTwoWave
                     : f == 'o' ? Knobs::kOneWave : Knobs::kRule;
    r.grad_onewave = first("SHW_GRAD_KERNEL") == 'o';
    const char* small = getenv("SHW_SMALL_GRID");
    r.small_grid = small ? atol(small) : 1024L;
    r.kpl_classes = first("SHW_KPL_CLASSES") != '0';
    r.p1_search = first("SHW_P1_SEARCH_KERNEL") == '1';
    const char p1 = first("SHW_P1_KERNEL");
    r.p1_kernel = p1 == 'c' ? Knobs::kP1Coop : p1 == 'm' ? Knobs::kP1Merge : Knobs::kP1Rule;
    const char* wide = getenv("SHW_BWD_WIDE");
    r.bwd_wide = wide ? (wide[0] == '0' ? 0 : (wide[0] == '2' ? 2 : 1)) : 1;
    return r;
  }();
  return k;
}

// ---------------------------------------------------------------------------------------------
// size classes
// ---------------------------------------------------------------------------------------------
inline int small_integer_power(float p) {
  const int q = (int)p;
  return ((float)q == p && q >= 1 && q <= 8) ? q : 0;
}

inline int next_pow2(int v) {
  int r = 1;
  while (r < v) r <<= 1;
  return r;
}

inline int gcd(int a, int b) {
  while (b) { const int t = a % b; a = b; b = t; }
  return a;
}

// p == 1: levels are kept as exact integers  num = (#u)*(m/g) - (#v)*(n/g),  g = gcd(n, m),  level = num / lcm(n, m)
struct LevelGrid { int mg, ng; float inv_lcm; };
inline LevelGrid level_grid(int n, int m) {
  const int g = gcd(n, m);
  return {m / g, n / g, 1.f / ((float)n * (float)(m / g))};
}

// size class: registers per lane (EPT) for the padded point count
inline int ept_for(int n, int m) {
  const int padded = next_pow2(n > m ? n : m);
  return padded <= 64 ? 1 : padded / 64;
}

// keys per lane of the two-wave kernels of 513..2048 points (round 3): the power-of-two classes plus 12, 20, 24 and 28, so
// that a cloud pays for the next multiple of 256 points (768: of 256 x 3) and not for the next power of two -- the
// notebooks' 1200 points (Flow_cube.ipynb:200) take 1280 slots instead of 2048.  SHW_KPL_CLASSES=0 keeps powers of two.
inline int kpl_for(int n, int m, bool training, const Knobs& K) {
  const int big = n > m ? n : m;
  const int e = ept_for(n, m);
  if (!K.kpl_classes || e < 16) return e;
  for (int k = e / 2 + 4; k < e; k += 4) {           // 16: 12;  32: 20, 24, 28
    // (28 keys per lane: the loss kernel gains -- N = 1700: 0.299 -> 0.277 ms -- the training kernel does not: 0.632 -> 0.642)
    if (k * 64 >= big && !(training && k == 28)) return k;
  }
  return e;
}

// keys per lane of the cooperative kernels above 2048 points (W = 2 or 4 waves per slice): 20, 24 or 32.  Measured per
// pair at B N ~ 131 k, L = 512 (profiles/r03_size_sweep.txt): 28 keys per lane is never faster than 32 (the partially
// filled 32 class costs the same), nor is 24 at W = 4 in training; 20 and 24 pay (N = 3000: training 1.40 -> 0.83 ms,
// N = 5000: 1.88 -> 0.89).
inline int coop_kpl_for(int points, int W, bool training, const Knobs& K) {
  if (!K.kpl_classes) return 32;
  if (20 * 64 * W >= points) return 20;
  if (24 * 64 * W >= points && !(training && W == 4)) return 24;
  return 32;
}

// p == 1, cooperative kernel: W waves of 20 / 24 / 32 merged atoms per lane -- the smallest of the 12 classes (1280 ...
// 16384 slots) that holds n + m (round 3: 1200 + 1200 points pay for 2560 slots, not 4096; SHW_KPL_CLASSES=0 keeps 32
// per lane).  W = 0: none.
inline void level_median_coop_class(int total, const Knobs& K, int& W, int& ept) {
  W = 0; ept = 0;
  for (int w = 1; w <= 8 && W == 0; w *= 2) {
    for (int e : {20, 24, 32}) {
      if ((e == 32 || K.kpl_classes) && 64 * w * e >= total) { W = w; ept = e; break; }
    }
  }
}
// merged slots of the class that serves n + m atoms (0: none)
inline int level_median_coop_slots(int total, const Knobs& K) {
  int W, ept;
  level_median_coop_class(total, K, W, ept);
  return 64 * W * ept;
}
// training form available?  (12 bytes of LDS per merged slot up to n + m = 8192, 9 above: four keys per bin)
inline bool level_median_coop_trains(int n, int m) { return next_pow2(n + m) <= 16384; }

#ifndef SHW_COOP_EPT
#define SHW_COOP_EPT 32     // keys per lane (measured at 2048 points: 32 / W=1: 0.267 ms, 16 / W=2: 0.288, 8 / W=4: 0.292)
#endif

// ---------------------------------------------------------------------------------------------
// plans: ALL selection rules of the float32 loss
// ---------------------------------------------------------------------------------------------
enum class Family {
  invalid,
  forward,             // shw_ssw_fwd.hip        one wave per slice (kpl <= 32) or the bitonic multi-wave kernel (kpl 64, 128)
  forward2,            // shw_ssw_fwd2.hip       two waves per slice, one cloud each
  forward_coop,        // shw_ssw_coop.hip       W waves per slice, cooperative distribution sort
  forward_grad,        // shw_ssw_grad.hip       one wave per slice, kpl <= 64
  forward_grad2,       // shw_ssw_grad2.hip      two waves per slice
  forward_grad2_m32,   // shw_ssw_grad2_m32.hip  ... its partially filled 32-keys-per-lane class (built with SLP vectorisation)
  forward_grad_coop,   // shw_ssw_grad_coop.hip  W waves per slice
  forward_grad_kv,     // shw_ssw_grad_kv.hip    one wave per slice, 128 keys per lane as 64-bit items
  level_median,        // shw_ssw_p1.hip         p == 1, one-wave search kernel
  level_median_merge,  // shw_ssw_p1_merge.hip   p == 1, two waves per slice
  level_median_coop,   // shw_ssw_p1_coop.hip    p == 1, W waves per slice
  general,             // shw_ssw_general.hip    n != m and / or weights; its three solvers are headers: the integer grid
                       //                        (general_grid.hpp), the cut search (general_cut.hpp), the level median at
                       //                        p == 1 (general_p1.hpp)
  backward_points,     // shw_ssw_grad.hip       one point per lane, `waves` (4 or 16) waves split the slices
  backward_points4     // shw_ssw_grad.hip       four points per lane, 16-byte loads
};

struct Plan {
  Family family;
  int kpl;     // keys (atoms) per lane: the size class inside the family
  int waves;   // wavefronts per (pair, slice) where the rule chooses them (cooperative families, backward_points)
  bool full;   // p != 1: both clouds fill the class exactly (no padding atoms): the mask-free kernel forms, which index with
               // shifts and masks and so exist for the power-of-two classes only
};

// P with `full` set for a class that holds `capacity` points
inline Plan filled(Plan P, int n, int m, int capacity) {
  P.full = (P.kpl & (P.kpl - 1)) == 0 && n == capacity && m == capacity;
  return P;
}

// Which loss-only kernel serves p != 1 (measured, profiles/r02_ab_twowave_fwd.txt):
//   n == m == 2048 exactly    : one wave per slice (ssw_forward_kernel, in-wave distribution sort) -- 0.228 ms at config 3
//                               against 0.240 for two waves (round 4: 0.207, and no longer spilling)
//   512..2048 (padded) points : otherwise two waves per slice, one cloud each (shw_ssw_fwd2.hip): no spills, and faster
//                               wherever the cloud does not fill its size class (N=2000: 0.306 vs 0.330 ms)
//   > 2048                    : W = padded / 2048 waves per slice, cooperative distribution sort (shw_ssw_coop.hip), 20 / 24 /
//                               32 keys per lane (round 3: a cloud of 3000 points pays for 3072 slots, not 4096)
//   < 512                     : one wave per slice, register network below 8 keys per lane
//   small grids               : fewer (pair, slice) problems than SIMDs -- latency-bound: W = padded / 512 waves per slice of
//                               8 keys per lane (see plan_forward_grad)
// SHW_FORWARD_KERNEL: onewave = never two waves; twowave = two waves also at 2048 exactly; network = the bitonic
// multi-wave kernel above 2048 points; coop = the cooperative kernel from 2048 points on.
inline Plan plan_forward(int n, int m, long problems, const Knobs& K) {
#ifndef SHW_NO_COOP
  const int big = n > m ? n : m, padded = next_pow2(big);
  const bool mid = padded >= 512 && padded <= 2048;
  if (K.forward_kernel == Knobs::kRule && mid && problems <= K.small_grid) return filled({Family::forward_coop, 8, padded / 512}, n, m, padded);
  if ((K.forward_kernel == Knobs::kRule && padded > 2048) || (K.forward_kernel == Knobs::kCoop && padded >= 2048)) {
    const int W = padded / (64 * SHW_COOP_EPT);
    const int kpl = W >= 2 ? coop_kpl_for(big, W, false, K) : SHW_COOP_EPT;
    return filled({Family::forward_coop, kpl, W}, n, m, 64 * kpl * W);
  }
  const bool headline = n == 2048 && m == 2048;
  if (mid && (K.forward_kernel == Knobs::kTwoWave || (K.forward_kernel == Knobs::kRule && !headline))) {
    const int kpl = kpl_for(n, m, false, K);
    return filled({Family::forward2, kpl, 2}, n, m, 64 * kpl);
  }
#endif
  const int e = ept_for(n, m);
  return filled({Family::forward, e, e <= 32 ? 1 : e / 32}, n, m, 64 * e);           // 2049..4096 points: two waves per slice, ..8192: four
}

// Which training kernel serves p != 1:
//   <= 256 points   : one wave per slice (shw_ssw_grad.hip)
//   257..2048       : two waves per slice (shw_ssw_grad2.hip), 8 .. 32 keys per lane without the 28 class
//   2049..8192      : W = 2 / 4 waves per slice (shw_ssw_grad_coop.hip), 20 / 24 / 32 atoms per lane (round 3: 3000 points
//                     pay for 3072 slots, 5000 for 5120)
//   small grids     : (round 3) when a launch has fewer (pair, slice) problems than the chip has SIMDs -- the notebooks'
//                     gradient flow is ONE pair x 100 slices (Flow_cube.ipynb:1381) -- a slice is latency, not throughput:
//                     8 atoms per lane and W = padded / 512 waves per slice (4 at 1025..2048 points) cut the dependent
//                     chain of the sort and the solve and put 400 waves on the chip instead of 200.  (For full grids the
//                     same form is slower: wave scans, barriers and the seam sort are paid W times --
//                     profiles/r02_ab_coop_keys_per_lane.txt.)
// SHW_GRAD_KERNEL=onewave: the one-wave kernels at every size (128 keys per lane: shw_ssw_grad_kv.hip).
inline Plan plan_forward_grad(int n, int m, long problems, const Knobs& K) {
  const int e = ept_for(n, m);
  if (!K.grad_onewave && e >= 8 && e <= 32) {
    if (problems <= K.small_grid)
      return n == m ? filled({Family::forward_grad_coop, 8, next_pow2(n) / 512}, n, m, next_pow2(n)) : Plan{Family::invalid};
    const int kpl = kpl_for(n, m, true, K);
    const Plan P = filled({Family::forward_grad2, kpl, 2}, n, m, 64 * kpl);
    return kpl == 32 && !P.full ? Plan{Family::forward_grad2_m32, kpl, 2, false} : P;
  }
  if (!K.grad_onewave && (e == 64 || e == 128)) {
    const int W = next_pow2(n) / 2048, kpl = coop_kpl_for(n, W, true, K);
    return n == m ? filled({Family::forward_grad_coop, kpl, W}, n, m, 64 * kpl * W) : Plan{Family::invalid};
  }
  return filled({e == 128 ? Family::forward_grad_kv : Family::forward_grad, e, 1}, n, m, 64 * e);
}

// Which kernel serves p == 1 (grad: with coefficients).  The cooperative kernel (one distribution sort of the tagged
// concatenation, shw_ssw_p1_coop.hip): every shape above 2048 points; at or below, the loss from 1025 merged atoms on
// (measured at n = m = 2048 / 1024: 0.42 / 0.20 ms against the merge kernel's 0.54 / 0.25) -- training stays with the
// merge kernel there (0.97 / 0.42 against 0.94 / 0.45 ms)
// round 3: ... unless the cooperative kernel's class (20 / 24 / 32 merged atoms per lane) is smaller than the merge
// kernel's two power-of-two halves by more than the 12 % the merge kernel is faster per slot (n = m = 1200: 2560 against
// 4096 slots, 0.52 against 0.74 ms per step).  Otherwise up to 2048 points the merge kernel (two waves per slice, merge
// by the sorting network, shw_ssw_p1_merge.hip), and the one-wave search kernel (shw_ssw_p1.hip) for what is left.
// SHW_P1_SEARCH_KERNEL=1: the search kernel at every size; SHW_P1_KERNEL=coop | merge: that kernel wherever it can run.
inline Plan plan_level_median(int n, int m, bool grad, const Knobs& K) {
  const bool small = n <= 2048 && m <= 2048;
  bool coop = small ? (n + m > 1024 && (!grad || 9 * level_median_coop_slots(n + m, K) < 8 * 128 * ept_for(n, m)))
                    : (!grad || level_median_coop_trains(n, m));
  if (K.p1_kernel == Knobs::kP1Coop && n + m > 1024) coop = true;
  if (K.p1_kernel == Knobs::kP1Merge && small) coop = false;
  if (K.p1_search) coop = false;
  if (coop) {
    Plan P{Family::level_median_coop, 0, 0};
    level_median_coop_class(n + m, K, P.waves, P.kpl);
    return P;
  }
  if (small && !K.p1_search) return {Family::level_median_merge, ept_for(n, m), 2};
  return {Family::level_median, ept_for(n, m), 1};
}

// n != m and / or weights: one family, the power-of-two classes up to 4096 points (its waves per slice are a compile-time
// choice of the unit, general_waves)
inline Plan plan_general(int n, int m) { return {Family::general, ept_for(n, m), 0}; }

// d loss / d points.  Sizes that are multiples of 4 with 16-byte aligned rows and points: four points per lane, 16-byte
// loads -- for launches that also fill the chip with 256-point workgroups (two per CU): a small grid -- the notebooks' one
// pair of 1200 points -- is latency, and the one-point-per-lane kernel has four times the workgroups (9.3 against 15.2 us
// there).  One point per lane: 4 waves split the slices, or sixteen when there are fewer workgroups than CUs.
// SHW_BWD_WIDE=0: never four points per lane; =2: whenever sizes and alignment allow.
inline Plan plan_backward_points(int n, int m, int pairs, int slices, bool aligned16, const Knobs& K) {
  const long wide_groups = (long)((n + 255) / 256 + (m + 255) / 256) * pairs;
  if (K.bwd_wide != 0 && aligned16 && n % 4 == 0 && m % 4 == 0 && n >= 4 && m >= 4 && (wide_groups >= 512 || K.bwd_wide == 2))
    return {Family::backward_points4, 4, 4};
  const long groups = (long)((n + 63) / 64 + (m + 63) / 64) * pairs;
  return {Family::backward_points, 1, groups < 256 && slices >= 32 ? 16 : 4};
}

// ---------------------------------------------------------------------------------------------
// launch entries: one per family unit (SswArgs validated by the C entry points in shw_capi.hip); each is the switch
// from Plan::kpl / Plan::waves to the unit's template instantiations
// ---------------------------------------------------------------------------------------------
int launch_forward(SswArgs& A, const Plan& P, hipStream_t stream);
int launch_forward2(SswArgs& A, const Plan& P, hipStream_t stream);
int launch_forward_coop(SswArgs& A, const Plan& P, hipStream_t stream);
int launch_forward_grad(SswArgs& A, const Plan& P, hipStream_t stream);
int launch_forward_grad2(SswArgs& A, const Plan& P, hipStream_t stream);
int launch_forward_grad2_m32(SswArgs& A, const Plan& P, hipStream_t stream);
int launch_forward_grad_coop(SswArgs& A, const Plan& P, hipStream_t stream);
int launch_forward_grad_kv(SswArgs& A, const Plan& P, hipStream_t stream);
int launch_level_median(SswArgs& A, const Plan& P, hipStream_t stream);
int launch_level_median_merge(SswArgs& A, const Plan& P, hipStream_t stream);
int launch_level_median_coop(SswArgs& A, const Plan& P, hipStream_t stream);
// (fills GeneralArgs -- general_common.hpp -- and launches the solver the weights and p call for)
int launch_general(SswArgs& A, const Plan& P, const float* wu, const float* wv, long wu_pair_stride, long wv_pair_stride,
                   float* slice_theta, hipStream_t stream);
int launch_backward_points(const Plan& P, const float* xs, const float* xt, const float* dirs, const float* coef_s,
                           const float* coef_t, int pairs, int n, int m, int slices, long u_pair_stride, float scale,
                           const float* pair_w, const float* total_w, float* grad_xs, float* grad_xt, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// launch helpers
// ---------------------------------------------------------------------------------------------
// workgroups of a launch whose workgroup serves `per_group` (pair, slice) problems; false: more than a grid holds
inline bool problem_groups(int pairs, int slices, int per_group, int& groups) {
  const long g = ((long)pairs * slices + per_group - 1) / per_group;
  if (g > 0x7fffffffL) return false;
  groups = (int)g;
  return true;
}

// The (PMODE, FULL) ladder of a family, as two nestable steps: f receives PMODE (2: p == 2, 0: any p) resp. FULL (n == m ==
// the class's capacity: the mask-free forms; FULL_FORMS = false: a class without them) as an integral constant.  A unit
// nests them in the order in which it has always instantiated its kernels.
template <class F>
inline void with_pmode(int p_int, F f) {
  if (p_int == 2) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 0>{});
}
template <bool FULL_FORMS = true, class F>
inline void with_full(bool full, F f) {
  if constexpr (FULL_FORMS) {
    if (full) return f(std::true_type{});
  }
  f(std::false_type{});
}

// More than 64 KB of dynamic LDS has to be asked for.  The largest request so far is remembered per kernel instantiation
// and device, so a kernel whose request is a constant of the instantiation is raised once, on its first launch, and
// never inside a later stream capture; one whose request grows with the problem (ssw_f64_kernel) is raised again when it
// does.
template <auto Kernel>
inline hipError_t raise_dynamic_lds(size_t bytes) {
  static size_t raised[64] = {};
  if (bytes <= 64 * 1024) return hipSuccess;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (bytes > raised[dev & 63]) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)bytes);
    if (e != hipSuccess) return e;
    raised[dev & 63] = bytes;
  }
  return hipSuccess;
}

}  // namespace shw
