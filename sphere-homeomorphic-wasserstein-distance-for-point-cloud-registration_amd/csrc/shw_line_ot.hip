// shw_line_ot.hip -- exact 1-D optimal transport between two weighted empirical measures on the line: the quantile
// merge  W_p^p = int_0^1 |F_u^-1(t) - F_v^-1(t)|^p dt  for n != m and / or weights, with gradients w.r.t. the values.
// The line-level counterpart of the general circular path; the Euclidean sliced family (SWD, max-SW, ASWD, GSW, DSWD)
// sits on it wherever the two clouds differ in size or carry weights.
//
// One wavefront per row (rows form: the caller's keys) or per (pair, slice) (fused form: keys sum_d x_d theta_d in the
// order d = 0..D-1, the loader of shw_esw_dim.hip, so no (B,L,n) key matrix exists).  A kernel is instantiated per size
// class MAXE = max(EU, EV); inside it each side sorts with its own class (EU for n, EV for m, 1 .. 64 keys per lane)
// through one wave-uniform switch, so (4096, 1) sorts 4096 and 1 keys, not 4096 twice.
//
//   sort      : (orderable key, original index) items, wave_sort_kv (bare keys, wave_sort, when no index is needed);
//               sorted position e = lane * E + r.
//   stage     : sorted values, CDF ends and original indices of both sides in LDS, position e at [(e % E) * 64 + e / E]:
//               the owner lane reads its own atoms conflict-free (64 banks of 4 bytes, one lane per bank).
//               per wave 64 (EU + EV) dwords per array: 2 arrays for a value-only call with uniform weights (bare keys
//               are sorted, no index exists), 4 with gradients (the uniform grid is not staged), 6 and 64 doubles of
//               scan scratch for weighted ones: 4096 against 4096 points is 32 / 64 / 96.5 KB, one wave per workgroup;
//               2048 against 2048, two waves per workgroup, 32 / 64 / 97 KB.
//   CDF       : integers in both forms, so min, max and every overlap are exact.
//               weighted: weights gathered by original index (0 at the pads) and summed in double: P_e = base_lane +
//               local inclusive sum, base_{lane+1} = base_lane + lane total summed serially over the 64 lane totals --
//               the fixed order "lane-local prefix, then the wave scan" -- so P is monotone and a zero weight repeats
//               its predecessor's P bit for bit; the staged end is rint(P_e * 2^30 / T), the last one exactly 2^30.
//               (A float32 CDF resolves 6e-8 near 1: against an atom of mass 1/4096 that is 2.4e-4 of its gradient.
//               The grid resolves 9.3e-10; an atom lighter than that against the total is rounded away.)
//               uniform: the grid A_i = (i + 1) m/g, B_j = (j + 1) n/g, g = gcd(n, m), total nm/g <= 2^24, computed
//               from the index and never staged; ties i m = j n are exact.
//               The sums are scaled by one grid step (g / (n m), or 2^-30) once at the end.
//   pass U    : each lane owns its contiguous sorted u atoms; it finds the first v atom that overlaps (uniform: one
//               integer division; weighted: a 12-step binary search on B) and walks the overlaps
//               delta = min(A_i, B_j) - max(A_{i-1}, B_{j-1}), accumulating the cost and coef_u[idx_i].
//   pass V    : the same with the roles swapped, for coef_v only; skipped when no gradient is asked for.
// Owner-computed, no atomics: cost and gradients are the same bits on every run.
// Every loop is bounded by its index alone: the sorts are networks; the serial scan runs 64 steps; the binary search runs
// 12 steps; a walk's outer loop runs over the lane's <= E atoms and its inner loop advances j by one per trip and stops
// at j = count - 1, whatever the keys and weights are (the walk compares integers only).
// A negative or zero weight sum is not checked on the device: such a row yields, in bounded time, a value that means nothing.
//
// Gradients w.r.t. the weights (line_ot_pot_kernel, the weighted path only; include/shw.h has the definition).  The
// derivative of the cost w.r.t. a weight is the Kantorovich potential at that atom, and the jump of the potential across
// the CDF end that closes own atom r is c(r, j) - c(r + 1, j) with j the other side's atom active at that end.  The same
// walk finds j: after the inner loop of own atom r it stands on the first j with B_j >= A_r (pass U; on equal levels
// the u end comes first) or on the first i with A_i > B_j (pass V: the strict form of the same loop, so that both passes
// describe ONE merged order).  The next own value is read from LDS, whichever lane owns it.  The walk leaves, per atom,
// the sum of the jumps before it inside the lane (a fourth staged array per side: 64 (EU + EV) more dwords per wave, 129
// KB at 2048 against 2048 and 128.5 KB at 4096 against 4096, one workgroup per CU as before) and, per lane, the sum of
// its jumps, of its masses and of mass * prefix.  f_r = (jumps of this lane and the lanes after it) - prefix; the 64 lane
// totals are summed serially in double, from the last lane down, the same chain in every lane; a second serial sum gives
// sum_s abar_s f_s; a short pass over the lane's atoms writes (f_r - mean) / T at the original index.
// Costs are float32; their differences are summed in double.  An atom of weight 0 may lie far out (padding): its cost
// enters the sums with one jump and leaves with the next, the same float both times, so in double it cancels exactly and
// the atoms that carry mass do not see it.  For the same reason the parked float32 prefix is taken relative to the
// lane's first cost, which may be such an atom's.
#include "euclid_common.hpp"

namespace shw {


struct LineArgs {
  const float* a;          // rows: u (rows, n); fused: xs (pairs, n, dim)
  const float* b;          // rows: v (rows, m); fused: xt (pairs, m, dim)
  const float* thetas;     // fused only: (slices, dim) or (pairs, slices, dim); null = rows form
  const float* wa;         // optional weights of a: per row (rows form) or per pair (fused), stride 0 = shared
  const float* wb;
  long wa_stride, wb_stride;
  float* cost;             // (rows) or (pairs*slices)
  float* coef_a;           // optional, (rows*n): d cost / d key, original element order
  float* coef_b;           // optional, (rows*m)
  long rows;               // rows, or pairs*slices
  int n, m, dim, slices;
  long theta_pair_stride;  // 0 = shared
  float p;
  int p_int;
  int num_groups;
  int log_ea, log_eb;      // log2 of each side's keys per lane
  int wave_floats;         // LDS floats per wave (line_wave_floats)
  int mg, ng;              // uniform grid steps m/g and n/g
  float inv_total;         // one grid step: uniform g / (n m), weighted 2^-30
};

// one side as staged in LDS
struct LineSide {
  const float* val;        // sorted values
  const int* cdf;          // CDF ends on the 2^30 grid (weighted only)
  const int* idx;          // original indices
  int count;
  int log_e;
  int step;                // uniform grid: the end of atom i is (i + 1) * step
};

__device__ __forceinline__ int line_slot(int e, int log_e) { return ((e & ((1 << log_e) - 1)) << 6) + (e >> log_e); }

template <bool UNI>
__device__ __forceinline__ int line_end(const LineSide& S, int i) {
  if constexpr (UNI) return (i + 1) * S.step;
  else return S.cdf[line_slot(i, S.log_e)];
}

// (The register half below is sort_keys of euclid_common.hpp written out.  It stays written out on purpose: over
// load_row_keys + sort_keys the line kernels compile to another schedule, 0.5 .. 1.4 % slower -- profiles/r29_euclid_refactor.txt.)
// keys of one side (rows form or fused), sorted, into LDS.  IDX: with their original indices ((orderable key, index)
// items); a value-only call with uniform weights needs none and sorts bare keys, as the equal-size kernels do.
template <int E, bool IDX>
__device__ __forceinline__ void line_sort_side(const float* __restrict__ X, int count, int dim, const float* __restrict__ T,
                                               int lane, float* val, int* idx) {
  float key[E];
  if (T) {
    load_projections_dim<E>(X, count, dim, lane, T, key);
  } else {
#pragma unroll
    for (int r = 0; r < E; ++r) {
      const int i = r * kWave + lane;
      const float x = X[min(i, count - 1)];
      key[r] = i < count ? x : __builtin_inff();
    }
  }
  if constexpr (IDX) {
    item_t item[E];
#pragma unroll
    for (int r = 0; r < E; ++r) item[r] = make_item(orderable(key[r]), r * kWave + lane);
    wave_sort_kv<E>(item, lane);
#pragma unroll
    for (int r = 0; r < E; ++r) {
      val[r * kWave + lane] = from_orderable(item_key(item[r]));
      idx[r * kWave + lane] = item_idx(item[r]);
    }
  } else {
    wave_sort<E>(key, lane);
#pragma unroll
    for (int r = 0; r < E; ++r) val[r * kWave + lane] = key[r];
  }
}

template <int MAXE, bool IDX>
__device__ __forceinline__ void line_sort_class(int log_e, const float* __restrict__ X, int count, int dim,
                                                const float* __restrict__ T, int lane, float* val, int* idx) {
  switch (log_e) {                                            // wave-uniform
    case 0: line_sort_side<1, IDX>(X, count, dim, T, lane, val, idx); break;
    case 1: if constexpr (MAXE >= 2) line_sort_side<2, IDX>(X, count, dim, T, lane, val, idx); break;
    case 2: if constexpr (MAXE >= 4) line_sort_side<4, IDX>(X, count, dim, T, lane, val, idx); break;
    case 3: if constexpr (MAXE >= 8) line_sort_side<8, IDX>(X, count, dim, T, lane, val, idx); break;
    case 4: if constexpr (MAXE >= 16) line_sort_side<16, IDX>(X, count, dim, T, lane, val, idx); break;
    case 5: if constexpr (MAXE >= 32) line_sort_side<32, IDX>(X, count, dim, T, lane, val, idx); break;
    default: if constexpr (MAXE >= 64) line_sort_side<64, IDX>(X, count, dim, T, lane, val, idx); break;
  }
}

// CDF ends of one weighted side on the 2^30 grid (W null: every live atom weighs 1).  Rolled loops over the lane's
// 1 << log_e atoms; the sums run in double, so a prefix is exact to 2^-53 of the total before it is put on the grid.
constexpr int kLineGrid = 1 << 30;
__device__ __forceinline__ double line_cdf(const float* __restrict__ W, int count, int log_e, int lane, const int* idx,
                                           int* cdf) {
  const int E = 1 << log_e;
  const int e0 = lane << log_e;
  double tot = 0.0;
#pragma unroll 8
  for (int r = 0; r < E; ++r) {
    const int ix = idx[r * kWave + lane];
    float w = W ? W[min(ix, count - 1)] : 1.f;
    // (a NaN key orders after the +inf pads and puts a pad's index below count: such an atom weighs 0)
    w = (e0 + r < count && ix < count) ? w : 0.f;
    cdf[r * kWave + lane] = as_i(w);                          // parked in the atom's own slot
    tot += (double)w;
  }
  __builtin_amdgcn_wave_barrier();
  double* scratch = reinterpret_cast<double*>(cdf + (E << 6));   // the lane totals: 64 doubles behind the side's E rows
  scratch[lane] = tot;
  __builtin_amdgcn_wave_barrier();
  double base = 0.0, total = 0.0;
#pragma unroll 8
  for (int k = 0; k < kWave; ++k) {                           // serial, the same chain in every lane
    const double t = scratch[k];
    base = k == lane ? total : base;
    total += t;
  }
  __builtin_amdgcn_wave_barrier();
  const double to_grid = (double)kLineGrid / total;
  double local = 0.0;
#pragma unroll 8
  for (int r = 0; r < E; ++r) {
    local += (double)as_f(cdf[r * kWave + lane]);
    // (clamped before the conversion, NaN to 0: a zero, negative or non-finite total cannot leave the grid)
    const double end = __builtin_fmin(__builtin_fmax((base + local) * to_grid, 0.0), (double)kLineGrid);
    cdf[r * kWave + lane] = (e0 + r >= count - 1) ? kLineGrid : (int)__builtin_rint(end);
  }
  return total;                                               // the sum of the raw weights, the same in every lane
}

// One pass: the lane's own atoms of side O against the atoms of side X.  COST: accumulate the cost (pass U); the
// coefficient of own atom i is sign * sum_k delta_k d|D|^p/dD at D = u - v, written to coef[idx_i] when coef != null.
// CDF ends and overlaps are integers (the uniform grid of lcm(n, m) steps, or the 2^30 grid): min, max and the
// difference are exact, and an overlap is rounded once, when it becomes a float factor.
//
// TIE != 0: the walk also leaves what the potentials of the own side need (pre != null; LinePotSums).  The merged order
// puts the u end first on equal levels, so the atom of X active at the end of own atom i is the first with B_j >= A_i in
// pass U (TIE 1) and the first with A_i > B_j in pass V (TIE 2): the inner loop stops on it, and the lane's search starts
// where the lane before it stopped (TIE 1: first B_j >= lo).  The atoms this adds to a walk overlap nothing (delta <= 0),
// so cost and coefficients are the bits of TIE 0.
struct LinePotSums {
  double jumps = 0.0;      // sum of the jumps at the ends of the lane's atoms: in double, so that a cost that enters
                           // with one atom and leaves with the next (a far-out atom of weight 0) cancels exactly
  double anchor = 0.0;     // the lane's first cost: the prefixes are parked relative to it (float32), because up to there a
                           // prefix is that cost minus the atom's own plus costs between atoms that carry mass
  double mass = 0.0;       // sum of their normalised masses
  double mass_pre = 0.0;   // sum of mass * (jumps before the atom inside the lane)
};

template <int PMODE, bool UNI, bool COST, int TIE = 0>
__device__ __forceinline__ float line_walk(const LineSide& O, const LineSide& X, int lane, float p, int p_int, float scale,
                                           float* coef, float* pre = nullptr, LinePotSums* sums = nullptr) {
  float acc = 0.f;
  const int E = 1 << O.log_e;
  const int i0 = lane << O.log_e;
  if (i0 >= O.count) return acc;
  const int i1 = min(i0 + E, O.count);
  const int last = X.count - 1;
  int lo = i0 > 0 ? line_end<UNI>(O, i0 - 1) : 0;
  int j;
  if constexpr (UNI) {
    j = min(lo / X.step, last);                               // first j with (j + 1) step_x > i0 step_o
  } else {
    int a = 0, b = last;                                      // first j with B_j > lo, at most `last`
    for (int it = 0; it < 12; ++it) {                         // 2^12 = the largest count: the bracket closes in 12 halvings
      if (a < b) {
        const int mid = (a + b) >> 1;
        if (TIE == 1 ? line_end<UNI>(X, mid) >= lo : line_end<UNI>(X, mid) > lo) b = mid; else a = mid + 1;
      }
    }
    j = a;
  }
  int blo = j > 0 ? line_end<UNI>(X, j - 1) : 0;
  int bhi = line_end<UNI>(X, j);
  float xv = X.val[line_slot(j, X.log_e)];
  for (int i = i0; i < i1; ++i) {                             // <= E trips
    const int so = ((i - i0) << 6) + lane;                    // = line_slot(i, O.log_e)
    const int hi = line_end<UNI>(O, i);
    const float ov = O.val[so];
    float g = 0.f;
    // j only grows and stops at `last`: at most (i1 - i0) + X.count trips over the whole pass
    for (;;) {
      const int delta = min(hi, bhi) - max(lo, blo);
      if (delta > 0) {
        const float w = (float)delta;
        const float d = COST ? ov - xv : xv - ov;             // always u - v
        if constexpr (COST) acc = fmaf(w, pow_abs<PMODE>(d, p, p_int), acc);
        g = fmaf(w, dpow_abs<PMODE>(d, p, p_int), g);
      }
      if ((TIE == 2 ? bhi > hi : bhi >= hi) || j >= last) break;
      ++j;
      blo = bhi;
      bhi = line_end<UNI>(X, j);
      xv = X.val[line_slot(j, X.log_e)];
    }
    if (coef) {
      const int ix = O.idx[so];
      if (ix < O.count) coef[ix] = (COST ? g : -g) * scale;
    }
    if constexpr (TIE != 0) {
      if (pre) {
        const float mass = (float)(hi - lo) * scale;
        const float own = pow_abs<PMODE>(ov - xv, p, p_int);
        if (i == i0) sums->anchor = (double)own;
        pre[so] = (float)(sums->jumps - sums->anchor);
        sums->mass += (double)mass;
        sums->mass_pre = __builtin_fma((double)mass, sums->jumps, sums->mass_pre);
        if (i + 1 < O.count) {                                // the last end has no jump
          const float nv = O.val[line_slot(i + 1, O.log_e)];
          sums->jumps += (double)own - (double)pow_abs<PMODE>(nv - xv, p, p_int);
        }
      }
    }
    lo = hi;
  }
  return acc;
}

// The potentials of one side from what its walk left: d cost / d weight at the original index.  Every lane takes part
// (a lane without atoms brings zeros); `scratch` is 64 doubles.
__device__ __forceinline__ void line_pot_finish(const LineSide& O, int lane, const float* pre, const LinePotSums& sums,
                                                double total, double* scratch, float* __restrict__ pot) {
  scratch[lane] = sums.jumps;
  __builtin_amdgcn_wave_barrier();
  double suffix = 0.0, run = 0.0;
#pragma unroll 8
  for (int k = kWave - 1; k >= 0; --k) {                      // serial, the same chain in every lane
    run += scratch[k];
    suffix = k == lane ? run : suffix;
  }
  __builtin_amdgcn_wave_barrier();
  scratch[lane] = suffix * sums.mass - sums.mass_pre;         // sum of abar_s f_s over the lane's atoms
  __builtin_amdgcn_wave_barrier();
  double mean = 0.0;
#pragma unroll 8
  for (int k = 0; k < kWave; ++k) mean += scratch[k];
  __builtin_amdgcn_wave_barrier();
  const double inv = 1.0 / total;
  const double above = suffix - sums.anchor;                   // the parked prefixes are relative to the anchor
  const int E = 1 << O.log_e;
  const int i0 = lane << O.log_e;
#pragma unroll 8
  for (int r = 0; r < E; ++r) {
    if (i0 + r < O.count) {
      const int so = (r << 6) + lane;
      const int ix = O.idx[so];
      if (ix < O.count) pot[ix] = (float)((above - (double)pre[so] - mean) * inv);
    }
  }
}

template <int PMODE, bool UNI>
__device__ __forceinline__ float line_passes(const LineSide& U, const LineSide& V, int lane, float p, int p_int, float scale,
                                             float* cu, float* cv) {
  const float acc = line_walk<PMODE, UNI, true>(U, V, lane, p, p_int, scale, cu);
  if (cv) (void)line_walk<PMODE, UNI, false>(V, U, lane, p, p_int, scale, cv);
  return acc;
}

// LDS floats per wave: values of both sides, 64 << log_e each; their indices unless the call is value-only with uniform
// weights; weighted: the CDF ends as well, and 64 doubles for the lane totals of the serial scan
inline int line_wave_floats(int log_ea, int log_eb, bool uniform, bool grad) {
  const int atoms = (kWave << log_ea) + (kWave << log_eb);
  return uniform ? (grad ? 2 : 1) * atoms : 3 * atoms + 2 * kWave;
}
// with potentials (weighted only): a fourth array per side behind the 64 doubles, the jumps before each atom inside its lane
inline int line_pot_wave_floats(int log_ea, int log_eb) {
  return line_wave_floats(log_ea, log_eb, false, true) + (kWave << log_ea) + (kWave << log_eb);
}

// the weighted passes with the potentials of the sides that have a row: pass V runs for them even without coefficients
template <int PMODE>
__device__ __forceinline__ float line_passes_pot(const LineSide& U, const LineSide& V, int lane, float p, int p_int,
                                                 float scale, float* cu, float* cv, float* pre_u, float* pre_v,
                                                 LinePotSums& su, LinePotSums& sv) {
  const float acc = line_walk<PMODE, false, true, 1>(U, V, lane, p, p_int, scale, cu, pre_u, &su);
  if (cv || pre_v) (void)line_walk<PMODE, false, false, 2>(V, U, lane, p, p_int, scale, cv, pre_v, &sv);
  return acc;
}

template <int MAXE, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void line_ot_kernel(LineArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ra = kWave << A.log_ea, rb = kWave << A.log_eb;
  float* base = lds + wave * A.wave_floats;
  // order: a.val, b.val, a.idx, b.idx, then (weighted only) a.cdf, b.cdf, 64 doubles.  The scan's lane totals sit behind
  // the side's CDF rows: for side a in b.cdf and what follows it, written later; for side b in the last 64 doubles.
  float* aval = base;
  float* bval = aval + ra;
  int* aidx = reinterpret_cast<int*>(bval + rb);
  int* bidx = aidx + ra;
  int* acdf = bidx + rb;
  int* bcdf = acdf + ra;

  const int vid = xcd_contiguous_id(blockIdx.x, A.num_groups);
  const long s = (long)vid * WAVES + wave;
  if (s >= A.rows) return;
  const int n = A.n, m = A.m;
  const float* T = nullptr;
  const float* Xa;
  const float* Xb;
  long wrow = s;                                               // which weight row: the row, or the pair
  if (A.thetas) {
    const int si = (int)s, b = si / A.slices, l = si - b * A.slices;   // pairs*slices fits an int (checked by the entry)
    T = A.thetas + (long)b * A.theta_pair_stride + (long)l * A.dim;
    Xa = A.a + (long)b * n * A.dim;
    Xb = A.b + (long)b * m * A.dim;
    wrow = b;
  } else {
    Xa = A.a + s * n;
    Xb = A.b + s * m;
  }
  const bool uniform = A.wa == nullptr && A.wb == nullptr;

  const bool indexed = !uniform || A.coef_a != nullptr;         // weights are gathered, coefficients scattered, by index
#pragma nounroll
  for (int which = 0; which < 2; ++which) {                    // one copy of the sorts serves both sides
    const bool sb = which == 0;
    if (indexed)
      line_sort_class<MAXE, true>(sb ? A.log_eb : A.log_ea, sb ? Xb : Xa, sb ? m : n, A.dim, T, lane, sb ? bval : aval,
                                  sb ? bidx : aidx);
    else
      line_sort_class<MAXE, false>(sb ? A.log_eb : A.log_ea, sb ? Xb : Xa, sb ? m : n, A.dim, T, lane, sb ? bval : aval,
                                   nullptr);
  }
  __builtin_amdgcn_wave_barrier();
  if (!uniform) {
    // side a first: its scratch may lie in b.cdf
    line_cdf(A.wa ? A.wa + wrow * A.wa_stride : nullptr, n, A.log_ea, lane, aidx, acdf);
    __builtin_amdgcn_wave_barrier();
    line_cdf(A.wb ? A.wb + wrow * A.wb_stride : nullptr, m, A.log_eb, lane, bidx, bcdf);
    __builtin_amdgcn_wave_barrier();
  }

  const LineSide U{aval, acdf, aidx, n, A.log_ea, A.mg};
  const LineSide V{bval, bcdf, bidx, m, A.log_eb, A.ng};
  float* cu = A.coef_a ? A.coef_a + s * n : nullptr;
  float* cv = A.coef_b ? A.coef_b + s * m : nullptr;
  float acc;
  if (uniform) {
    if (A.p_int == 2) acc = line_passes<2, true>(U, V, lane, A.p, A.p_int, A.inv_total, cu, cv);
    else acc = line_passes<0, true>(U, V, lane, A.p, A.p_int, A.inv_total, cu, cv);
  } else {
    if (A.p_int == 2) acc = line_passes<2, false>(U, V, lane, A.p, A.p_int, A.inv_total, cu, cv);
    else acc = line_passes<0, false>(U, V, lane, A.p, A.p_int, A.inv_total, cu, cv);
  }
  acc = wave_sum(acc, lane);
  if (lane == 0) A.cost[s] = acc * A.inv_total;
}

// The call with potentials: the weighted path of line_ot_kernel (always indexed, never the uniform grid) with the fourth
// staged array, the potential forms of the walks and the finishing pass.  It is a kernel of its own with an argument block
// of its own, and line_ot_kernel above is left as written: folded into one body with a template flag, the compiler
// schedules the call without potentials differently (tools/kernel_digest.py), and that call must run the code it ran.
struct LinePotArgs {
  LineArgs line;
  float* pot_a;            // optional, (rows*n): d cost / d weight of a, original element order; needs wa
  float* pot_b;            // optional, (rows*m); needs wb
};

template <int MAXE, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void line_ot_pot_kernel(LinePotArgs P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const LineArgs& A = P.line;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ra = kWave << A.log_ea, rb = kWave << A.log_eb;
  float* base = lds + wave * A.wave_floats;
  // order: a.val, b.val, a.idx, b.idx, a.cdf, b.cdf, 64 doubles (line_ot_kernel's), then a.pre, b.pre
  float* aval = base;
  float* bval = aval + ra;
  int* aidx = reinterpret_cast<int*>(bval + rb);
  int* bidx = aidx + ra;
  int* acdf = bidx + rb;
  int* bcdf = acdf + ra;
  double* scratch = reinterpret_cast<double*>(bcdf + rb);      // free for the potentials once the CDFs stand
  float* apre = reinterpret_cast<float*>(scratch + kWave);
  float* bpre = apre + ra;

  const int vid = xcd_contiguous_id(blockIdx.x, A.num_groups);
  const long s = (long)vid * WAVES + wave;
  if (s >= A.rows) return;
  const int n = A.n, m = A.m;
  const float* T = nullptr;
  const float* Xa;
  const float* Xb;
  long wrow = s;
  if (A.thetas) {
    const int si = (int)s, b = si / A.slices, l = si - b * A.slices;
    T = A.thetas + (long)b * A.theta_pair_stride + (long)l * A.dim;
    Xa = A.a + (long)b * n * A.dim;
    Xb = A.b + (long)b * m * A.dim;
    wrow = b;
  } else {
    Xa = A.a + s * n;
    Xb = A.b + s * m;
  }
#pragma nounroll
  for (int which = 0; which < 2; ++which) {
    const bool sb = which == 0;
    line_sort_class<MAXE, true>(sb ? A.log_eb : A.log_ea, sb ? Xb : Xa, sb ? m : n, A.dim, T, lane, sb ? bval : aval,
                                sb ? bidx : aidx);
  }
  __builtin_amdgcn_wave_barrier();
  const double total_a = line_cdf(A.wa ? A.wa + wrow * A.wa_stride : nullptr, n, A.log_ea, lane, aidx, acdf);
  __builtin_amdgcn_wave_barrier();
  const double total_b = line_cdf(A.wb ? A.wb + wrow * A.wb_stride : nullptr, m, A.log_eb, lane, bidx, bcdf);
  __builtin_amdgcn_wave_barrier();

  const LineSide U{aval, acdf, aidx, n, A.log_ea, A.mg};
  const LineSide V{bval, bcdf, bidx, m, A.log_eb, A.ng};
  float* cu = A.coef_a ? A.coef_a + s * n : nullptr;
  float* cv = A.coef_b ? A.coef_b + s * m : nullptr;
  float* pre_u = P.pot_a ? apre : nullptr;
  float* pre_v = P.pot_b ? bpre : nullptr;
  LinePotSums su, sv;
  float acc;
  if (A.p_int == 2) acc = line_passes_pot<2>(U, V, lane, A.p, A.p_int, A.inv_total, cu, cv, pre_u, pre_v, su, sv);
  else acc = line_passes_pot<0>(U, V, lane, A.p, A.p_int, A.inv_total, cu, cv, pre_u, pre_v, su, sv);
  __builtin_amdgcn_wave_barrier();
  if (P.pot_a) line_pot_finish(U, lane, apre, su, total_a, scratch, P.pot_a + s * n);
  if (P.pot_b) line_pot_finish(V, lane, bpre, sv, total_b, scratch, P.pot_b + s * m);
  acc = wave_sum(acc, lane);
  if (lane == 0) A.cost[s] = acc * A.inv_total;
}

// grad[g, i] = sum over the rows r of group g (rows_per_group consecutive rows, ascending) of w[r] * pot[r, i]; w null = 1.
// One lane per element, coalesced along i; no atomics: the same bits on every run.
__global__ __launch_bounds__(256) void line_weight_reduce_kernel(const float* __restrict__ pot, const float* __restrict__ w,
                                                                 long rows, int rows_per_group, int count,
                                                                 float* __restrict__ grad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int ic = min(i, count - 1);
  const long r0 = (long)blockIdx.y * rows_per_group;
  const long r1 = r0 + rows_per_group < rows ? r0 + rows_per_group : rows;
  float g = 0.f;
  for (long r = r0; r < r1; ++r) g = fmaf(w ? w[r] : 1.f, pot[r * count + ic], g);
  if (i < count) grad[(long)blockIdx.y * count + i] = g;
}

// grad[b,i,d0+k] = sum_l w[b,l] * coef[b,l,i] * theta[b,l,d0+k], k < DC: one point per lane, DC coordinates per
// workgroup (blockIdx.z picks the chunk, so D > 16 splits over the grid instead of spilling); the first chunks_s
// workgroups of a pair serve the n source points, the rest the m target points.  Coordinates past D re-read the last
// one and are not stored.
template <int DC>
__global__ __launch_bounds__(256) void line_esw_backward_points_kernel(const float* __restrict__ thetas,
                                                                       const float* __restrict__ coef_s,
                                                                       const float* __restrict__ coef_t,
                                                                       const float* __restrict__ slice_w, int n, int m,
                                                                       int dim, int slices, long theta_pair_stride,
                                                                       float* __restrict__ grad_xs,
                                                                       float* __restrict__ grad_xt, int chunks_s) {
  const int b = blockIdx.y;
  const int d0 = blockIdx.z * DC;
  const bool is_t = (int)blockIdx.x >= chunks_s;
  const int chunk = is_t ? blockIdx.x - chunks_s : blockIdx.x;
  const int count = is_t ? m : n;
  const int i = chunk * 256 + threadIdx.x;
  const int ic = min(i, count - 1);
  const int last = dim - d0 - 1;
  const float* C = (is_t ? coef_t : coef_s) + (long)b * slices * count;
  float* G = (is_t ? grad_xt : grad_xs) + (long)b * count * dim + d0;
  const float* Tb = thetas + (long)b * theta_pair_stride + d0;
  const float* W = slice_w + (long)b * slices;
  float g[DC];
#pragma unroll
  for (int k = 0; k < DC; ++k) g[k] = 0.f;
  for (int l = 0; l < slices; ++l) {
    const float c = C[(long)l * count + ic] * W[l];
    const float* Tl = Tb + (long)l * dim;
#pragma unroll
    for (int k = 0; k < DC; ++k) g[k] = fmaf(c, Tl[min(k, last)], g[k]);
  }
  if (i < count) {
#pragma unroll
    for (int k = 0; k < DC; ++k)
      if (k <= last) G[(long)i * dim + k] = g[k];
  }
}

// grad_theta[b,l,d0+k] = w[b,l] * ( sum_{i<n} coef_s[b,l,i] xs[b,i,d0+k] + sum_{j<m} coef_t[b,l,j] xt[b,j,d0+k] ): one
// workgroup per (slice, pair, coordinate chunk); each lane a strided run of the source points, then of the target
// points, then wave sums and (w0 + w1) + (w2 + w3).  No atomics: the same bits on every run.
template <int DC>
__global__ __launch_bounds__(256) void line_esw_backward_dirs_kernel(const float* __restrict__ xs,
                                                                     const float* __restrict__ xt,
                                                                     const float* __restrict__ coef_s,
                                                                     const float* __restrict__ coef_t,
                                                                     const float* __restrict__ slice_w, int n, int m,
                                                                     int dim, int slices, float* __restrict__ grad_thetas) {
  __shared__ float red[DC][4];
  const int l = blockIdx.x, b = blockIdx.y;
  const int d0 = blockIdx.z * DC;
  const int last = dim - d0 - 1;
  const float* Xs = xs + (long)b * n * dim + d0;
  const float* Xt = xt + (long)b * m * dim + d0;
  const float* Cs = coef_s + ((long)b * slices + l) * n;
  const float* Ct = coef_t + ((long)b * slices + l) * m;
  float g[DC];
#pragma unroll
  for (int k = 0; k < DC; ++k) g[k] = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float c = Cs[i];
    const long row = (long)i * dim;
#pragma unroll
    for (int k = 0; k < DC; ++k) g[k] = fmaf(c, Xs[row + min(k, last)], g[k]);
  }
  for (int i = threadIdx.x; i < m; i += 256) {
    const float c = Ct[i];
    const long row = (long)i * dim;
#pragma unroll
    for (int k = 0; k < DC; ++k) g[k] = fmaf(c, Xt[row + min(k, last)], g[k]);
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

template <int MAXE, int WAVES>
static int launch_line(LineArgs& A, hipStream_t stream) {
  const long groups = (A.rows + WAVES - 1) / WAVES;
  if (groups > 0x7fffffffL) return (int)hipErrorInvalidValue;
  A.num_groups = (int)groups;
  A.wave_floats = line_wave_floats(A.log_ea, A.log_eb, A.wa == nullptr && A.wb == nullptr, A.coef_a != nullptr);
  const size_t lds = (size_t)WAVES * A.wave_floats * sizeof(float);
  const hipError_t e = raise_dynamic_lds<line_ot_kernel<MAXE, WAVES>>(lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((line_ot_kernel<MAXE, WAVES>), dim3((unsigned)groups), dim3(WAVES * 64), lds, stream, A);
  return (int)hipGetLastError();
}

template <int MAXE, int WAVES>
static int launch_line_pot(LinePotArgs& P, hipStream_t stream) {
  LineArgs& A = P.line;
  const long groups = (A.rows + WAVES - 1) / WAVES;
  if (groups > 0x7fffffffL) return (int)hipErrorInvalidValue;
  A.num_groups = (int)groups;
  A.wave_floats = line_pot_wave_floats(A.log_ea, A.log_eb);
  const size_t lds = (size_t)WAVES * A.wave_floats * sizeof(float);
  const hipError_t e = raise_dynamic_lds<line_ot_pot_kernel<MAXE, WAVES>>(lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((line_ot_pot_kernel<MAXE, WAVES>), dim3((unsigned)groups), dim3(WAVES * 64), lds, stream, P);
  return (int)hipGetLastError();
}

inline int log2_of(int pow2) {
  int r = 0;
  while ((1 << r) < pow2) ++r;
  return r;
}

// pot_a / pot_b: both null = the call without potentials
static int launch_line_class(LineArgs& A, hipStream_t stream, float* pot_a = nullptr, float* pot_b = nullptr) {
  const int ea = ept_for(A.n, A.n), eb = ept_for(A.m, A.m);
  A.log_ea = log2_of(ea);
  A.log_eb = log2_of(eb);
  const int g = gcd(A.n, A.m);
  A.mg = A.m / g;
  A.ng = A.n / g;
  const bool uniform = A.wa == nullptr && A.wb == nullptr;
  A.inv_total = uniform ? 1.f / ((float)A.n * (float)A.mg) : 1.f / (float)kLineGrid;
  A.p_int = small_integer_power(A.p);
  if (pot_a || pot_b) {
    LinePotArgs P{A, pot_a, pot_b};
    return with_ept_waves(ea > eb ? ea : eb, [&](auto maxe, auto waves) {
      return launch_line_pot<decltype(maxe)::value, decltype(waves)::value>(P, stream);
    });
  }
  return with_ept_waves(ea > eb ? ea : eb, [&](auto maxe, auto waves) {
    return launch_line<decltype(maxe)::value, decltype(waves)::value>(A, stream);
  });
}

inline bool line_counts_ok(int n, int m) { return n >= 1 && n <= kMaxEuclidPoints && m >= 1 && m <= kMaxEuclidPoints; }

inline bool line_weights_ok(const float* w, long stride, int count) { return stride == 0 || (w && stride >= count); }

int launch_line_esw_backward_points(const float* thetas, const float* coef_s, const float* coef_t, const float* slice_w,
                                    int pairs, int n, int m, int dim, int slices, long theta_pair_stride, float* grad_xs,
                                    float* grad_xt, hipStream_t stream) {
  const int chunks_s = (n + 255) / 256, chunks_t = (m + 255) / 256;
  with_coord_chunk(dim, [&](auto dc, unsigned z) {
    hipLaunchKernelGGL(line_esw_backward_points_kernel<decltype(dc)::value>, dim3(chunks_s + chunks_t, pairs, z), dim3(256), 0,
                       stream, thetas, coef_s, coef_t, slice_w, n, m, dim, slices, theta_pair_stride, grad_xs, grad_xt,
                       chunks_s);
  });
  return (int)hipGetLastError();
}

// the two forward entries, with or without potential rows
static int line_rows_forward(const float* u, const float* v, long rows, int n, int m, float p, const float* u_weights,
                             const float* v_weights, long u_weight_stride, long v_weight_stride, float* row_cost,
                             float* coef_u, float* coef_v, float* pot_u, float* pot_v, void* stream) {
  if (!u || !v || !row_cost) return (int)hipErrorInvalidValue;
  if ((coef_u == nullptr) != (coef_v == nullptr)) return (int)hipErrorInvalidValue;
  if ((pot_u && !u_weights) || (pot_v && !v_weights)) return (int)hipErrorInvalidValue;
  if (rows < 0 || !line_counts_ok(n, m) || !(p >= 1.f)) return (int)hipErrorInvalidValue;
  if (!line_weights_ok(u_weights, u_weight_stride, n) || !line_weights_ok(v_weights, v_weight_stride, m))
    return (int)hipErrorInvalidValue;
  if (rows == 0) return 0;
  LineArgs A{};
  A.a = u; A.b = v; A.wa = u_weights; A.wb = v_weights; A.wa_stride = u_weight_stride; A.wb_stride = v_weight_stride;
  A.cost = row_cost; A.coef_a = coef_u; A.coef_b = coef_v;
  A.rows = rows; A.n = n; A.m = m; A.dim = 1; A.slices = 1; A.p = p;
  return launch_line_class(A, (hipStream_t)stream, pot_u, pot_v);
}

static int line_esw_forward(const float* xs, const float* xt, const float* thetas, int pairs, int n, int m, int dim,
                            int slices, long theta_pair_stride, float p, const float* u_weights, const float* v_weights,
                            long u_weight_stride, long v_weight_stride, float* slice_cost, float* coef_s, float* coef_t,
                            float* pot_u, float* pot_v, void* stream) {
  if (!xs || !xt || !thetas || !slice_cost) return (int)hipErrorInvalidValue;
  if ((coef_s == nullptr) != (coef_t == nullptr)) return (int)hipErrorInvalidValue;
  if ((pot_u && !u_weights) || (pot_v && !v_weights)) return (int)hipErrorInvalidValue;
  if (!euclid_sizes_ok(kGridYPairs, pairs, n, m, dim, slices, theta_pair_stride) || !(p >= 1.f))
    return (int)hipErrorInvalidValue;
  if (!line_weights_ok(u_weights, u_weight_stride, n) || !line_weights_ok(v_weights, v_weight_stride, m))
    return (int)hipErrorInvalidValue;
  if (pairs == 0 || slices == 0) return 0;
  if ((long)pairs * slices > 0x7fffffffL) return (int)hipErrorInvalidValue;
  LineArgs A{};
  A.a = xs; A.b = xt; A.thetas = thetas; A.wa = u_weights; A.wb = v_weights;
  A.wa_stride = u_weight_stride; A.wb_stride = v_weight_stride;
  A.cost = slice_cost; A.coef_a = coef_s; A.coef_b = coef_t;
  A.rows = (long)pairs * slices; A.n = n; A.m = m; A.dim = dim; A.slices = slices;
  A.theta_pair_stride = theta_pair_stride; A.p = p;
  return launch_line_class(A, (hipStream_t)stream, pot_u, pot_v);
}

// the reduction over slices with weights shared by the pairs: rows per group of its first stage
constexpr int kLineReduceRows = 64;
inline long line_reduce_groups(long rows) { return (rows + kLineReduceRows - 1) / kLineReduceRows; }

}  // namespace shw

extern "C" {

int shw_line_rows_forward(const float* u, const float* v, long rows, int n, int m, float p, const float* u_weights,
                          const float* v_weights, long u_weight_stride, long v_weight_stride, float* row_cost,
                          float* coef_u, float* coef_v, void* stream) {
  return shw::line_rows_forward(u, v, rows, n, m, p, u_weights, v_weights, u_weight_stride, v_weight_stride, row_cost,
                                coef_u, coef_v, nullptr, nullptr, stream);
}

int shw_line_rows_forward_pot(const float* u, const float* v, long rows, int n, int m, float p, const float* u_weights,
                              const float* v_weights, long u_weight_stride, long v_weight_stride, float* row_cost,
                              float* coef_u, float* coef_v, float* pot_u, float* pot_v, void* stream) {
  return shw::line_rows_forward(u, v, rows, n, m, p, u_weights, v_weights, u_weight_stride, v_weight_stride, row_cost,
                                coef_u, coef_v, pot_u, pot_v, stream);
}

int shw_line_esw_forward(const float* xs, const float* xt, const float* thetas, int pairs, int n, int m, int dim,
                         int slices, long theta_pair_stride, float p, const float* u_weights, const float* v_weights,
                         long u_weight_stride, long v_weight_stride, float* slice_cost, float* coef_s, float* coef_t,
                         void* stream) {
  return shw::line_esw_forward(xs, xt, thetas, pairs, n, m, dim, slices, theta_pair_stride, p, u_weights, v_weights,
                               u_weight_stride, v_weight_stride, slice_cost, coef_s, coef_t, nullptr, nullptr, stream);
}

int shw_line_esw_forward_pot(const float* xs, const float* xt, const float* thetas, int pairs, int n, int m, int dim,
                             int slices, long theta_pair_stride, float p, const float* u_weights, const float* v_weights,
                             long u_weight_stride, long v_weight_stride, float* slice_cost, float* coef_s, float* coef_t,
                             float* pot_u, float* pot_v, void* stream) {
  return shw::line_esw_forward(xs, xt, thetas, pairs, n, m, dim, slices, theta_pair_stride, p, u_weights, v_weights,
                               u_weight_stride, v_weight_stride, slice_cost, coef_s, coef_t, pot_u, pot_v, stream);
}

size_t shw_line_weight_grads_workspace_bytes(int pairs, int slices, int count, int shared) {
  if (!shared || pairs < 0 || slices < 0 || count < 1) return 0;
  const long groups = shw::line_reduce_groups((long)pairs * slices);
  return groups > 1 ? (size_t)groups * count * sizeof(float) : 0;
}

int shw_line_weight_grads(const float* pot, const float* slice_w, int pairs, int slices, int count, int shared,
                          void* workspace, float* grad, void* stream) {
  if (!pot || !slice_w || !grad) return (int)hipErrorInvalidValue;
  if (pairs < 0 || pairs > 65535 || slices < 0 || count < 1 || count > shw::kMaxEuclidPoints) return (int)hipErrorInvalidValue;
  const long rows = (long)pairs * slices;
  if (rows > 0x7fffffffL) return (int)hipErrorInvalidValue;
  if (pairs == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned chunks = (count + 255) / 256;
  if (!shared) {                                               // one group per pair, straight into grad (pairs, count)
    hipLaunchKernelGGL(shw::line_weight_reduce_kernel, dim3(chunks, pairs), dim3(256), 0, st, pot, slice_w, rows, slices,
                       count, grad);
    return (int)hipGetLastError();
  }
  // shared: pairs and slices as one run of rows, in groups of kLineReduceRows; then the groups, in ascending order
  const long groups = shw::line_reduce_groups(rows);
  if (groups > 65535) return (int)hipErrorInvalidValue;
  if (groups <= 1) {
    hipLaunchKernelGGL(shw::line_weight_reduce_kernel, dim3(chunks, 1), dim3(256), 0, st, pot, slice_w, rows,
                       shw::kLineReduceRows, count, grad);
    return (int)hipGetLastError();
  }
  if (!workspace) return (int)hipErrorInvalidValue;
  float* partial = static_cast<float*>(workspace);
  hipLaunchKernelGGL(shw::line_weight_reduce_kernel, dim3(chunks, (unsigned)groups), dim3(256), 0, st, pot, slice_w, rows,
                     shw::kLineReduceRows, count, partial);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(shw::line_weight_reduce_kernel, dim3(chunks, 1), dim3(256), 0, st, (const float*)partial,
                     (const float*)nullptr, groups, (int)groups, count, grad);
  return (int)hipGetLastError();
}

int shw_line_esw_backward_points(const float* thetas, const float* coef_s, const float* coef_t, const float* slice_w,
                                 int pairs, int n, int m, int dim, int slices, long theta_pair_stride, float* grad_xs,
                                 float* grad_xt, void* stream) {
  if (!thetas || !coef_s || !coef_t || !slice_w || !grad_xs || !grad_xt) return (int)hipErrorInvalidValue;
  if (!shw::euclid_sizes_ok(shw::kGridYPairs, pairs, n, m, dim, slices, theta_pair_stride)) return (int)hipErrorInvalidValue;
  if (pairs == 0) return 0;
  return shw::launch_line_esw_backward_points(thetas, coef_s, coef_t, slice_w, pairs, n, m, dim, slices, theta_pair_stride,
                                              grad_xs, grad_xt, (hipStream_t)stream);
}

int shw_line_esw_backward_dirs(const float* xs, const float* xt, const float* coef_s, const float* coef_t,
                               const float* slice_w, int pairs, int n, int m, int dim, int slices, float* grad_thetas,
                               void* stream) {
  if (!xs || !xt || !coef_s || !coef_t || !slice_w || !grad_thetas) return (int)hipErrorInvalidValue;
  if (!shw::euclid_sizes_ok(shw::kGridYPairs, pairs, n, m, dim, slices, 0)) return (int)hipErrorInvalidValue;
  if (pairs == 0 || slices == 0) return 0;
  shw::with_coord_chunk(dim, [&](auto dc, unsigned z) {
    hipLaunchKernelGGL(shw::line_esw_backward_dirs_kernel<decltype(dc)::value>, dim3(slices, pairs, z), dim3(256), 0,
                       (hipStream_t)stream, xs, xt, coef_s, coef_t, slice_w, n, m, dim, slices, grad_thetas);
  });
  return (int)hipGetLastError();
}

}  // extern "C"
