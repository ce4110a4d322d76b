// general_cut.hpp -- general circular OT, solver (b) of general_common.hpp: weights, p != 1 -- the rotated target, the
// slopes and the cost at a cut, and the owner-computed gradient walks (the solve itself is in ssw_general_kernel).
#pragma once
#include "general_common.hpp"

#ifndef SHW_GENERAL_FIRST_GAIN
#define SHW_GENERAL_FIRST_GAIN 0.55f  // first step of the cut search at p = 2, in units of |slope|: Newton at curvature 2 is 0.5; stepping 10 % past it brackets the root at the second evaluation (measured 2.43 -> 2.35 ms; 0.6: 2.38, 0.7: 2.43)
#endif
#ifndef SHW_GENERAL_CHAINS
#define SHW_GENERAL_CHAINS 2    // interleaved rank walks per lane in the weighted slope evaluation
#endif

namespace shw {

// the target after moving mass theta around the circle (reference :31-48, evaluated lazily)
template <int EPT>
struct Rotated {
  Side<EPT> t;
  float turns, frac;
  int start;                               // number of wrapped atoms = first atom of the rotated order
  __device__ __forceinline__ void set(const Side<EPT>& target, float theta, int lane) {
    t = target;
    turns = floorf(theta);
    frac = theta - turns;
    // (cdf - frac) < 0  <=>  cdf < frac
    start = wave_lower_bound_arr<EPT>(target.cdf, target.count, frac, lane);
    if (start >= target.count) start = 0;  // degenerate (no atom left unwrapped): argmin over all-inf = 0
  }
  // atom j of the sorted target: shifted CDF and position unrolled onto the real line
  __device__ __forceinline__ void atom(int j, float& cdf, float& pos) const {
    const float sh = t.c(j) - frac;
    const bool wrapped = sh < 0.f;
    cdf = wrapped ? sh + 1.f : sh;
    pos = t.v(j) + (turns + (wrapped ? 1.f : 0.f));
  }
  // rotated index rho in [0, m]: rho = m is the appended copy of the first atom, one turn later
  __device__ __forceinline__ int source_index(int rho) const {
    const int j = rho + start;
    return j >= t.count ? j - t.count : j;
  }
  __device__ __forceinline__ float cdf_at(int rho) const { float c, p; atom(source_index(rho), c, p); return c; }
  __device__ __forceinline__ float pos_at(int rho) const {
    float c, p;
    if (rho >= t.count) { atom(start, c, p); return p + 1.f; }
    atom(source_index(rho), c, p);
    return p;
  }
  // number of rotated CDF entries strictly below key  == searchsorted(v_cdf_theta_rolled, key)
  __device__ __forceinline__ int below(float key) const {
    int lo = 0, hi = t.count;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const bool go = cdf_at(mid) < key;
      lo = go ? mid + 1 : lo;
      hi = go ? hi : mid;
    }
    return lo;
  }
  // the same for NB ASCENDING keys by a forward walk over the rotated entries (see walk_lower_bounds2; no restart:
  // the keys are source levels).  cnt_io: in, a count not above key[0]'s; out, the count of the last key.
  template <int NB>
  __device__ __forceinline__ void below_walk(const float (&key)[NB], int& cnt_io, int (&cnt)[NB]) const {
    const int m = t.count;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      int rounds = 0;
      for (;;) {
        float x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = cdf_at(min(cnt_io + q, m - 1));
        int adv = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) adv += ((cnt_io + q < m) && (x[q] < key[b])) ? 1 : 0;
        cnt_io += adv;
        if (__builtin_amdgcn_ballot_w64(adv == 4) == 0) break;
        if (++rounds >= kWalkRounds) {
          const float k1[1] = {key[b]};
          int c1[1];
          below_batch<1>(k1, c1);
          cnt_io = c1[0];
          break;
        }
      }
      cnt[b] = cnt_io;
    }
  }
  // the same for NB keys at once, fixed trip count (see lower_bounds2)
  template <int NB>
  __device__ __forceinline__ void below_batch(const float (&key)[NB], int (&cnt)[NB]) const {
    constexpr int P = EPT * kWave;
    const int m = t.count;
#pragma unroll
    for (int b = 0; b < NB; ++b) cnt[b] = 0;
#pragma unroll
    for (int st = P / 2; st >= 1; st >>= 1) {
      float x[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) x[b] = cdf_at(min(cnt[b] + st - 1, m - 1));
#pragma unroll
      for (int b = 0; b < NB; ++b) cnt[b] += ((cnt[b] + st - 1 < m) && (x[b] < key[b])) ? st : 0;
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const float x = cdf_at(min(cnt[b], m - 1));
      cnt[b] += ((cnt[b] < m) && (x < key[b])) ? 1 : 0;
    }
  }
};

// one-sided derivatives of the cost w.r.t. theta (reference dCost, :50-63), uniform over the slice's waves.
// tid: index of the thread among the 64 W threads of the slice; it owns target atoms [tid AP, (tid+1) AP), AP = EPT / W.
template <int EPT, int PMODE, int W>
__device__ void cut_slopes(const Side<EPT>& S, const Side<EPT>& T, float theta, int lane, int tid, float p,
                           int p_int, SliceTeam<W>& team, float& d_plus, float& d_minus) {
  constexpr int AP = EPT / W;
  Rotated<EPT> R;
  R.set(T, theta, lane);
  const int n = S.count, m = T.count;
  float sp = 0.f, sm = 0.f;
  constexpr int NA = AP < 8 ? AP : 8;                        // atoms searched together
  int walk_ptr = 0;                                          // rank of the thread's previous atom
  float walk_prev = 0.f;
  {
    float c0, p0;
    R.atom(min(tid * AP, m - 1), c0, p0);
    walk_ptr = lower_bound_arr<EPT>(S.cdf, n, c0);
    walk_prev = c0;
  }
#pragma nounroll
  for (int r0 = 0; r0 < AP; r0 += NA) {
    // NA + 1 consecutive atoms: atom a and its successor a + 1 (the atom after the last one is atom 0; indices
    // past the end repeat the last atom and are masked below)
    float wc[NA + 1], wp[NA + 1];
    int wj[NA + 1];
#pragma unroll
    for (int a = 0; a <= NA; ++a) {
      const int q = tid * AP + r0 + a;
      wj[a] = q < m ? q : (q == m ? 0 : m - 1);
      R.atom(wj[a], wc[a], wp[a]);
    }
    float cdf[NA], pos[NA], npos[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      cdf[a] = wc[a];
      pos[a] = wp[a];
      npos[a] = wp[a + 1] + ((wj[a + 1] == R.start) ? 1.f : 0.f);   // successor of the last rotated atom: first + 1
    }
    int lt[NA], le[NA];
    {
      bool alive[NA];
#pragma unroll
      for (int a = 0; a < NA; ++a) alive[a] = (tid * AP + r0 + a) < m;
      walk_lower_bounds2<EPT, NA>(S.cdf, n, cdf, alive, walk_prev, walk_ptr, lt, le);
    }
    const float v0 = S.v(0);
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const float al = S.v(min(lt[a], n - 1));               // left-continuous source quantile (:50-51)
      // right-continuous on the extended arrays (:54-57): past the last source level the quantile is the first
      // atom one turn later (the second extension, level c0 + 1, cannot be reached: cdf <= 1); unconditional read
      const float sv = S.v(min(le[a], n - 1));
      const float ar = le[a] < n ? sv : v0 + 1.f;
      const bool live = (tid * AP + r0 + a) < m;
      const float tp = powp<PMODE>(al - npos[a], p, p_int) - powp<PMODE>(al - pos[a], p, p_int);
      const float tm = powp<PMODE>(ar - npos[a], p, p_int) - powp<PMODE>(ar - pos[a], p, p_int);
      sp += live ? tp : 0.f;
      sm += live ? tm : 0.f;
    }
  }
  float sums[2] = {wave_sum_uniform(sp, lane), wave_sum_uniform(sm, lane)};
  team.sum(sums, lane);
  d_plus = sums[0];
  d_minus = sums[1];
}

// cut_slopes for weighted clouds as C interleaved walks (see walk_lower_bounds2): chain c covers atoms
// [c * AP/C, (c+1) * AP/C) of the thread's AP atoms, the C chains advance together -- 4 C independent reads per round, EPT/C
// rounds per evaluation -- and each chain's first rank is carried from one evaluation of the solve to the next
// (`anchor`; warm = false: binary search): the cut moves by less than a level spacing between late evaluations, so
// the carried rank is put right by one backward and one forward round instead of a 12-probe search.
template <int EPT, int PMODE, int C, int W>
__device__ void cut_slopes_walk(const Side<EPT>& S, const Side<EPT>& T, float theta, int lane, int tid, float p,
                                int p_int, SliceTeam<W>& team, float& d_plus, float& d_minus, int (&anchor)[C], bool warm,
                                float& cost_scale) {
  constexpr int AP = EPT / W;                                // atoms of the thread: [tid AP, (tid+1) AP)
  constexpr int LEN = AP / C;
  static_assert(AP % C == 0, "chains of equal length");
  Rotated<EPT> R;
  R.set(T, theta, lane);
  const int n = S.count, m = T.count;
  const float* arr = S.cdf;
  auto atom_q = [&](int q, float& c, float& ps, int& j) {    // atom q of the lane's run; q == m: atom 0, past it: the last
    j = q < m ? q : (q == m ? 0 : m - 1);
    R.atom(j, c, ps);
  };
  int ptr[C];
  float prev[C], own_c[C], own_p[C], mass[C];
  // ---- first ranks
#pragma unroll
  for (int c = 0; c < C; ++c) {
    int j;
    atom_q(tid * AP + c * LEN, own_c[c], own_p[c], j);
    prev[c] = own_c[c];
    ptr[c] = min(max(anchor[c], 0), n);
    float bc, bp;                                            // mass of the chain's first atom: level step from its predecessor
    R.atom(j > 0 ? j - 1 : m - 1, bc, bp);
    mass[c] = own_c[c] - bc;
    mass[c] += mass[c] < 0.f ? 1.f : 0.f;
  }
  if (warm) {                                                // backwards until the entry before ptr is below the key
    int rounds = 0;
    for (;;) {
      bool more = false;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        int back = 0;
        bool run = true;
#pragma unroll
        for (int q = 1; q <= 4; ++q) {
          const float x = arr[lds_slot<EPT>(max(ptr[c] - q, 0))];
          run = run && (ptr[c] - q >= 0) && !(x < prev[c]);
          back += run ? 1 : 0;
        }
        ptr[c] -= back;
        more |= back == 4;
      }
      if (__builtin_amdgcn_ballot_w64(more) == 0) break;
      if (++rounds >= kWalkRounds) { warm = false; break; }
    }
  }
  if (!warm) {
#pragma unroll
    for (int c = 0; c < C; ++c) ptr[c] = lower_bound_arr<EPT>(arr, n, prev[c]);
  }
  float sp = 0.f, sm = 0.f, sc = 0.f;
  const float v0 = S.v(0);
#pragma nounroll
  for (int i = 0; i < LEN; ++i) {
    float k[C], pos[C], npos[C], w[C];
    bool live[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int q = tid * AP + c * LEN + i;
      live[c] = q < m;
      pos[c] = own_p[c];
      k[c] = live[c] ? own_c[c] : prev[c];
      w[c] = mass[c];
      const float before = own_c[c];
      int nj;
      atom_q(q + 1, own_c[c], own_p[c], nj);                 // the successor: the chain's own atom of the next round
      mass[c] = own_c[c] - before;                           // levels are rotated by a common shift: steps survive, mod 1
      mass[c] += mass[c] < 0.f ? 1.f : 0.f;
      npos[c] = own_p[c] + ((nj == R.start) ? 1.f : 0.f);    // successor of the last rotated atom: first + 1
      ptr[c] = k[c] < prev[c] ? 0 : ptr[c];                  // the wrap: levels restart at ~0
      prev[c] = k[c];
    }
    int le[C];
    walk_window<EPT, C>(arr, n, k, ptr, le);
    if (i == 0) {
#pragma unroll
      for (int c = 0; c < C; ++c) anchor[c] = ptr[c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float al = S.v(min(ptr[c], n - 1));              // left-continuous source quantile (:50-51)
      const float sv = S.v(min(le[c], n - 1));               // right-continuous on the extended arrays (:54-57)
      const float ar = le[c] < n ? sv : v0 + 1.f;
      const float tp = powp<PMODE>(al - npos[c], p, p_int) - powp<PMODE>(al - pos[c], p, p_int);
      const float tm = powp<PMODE>(ar - npos[c], p, p_int) - powp<PMODE>(ar - pos[c], p, p_int);
      sp += live[c] ? tp : 0.f;
      sm += live[c] ? tm : 0.f;
      sc += live[c] ? w[c] * powp<PMODE>(al - pos[c], p, p_int) : 0.f;
    }
  }
  // sc: the cost with every target atom sent whole to the source quantile at its level: the size of the cost, for the
  // solve's exit test
  float sums[3] = {wave_sum_uniform(sp, lane), wave_sum_uniform(sm, lane), wave_sum_uniform(sc, lane)};
  team.sum(sums, lane);
  d_plus = sums[0];
  d_minus = sums[1];
  cost_scale = sums[2];
}

// transport cost at a fixed cut (reference Cost, :94-112), uniform over the slice's waves.  Thread tid evaluates the grid
// points of source atoms and of target atoms [tid AP, (tid+1) AP).
template <int EPT, int PMODE, int W>
__device__ float cut_cost(const Side<EPT>& S, const Side<EPT>& T, float theta, int lane, int tid, float p,
                          int p_int, SliceTeam<W>& team) {
  constexpr int AP = EPT / W;
  Rotated<EPT> R;
  R.set(T, theta, lane);
  const int n = S.count, m = T.count;
  float acc = 0.f;
  constexpr int NA = AP < 8 ? AP : 8;                        // atoms searched together
  int walk_cnt = 0, walk_ptr = 0;                            // ranks of the thread's previous atoms
  float walk_prev = 0.f;
  {
    const float k1[1] = {S.c(min(tid * AP, n - 1))};
    int c1[1];
    R.template below_batch<1>(k1, c1);
    walk_cnt = c1[0];
    float c0, p0;
    R.atom(min(tid * AP, m - 1), c0, p0);
    walk_ptr = lower_bound_arr<EPT>(S.cdf, n, c0);
    walk_prev = c0;
  }
#pragma nounroll
  for (int r0 = 0; r0 < AP; r0 += NA) {
    {  // grid points = source CDF levels A_e
      float g[NA];
      int cnt[NA];
#pragma unroll
      for (int a = 0; a < NA; ++a) g[a] = S.c(min(tid * AP + r0 + a, n - 1));
      R.template below_walk<NA>(g, walk_cnt, cnt);             // rotated target atom active at g
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const int e = tid * AP + r0 + a;
        const bool live = e < n;
        const int ec = min(e, n - 1);
        const float b = R.pos_at(min(cnt[a], m));
        const float prev_a = ec > 0 ? S.c(ec - 1) : 0.f;
        const float prev_c = cnt[a] > 0 ? R.cdf_at(cnt[a] - 1) : 0.f;
        const float width = g[a] - fmaxf(prev_a, prev_c);
        const float d = S.v(ec) - b;
        acc += live ? width * powp<PMODE>(d, p, p_int) : 0.f;
      }
    }
    {  // grid points = shifted target CDF levels C_e
      float g[NA], b[NA];
      int lt[NA], le[NA];
#pragma unroll
      for (int a = 0; a < NA; ++a) R.atom(min(tid * AP + r0 + a, m - 1), g[a], b[a]);
      if constexpr (general_walks<EPT>()) {                  // window reads (the rows under the source CDF exist)
#pragma unroll
        for (int a = 0; a < NA; ++a) {
          const float k1[1] = {g[a]};
          int p1[1] = {g[a] < walk_prev ? 0 : walk_ptr}, l1[1];    // (the wrap: levels restart at ~0)
          walk_prev = g[a];
          walk_window<EPT, 1>(S.cdf, n, k1, p1, l1);
          walk_ptr = p1[0];
          lt[a] = p1[0];
          le[a] = l1[0];
        }
      } else {
        bool alive[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a) alive[a] = true;        // (indices past the end repeat the last atom: keys ascend)
        walk_lower_bounds2<EPT, NA>(S.cdf, n, g, alive, walk_prev, walk_ptr, lt, le);
      }
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const int e = tid * AP + r0 + a;
        const bool live = e < m;
        const int ec = min(e, m - 1);
        const int rho = ec >= R.start ? ec - R.start : ec - R.start + m;
        const int il = min(lt[a], n - 1);
        const float av = S.v(il);
        const int na = le[a];                                // source levels <= g sort before g in the merged grid
        const float prev_a = na > 0 ? S.c(na - 1) : 0.f;
        const float prev_c = rho > 0 ? R.cdf_at(rho - 1) : 0.f;
        const float width = g[a] - fmaxf(prev_a, prev_c);
        const float d = av - b[a];
        acc += live ? width * powp<PMODE>(d, p, p_int) : 0.f;
      }
    }
  }
  float sums[1] = {wave_sum_uniform(acc, lane)};
  team.sum(sums, lane);
  return sums[0];
}

// ---------------------------------------------------------------------------------------------
// Gradient of Cost at the (detached) cut, OWNER-COMPUTED (round 3).  The merged CDF grid of Cost (:95-105) cuts [0, 1]
// into segments; on each one source atom i and one rotated target atom rho are active, and the segment adds
// width * |u_i - v_rho|^p to the cost, width * d|D|^p/dD to the coefficient of atom i and its negative to atom rho's.
// Round 2 accumulated both with LDS float atomics (sum order, hence the last bits, varied between runs).  Here every
// atom has ONE owner that walks the segments of the atom's own mass interval -- a two-pointer merge of its interval
// with the other cloud's levels, one segment per step -- accumulates in a register and writes the coefficient once:
//   walk_source_atoms : thread tid owns sorted source atoms [tid AP, (tid+1) AP); atom e's interval is
//                       (A_{e-1}, A_e], crossed by the rotated target levels C_rho inside it.  Also returns the
//                       thread's share of the cost (every segment belongs to exactly one source atom; the segments
//                       above the last source level -- rounding -- go to the last atom like the reference's clip).
//   walk_target_atoms : thread tid owns ROTATED target atoms [tid AP, (tid+1) AP) (the rotated order is the order of
//                       their levels); the owner of the last one also walks the tail (C_{m-1}, 1], where the active
//                       target atom is the appended copy of the first rotated atom one turn later (:48, :103): its
//                       coefficient belongs to that first atom and is handed over in `tail` (added in a fixed order).
// A step costs ~20 VALU + 3 LDS reads; a thread takes ~2 AP steps (its atoms + the foreign levels in its range), and
// threads are balanced because equal counts of atoms hold nearly equal mass.  Ties (a source level equal to a target
// level) advance the source first; the leftover segment has width 0 -- the reference's merged grid gives the duplicate
// grid point a zero delta too.
// ---------------------------------------------------------------------------------------------
template <int EPT, int PMODE, int W>
__device__ float walk_source_atoms(const Side<EPT>& S, const Rotated<EPT>& R, int tid, float p, int p_int,
                                   float* gs) {
  constexpr int AP = EPT / W;
  const int n = S.count, m = R.t.count;
  const float inf = __builtin_inff();
  int e = tid * AP;
  const int e_end = min(e + AP, n);
  bool active = e < e_end;
  const int e0 = min(e, n - 1);
  float a_prev = e0 > 0 ? S.c(e0 - 1) : 0.f;
  int rho = active ? (e0 > 0 ? R.below(a_prev) : 0) : m;
  float c_prev = rho > 0 ? R.cdf_at(min(rho, m) - 1) : 0.f;
  float a = S.c(e0), u = S.v(e0);
  float c = rho < m ? R.cdf_at(rho) : inf;
  float pos = R.pos_at(min(rho, m));
  float acc = 0.f, cost = 0.f;
  bool extended = false;                                     // the last source atom also takes the levels above A_{n-1}
  for (int guard = 0; guard < 2 * kWave * EPT + 8; ++guard) {
    if (__builtin_amdgcn_ballot_w64(active) == 0) break;
    if (active) {
      const float end = fminf(a, c);                         // (+inf: no level left on either side -- nothing to add)
      const float width = end < inf ? fmaxf(end - fmaxf(a_prev, c_prev), 0.f) : 0.f;
      const float d = u - pos;
      acc = fmaf(width, dpow_abs<PMODE>(d, p, p_int), acc);
      cost = fmaf(width, powp<PMODE>(d, p, p_int), cost);
      if (c < a) {                                           // the segment ended on a target level: next target atom
        c_prev = c;
        ++rho;
        c = rho < m ? R.cdf_at(rho) : inf;
        pos = R.pos_at(min(rho, m));
      } else if (e == n - 1 && !extended) {                  // (u_index.clip(0, n-1), :101)
        extended = true;
        a_prev = a;
        a = inf;
      } else {                                               // the atom's interval is done: its coefficient, once
        gs[lds_slot<EPT>(e)] = acc;
        acc = 0.f;
        a_prev = a;
        ++e;
        active = e < e_end;
        const int ec = min(e, n - 1);
        a = S.c(ec);
        u = S.v(ec);
      }
    }
  }
  return cost;
}

template <int EPT, int PMODE, int W>
__device__ void walk_target_atoms(const Side<EPT>& S, const Rotated<EPT>& R, int tid, float p, int p_int,
                                  float* gt, float* tail) {
  constexpr int AP = EPT / W;
  const int n = S.count, m = R.t.count;
  const float inf = __builtin_inff();
  int rho = tid * AP;
  const int rho_end = min(rho + AP, m);
  const bool owns_tail = (rho < m) && (rho_end == m);        // owner of the last rotated atom
  bool active = rho < rho_end;
  const int r0 = min(rho, m - 1);
  float c_prev = r0 > 0 ? R.cdf_at(r0 - 1) : 0.f;
  int i = active ? (r0 > 0 ? S.below(c_prev, true) : 0) : n;
  float a_prev = i > 0 ? S.c(min(i, n) - 1) : 0.f;
  float a = i < n ? S.c(i) : inf, u = S.v(min(i, n - 1));
  float c = R.cdf_at(r0), pos = R.pos_at(r0);
  float acc = 0.f;
  for (int guard = 0; guard < 2 * kWave * EPT + 8; ++guard) {
    if (__builtin_amdgcn_ballot_w64(active) == 0) break;
    if (active) {
      const float end = fminf(a, c);                         // (+inf: the tail beyond the last source level is empty)
      const float width = end < inf ? fmaxf(end - fmaxf(a_prev, c_prev), 0.f) : 0.f;
      acc = fmaf(width, dpow_abs<PMODE>(u - pos, p, p_int), acc);
      if (i < n && a <= c) {                                 // the segment ended on a source level: next source atom
        a_prev = a;
        ++i;
        a = i < n ? S.c(i) : inf;
        u = S.v(min(i, n - 1));
      } else {                                               // the atom's interval is done
        if (rho < m) gt[lds_slot<EPT>(R.source_index(rho))] = -acc;
        else *tail = -acc;                                   // the appended copy: belongs to the first rotated atom
        acc = 0.f;
        c_prev = c;
        ++rho;
        active = rho < rho_end || (owns_tail && rho == m);
        c = rho < m ? R.cdf_at(rho) : inf;
        pos = R.pos_at(min(rho, m));
      }
    }
  }
}

}  // namespace shw
