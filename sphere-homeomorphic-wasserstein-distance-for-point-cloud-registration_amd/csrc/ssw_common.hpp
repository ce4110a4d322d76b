// ssw_common.hpp -- shared device code of the spherical sliced-Wasserstein hot path for MI355X (gfx950, wave64).
//
// One 64-lane wavefront owns one (pair, slice): it projects both clouds of the pair onto the
// slice's great circle, sorts both coordinate arrays in registers (wave_sort.hpp), parks the sorted
// target in LDS and solves the circular optimal-transport problem against the sorted source that
// stays in registers.  No barrier, no inter-wave communication, no MFMA (there is no contraction).
//
// Reference being replaced (paths relative to /root/reference/Point_Cloud_Resistration/losses/):
//   sliced_cost            max_spherical_sliced_w.py:251-286, _fast.py:258-295
//   binary_search_circle   :117-207   (p != 1)      emd1D_circle :210-247 (p == 1)
// The p != 1 solve uses the equivalence of SURVEY.md 8a row A8: for n == m and uniform weights the
// value the reference's bisection converges to is  min_k c(k),
//     c(k) = (1/n) sum_i |u_(i) - v_ext(i+k)|^p ,  v_ext(q) = v_(q mod n) + floor(q/n),
// a convex sequence in k.  The kernel starts at k0 = round(sum u - sum v) (exact minimiser when the
// target atoms are equally spaced, since sum_i (u_(i) - v_ext(i+k)) = sum u - sum v - k) and walks
// the convex sequence by galloping + bisection on the sign of c(k+1) - c(k).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/shw.h"
#include "dispatch.hpp"
#include "wave_sort.hpp"

#ifndef SHW_INC_MASK_BY_EXEC
#define SHW_INC_MASK_BY_EXEC 1
#endif
#ifndef SHW_SOLVE_INC
#define SHW_SOLVE_INC 1
#endif
#ifndef SHW_GRAD2_INC
#define SHW_GRAD2_INC 1
#endif
#ifndef SHW_MASK_BY_EXEC
#define SHW_MASK_BY_EXEC 1      // pads of a partially filled class masked by exec (a kept branch) instead of three selects
#endif

namespace shw {

struct SswArgs {
  const float* xs;
  const float* xt;
  const float* dirs;
  float* slice_cost;
  int32_t* slice_shift;
  float* coef_s;   // forward_grad only
  float* coef_t;
  int pairs, n, m, slices;
  int pstride;     // floats per point: 3 (clouds, projected on the slice's frame) or 1 (rows of circle coordinates: the
                   // circle-level entry point shw_circle_ot; dirs is NULL then and a "pair" is one row)
  long u_pair_stride;
  float p;
  int p_int;       // p if p is a small integer (1..8), else 0
  int bisect_p1;   // p == 1 only: 1 = the reference's BISECTION at p = 1 (binary_search_circle's default p, :117, ending in
                   // Cost's p == 1 branch :107-108) instead of the level-median formula of emd1D_circle; set by shw_circle_ot
  int num_groups;  // workgroups launched (for the XCD remap)
};

// ---------------------------------------------------------------------------------------------
// XCD-aware workgroup renumbering: hardware deals workgroups round-robin over the 8 XCDs
// (blockIdx % 8 labels the XCD); give every XCD one contiguous range of (pair, slice) work so the
// two clouds of a pair are fetched into ONE XCD's L2 instead of eight.  Bijective for any count.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int xcd_contiguous_id(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7;
  const int xcd = bid & 7, idx = bid >> 3;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + idx;
}

// The slice's frame U (3,2) row-major, wave-uniform.  Coordinate-row mode (dirs == NULL): U[0] = NaN tells load_coords to
// take the input values as circle coordinates.
__device__ __forceinline__ void load_frame(const float* dirs, long offset, float (&U)[6]) {
  if (dirs) {
    const float* Ul = dirs + offset;
#pragma unroll
    for (int i = 0; i < 6; ++i) U[i] = Ul[i];
  } else {
#pragma unroll
    for (int i = 0; i < 6; ++i) U[i] = __builtin_nanf("");
  }
}

// circle coordinate of one projected point (reference :274-279):
//     coord = (atan2(-b, -a) + pi) / (2 pi)
// F.normalize (:274-275) is a positive rescale and cannot change the angle, so it is skipped.
// The coordinate is measured in turns from the start, with no angle in radians in between:
//     coord = K + sigma r',     r' = atan(mn / mx) / (2 pi) in [0, 1/8],  mn = min(|a|, |b|),  mx = max(|a|, |b|)
// r' = t q(t^2), t = mn / mx, q the degree-14 even polynomial whose coefficients are 1 / (2 pi) times those of the
// degree-15 odd minimax arctangent (1, c3 .. c15), scaled in double and rounded once.  K and sigma depend only on
// (A, B, S) = (sign bit of a, sign bit of b, |b| > |a|).  With alpha = 1 - 2 A, beta = 1 - 2 B, gamma = 1 - 2 S the three
// reflections of atan2 (about the diagonal, about the y-axis, about the x-axis) compose to sigma = alpha beta gamma and
//     (A, B, S)   000  001  010  011  100  101  110  111
//     8 K           0    2    8    6    4    2    4    6        (coord = 0 + r', 1/4 - r', 1 - r', 3/4 + r', ...)
// which is K = 1/2 - beta / 4 - alpha beta / 8 - alpha beta gamma / 8, hence
//     coord = ((1/2 - beta / 4) - alpha beta / 8) + alpha beta gamma (r' - 1/8).
// Every sign is one XOR of sign bits onto a constant or onto r' - 1/8 (full-rate bit operations: no compare, no select).
// S is the sign bit of |a| - |b| (clear when they are equal: the diagonal belongs to the octant next to the x-axis).
// Signed zeros follow the IEEE rules of atan2(-b, -a) that the reference relies on, through the sign BITS of a and b:
// (+0, +0) -> +0, (-0, +-0) -> 1/2, (+0, -0) -> 1; points on the axes land on 0, 1/4, 1/2, 3/4, 1 exactly (r' = 0).
// Error: the partial sums 1/2 - beta / 4 - alpha beta / 8 are multiples of 1/8 and exact; r' - 1/8 = fma(t, q, -1/8) lies
// in [-1/8, 0] and rounds once, by at most 2^-28 (2^-29 once r' > 1/16), so what remains is the error of t and q (1.5-ulp
// quotient, polynomial) and the rounding of the last add (<= 2^-25 in [1/2, 1)): <= 6e-8 in coordinate units against
// float64 atan2, rms 1.5e-8, measured over 2.2e7 points by the numpy restatement in tests/test_circle_coord_cpu.py (on
// the device, with its 1-ulp reciprocal: tests/test_circle_coord_gpu.py).
// Range: q(1) sums to 0.12499998 <= 1/8 and t q is largest at t = 1 (the restatement checks the 2e5 floats below 1 too),
// so r' - 1/8 is in [-1/8, +0] and never changes sign.  The exact partial sum is the octant's diagonal seam (1/8, 3/8,
// 5/8 or 7/8), and sigma (r' - 1/8) leads from it towards the octant's axis, at most 1/8 away, and never to the
// diagonal's other side: every coordinate is in [0, 1], the domain of the bin map of bin_sort.hpp, and the octants meet
// in order at all eight seams.
// Domain note: |a|,|b| below 1e-37 (denormal-scale projections) are treated as if max(|a|,|b|) were
// 1e-37, i.e. the angle of such a vector is not resolved; exact zeros are handled exactly.
__device__ __forceinline__ float circle_coord(float a, float b) {
  const float ax = fabsf(a), ay = fabsf(b);
  const float mx = fmaxf(fmaxf(ax, ay), 1e-37f), mn = fminf(ax, ay);
  const float t = mn * __builtin_amdgcn_rcpf(mx);  // v_rcp_f32 (1 ulp) * mn: t = mn/mx to 1.5 ulp
  const float s = t * t;
  float q = -6.9318414899e-04f;
  q = fmaf(q, s, 3.6669510882e-03f);
  q = fmaf(q, s, -9.1949515045e-03f);
  q = fmaf(q, s, 1.5588007867e-02f);
  q = fmaf(q, s, -2.2244419903e-02f);
  q = fmaf(q, s, 3.1771630049e-02f);
  q = fmaf(q, s, -5.3048983216e-02f);
  q = fmaf(q, s, 1.5915493667e-01f);
  const float d = fmaf(t, q, -0.125f);             // r' - 1/8, r' = t q = atan(mn/mx) / (2 pi): one rounding, in [-1/8, +0]
  const uint32_t sg = 0x80000000u;
  const uint32_t ia = __builtin_bit_cast(uint32_t, a), ib = __builtin_bit_cast(uint32_t, b);
  const uint32_t id = __builtin_bit_cast(uint32_t, ax - ay), x2 = ia ^ ib;
  const float w1 = __builtin_bit_cast(float, 0xBE800000u ^ (ib & sg));                      // -beta / 4
  const float w2 = __builtin_bit_cast(float, 0xBE000000u ^ (x2 & sg));                      // -alpha beta / 8
  const float t3 = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, d) ^ ((x2 ^ id) & sg));   // alpha beta gamma d
  return ((0.5f + w1) + w2) + t3;
}

// |d|^p.  PMODE 2: p == 2 (the reference's own call sites all use p = 2); PMODE 0: any p >= 1,
// small integer powers by repeated multiplication, otherwise powf.
template <int PMODE>
__device__ __forceinline__ float pow_abs(float d, float p, int p_int) {
  if constexpr (PMODE == 2) {
    return d * d;
  } else {
    const float a = fabsf(d);
    if (p_int > 0) {
      float r = a;
      for (int i = 1; i < p_int; ++i) r *= a;
      return r;
    }
    return powf(a, p);
  }
}

// d/dD |D|^p
template <int PMODE>
__device__ __forceinline__ float dpow_abs(float d, float p, int p_int) {
  if constexpr (PMODE == 2) {
    return 2.f * d;
  } else {
    const float a = fabsf(d);
    float r;
    if (p_int > 0) {
      r = 1.f;
      for (int i = 1; i < p_int; ++i) r *= a;
    } else {
      r = (a > 0.f) ? powf(a, p - 1.f) : 0.f;
    }
    return (a > 0.f) ? copysignf(p * r, d) : 0.f;
  }
}

// sorted target in LDS: sorted position q lives at [(q % EPT) * 64 + q / EPT]  (= register r of
// lane q/EPT, written with one conflict-free ds_write per register).
// NCOL = number of columns = lanes that hold the sorted array: 64 for one wave, 64*W when W waves of a
// workgroup sort one slice together (shw_ssw_fwd.hip, multi-wave kernel).
template <int EPT, int NCOL = 64>
__device__ __forceinline__ int lds_slot(int q) {
  if constexpr (is_pow2(EPT)) {
    constexpr int LOG = __builtin_ctz(EPT);
    return (q & (EPT - 1)) * NCOL + (q >> LOG);
  } else {                                          // (q >= 0: division by a constant)
    const unsigned col = (unsigned)q / (unsigned)EPT;
    return (int)(((unsigned)q - col * (unsigned)EPT) * (unsigned)NCOL + col);
  }
}

// floor(x / EPT) and x - EPT floor(x / EPT) for x >= -1024 EPT: shift and mask for the power-of-two classes
template <int EPT>
__device__ __forceinline__ int ediv(int x) {
  if constexpr (is_pow2(EPT)) return x >> __builtin_ctz(EPT);
  else return (int)((unsigned)(x + 1024 * EPT) / (unsigned)EPT) - 1024;
}
template <int EPT>
__device__ __forceinline__ int emod(int x) {
  if constexpr (is_pow2(EPT)) return x & (EPT - 1);
  else return x - ediv<EPT>(x) * EPT;
}

// v_ext(q) for q in [-2n, 3n): branch-free wrap onto [0, n) with the turn offset (two turns each
// way: the shift k ranges over [-n, n] and its neighbours k-1, k+1 are evaluated alongside)
template <int EPT, int NCOL = 64>
__device__ __forceinline__ float target_unrolled(const float* vbuf, int q, int n) {
  const int t1 = (q < 0) ? -1 : ((q >= n) ? 1 : 0);
  q -= t1 * n;
  const int t2 = (q < 0) ? -1 : ((q >= n) ? 1 : 0);
  q -= t2 * n;
  return vbuf[lds_slot<EPT, NCOL>(q)] + (float)(t1 + t2);
}

// c(k-1), c(k), c(k+1) (sums, not yet divided by n), valid in every lane.
// Lane owns sorted positions e0 .. e0+EPT-1 and needs v_ext(e0+k-1 .. e0+k+EPT): a sliding window,
// fetched 8 positions at a time to bound the registers in flight.
// `lane` is the index of the lane among the NCOL lanes that hold the slice (wave * 64 + lane in the multi-wave
// kernel, whose waves then add their partial sums).
// NR / r_base: the evaluation may cover only registers [r_base, r_base + NR) of every lane's EPT sorted positions
// (u then holds those NR atoms): the two-wave training kernel gives each wave half of the source.
template <int EPT, int PMODE, int NCOL = 64, int NR = EPT>
__device__ __forceinline__ void shift_costs3(const float (&u)[NR], const float* vbuf, int lane, int n,
                                             int k, float p, int p_int, float& cm, float& c0, float& cp,
                                             int r_base = 0) {
  float sm = 0.f, s0 = 0.f, sp = 0.f;
  const int e0 = lane * EPT + r_base;
  const int last = n - 1;
  float prev = target_unrolled<EPT, NCOL>(vbuf, min(e0, last) + k - 1, n);
  float cur = target_unrolled<EPT, NCOL>(vbuf, min(e0, last) + k, n);
  constexpr int CH = chunk_of(NR);
#pragma unroll
  for (int r0 = 0; r0 < NR; r0 += CH) {
    float nxt[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) nxt[j] = target_unrolled<EPT, NCOL>(vbuf, min(e0 + r0 + j, last) + k + 1, n);
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const bool live = (e0 + r0 + j) < n;
      const float a = pow_abs<PMODE>(u[r0 + j] - prev, p, p_int);
      const float b = pow_abs<PMODE>(u[r0 + j] - cur, p, p_int);
      const float c = pow_abs<PMODE>(u[r0 + j] - nxt[j], p, p_int);
      sm += live ? a : 0.f;
      s0 += live ? b : 0.f;
      sp += live ? c : 0.f;
      prev = cur;
      cur = nxt[j];
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  cm = wave_sum_uniform(sm, lane & 63);
  c0 = wave_sum_uniform(s0, lane & 63);
  cp = wave_sum_uniform(sp, lane & 63);
}

// c(kk) alone, as shift_costs3 forms each of its three sums: the term of register j reads the same target position
// e0 + j + kk (for every live j) and is added in the same order, then the same wave_sum_uniform -- so the result has
// the bits of the cm / c0 / cp that a three-shift evaluation at kk + 1 / kk / kk - 1 returns.  solve_shift uses it after a
// unit step, where two of the three costs are already known.
template <int EPT, int PMODE, int NCOL = 64, int NR = EPT>
__device__ __forceinline__ float shift_cost1(const float (&u)[NR], const float* vbuf, int lane, int n, int kk, float p,
                                             int p_int, int r_base = 0) {
  float s = 0.f;
  const int e0 = lane * EPT + r_base;
  const int last = n - 1;
  constexpr int CH = chunk_of(NR);
#pragma unroll
  for (int r0 = 0; r0 < NR; r0 += CH) {
    float v[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) v[j] = target_unrolled<EPT, NCOL>(vbuf, min(e0 + r0 + j, last) + kk, n);
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const bool live = (e0 + r0 + j) < n;
      const float a = pow_abs<PMODE>(u[r0 + j] - v[j], p, p_int);
      s += live ? a : 0.f;
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  return wave_sum_uniform(s, lane & 63);
}

// one fetch of shift_costs3_inc (arguments by value: as captured references the offsets end up as a table in scratch
// memory read through flat pointers)
__device__ __forceinline__ float inc_fetch(const char* row, bool before_turn, bool first_column, int a0, int a1, int b0,
                                           float t0, float tw) {
  const int a = before_turn ? (first_column ? a0 : a1) : b0;
  return *reinterpret_cast<const float*>(row + a) + (before_turn ? t0 : tw);
}
// the last fetch of a window of EPT + 2 positions (one-wave kernels): it may lie in the third column of the window, or in
// the second one after the end of the circle
__device__ __forceinline__ float inc_fetch_last(const char* row, bool before_turn, bool second_column, bool second_after_turn,
                                                int a1, int a2, int b0, int b1, float t0, float tw) {
  const int a = before_turn ? (second_column ? a1 : a2) : (second_after_turn ? b1 : b0);
  return *reinterpret_cast<const float*>(row + a) + (before_turn ? t0 : tw);
}

// shift_costs3 for any n with 6 VALU per fetched target atom instead of the ~15 of target_unrolled.  The window of a
// lane (NR + 2 consecutive positions) starts at slot (row0, col0) of the plain rows; while it is no longer than one column
// (NR + 2 <= EPT: the two-wave training kernel, NR = EPT/2) it meets at most one end of column (the address drops by a
// constant) and at most one end of the circle (position n: it restarts at slot (0, 0) one turn further on, and is then too
// short to meet anything else).  With the two per-lane thresholds jr = EPT - row0 and jn = n - q0 prepared once, fetch j is
//     ds_read(j*256 + (j < jn ? (j < jr ? A0 : A1) : B0)) + (j < jn ? t0 : t0 + 1).
// A window of EPT + 2 positions (NR = EPT: the one-wave kernels) can reach one column further with its LAST position only
// (jr >= 1, jn >= 1), which gets its own form.  Pads are masked by exec as in shift_costs3_ext.
template <int EPT, int PMODE, int NCOL = 64, int NR = EPT>
__device__ __forceinline__ void shift_costs3_inc(const float (&u)[NR], const float* vbuf, int lane, int n,
                                                 int k, float p, int p_int, float& cm, float& c0, float& cp,
                                                 int r_base = 0) {
  static_assert(NR <= EPT, "a window of at most EPT + 2 positions");
  int q = lane * EPT + r_base + k - 1;              // in [-n - 1, 64 EPT + n) within [-2n, 3n): two turns at most
  const int t1 = (q < 0) ? -1 : ((q >= n) ? 1 : 0);
  q -= t1 * n;
  const int t2 = (q < 0) ? -1 : ((q >= n) ? 1 : 0);
  q -= t2 * n;
  const float t0 = (float)(t1 + t2), tw = t0 + 1.f;
  const int col0 = ediv<EPT>(q), row0 = q - col0 * EPT;
  const int jr = EPT - row0, jn = n - q;
  constexpr int RB = NCOL * 4;                      // bytes per row
  const int A0 = row0 * RB + (col0 << 2);
  const int A1 = A0 + 4 - EPT * RB;
  const int B0 = -jn * RB;
  const char* rows = reinterpret_cast<const char*>(vbuf);
  auto fetch = [&](int j) -> float {                // j compile-time after unrolling
    if (j <= EPT) return inc_fetch(rows + j * RB, j < jn, j < jr, A0, A1, B0, t0, tw);
    return inc_fetch_last(rows + j * RB, j < jn, j < jr + EPT, j >= jn + EPT, A1, A1 + 4 - EPT * RB, B0, B0 + 4 - EPT * RB,
                          t0, tw);
  };
  const int live_regs = n - lane * EPT - r_base;
  float sm = 0.f, s0 = 0.f, sp = 0.f;
  float prev = fetch(0), cur = fetch(1);
  constexpr int CH = chunk_of(NR);
#pragma unroll
  for (int r0 = 0; r0 < NR; r0 += CH) {
    float nxt[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) nxt[j] = fetch(r0 + j + 2);
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const float a = pow_abs<PMODE>(u[r0 + j] - prev, p, p_int);
      const float b = pow_abs<PMODE>(u[r0 + j] - cur, p, p_int);
      const float c = pow_abs<PMODE>(u[r0 + j] - nxt[j], p, p_int);
#if SHW_INC_MASK_BY_EXEC
      if ((r0 + j) < live_regs) {
        asm volatile("" : "+v"(sm), "+v"(s0), "+v"(sp));
        sm += a; s0 += b; sp += c;
      }
#else
      const bool live = (r0 + j) < live_regs;
      sm += live ? a : 0.f;
      s0 += live ? b : 0.f;
      sp += live ? c : 0.f;
#endif
      prev = cur;
      cur = nxt[j];
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  cm = wave_sum_uniform(sm, lane & 63);
  c0 = wave_sum_uniform(s0, lane & 63);
  cp = wave_sum_uniform(sp, lane & 63);
}

// Fast form of shift_costs3 for n == 64*EPT exactly (every register slot is a real atom, n a power of
// two).  With base = k-1 = kh*EPT + kl (0 <= kl < EPT) the window position j of lane l is sorted
// position (l + kh + c)*EPT + row with  row = (kl + j) mod EPT  and carry  c = (kl + j) div EPT in
// {0,1,2}: row and c are WAVE-UNIFORM, so each fetch is  ds_read(addr_c + row*256) + turn_c  with the
// three per-lane (address, turn) pairs prepared once per evaluation -- 4 VALU per fetch instead of ~15.
template <int EPT, int PMODE, int NCOL = 64, int NR = EPT>
__device__ __forceinline__ void shift_costs3_full(const float (&u)[NR], const float* vbuf, int lane, int k,
                                                  float p, int p_int, float& cm, float& c0, float& cp,
                                                  int r_base = 0) {
  constexpr int LOG = __builtin_ctz(EPT);
  const int base = k - 1 + r_base;            // registers [r_base, r_base + NR): the same window, r_base further on
  const int kl = base & (EPT - 1);
  const int kh = base >> LOG;                                   // floor division (arithmetic shift)
  int addr[3];
  float turn[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int col = lane + kh + c;                              // unwrapped lane index of the atom
    addr[c] = (col & (NCOL - 1)) << 2;                          // byte offset inside an LDS row
    turn[c] = (float)(col >> __builtin_ctz(NCOL));              // whole turns around the circle
  }
  const char* rows = reinterpret_cast<const char*>(vbuf);
  auto fetch = [&](int j) -> float {                            // j compile-time after unrolling
    const int rj = kl + j;                                      // scalar
    const int row = rj & (EPT - 1);
    const bool carry = (j < EPT) ? (rj >= EPT) : (rj >= 2 * EPT);
    const int a = (j < EPT) ? (carry ? addr[1] : addr[0]) : (carry ? addr[2] : addr[1]);
    const float t = (j < EPT) ? (carry ? turn[1] : turn[0]) : (carry ? turn[2] : turn[1]);
    return *reinterpret_cast<const float*>(rows + a + row * (NCOL * 4)) + t;
  };
  float sm = 0.f, s0 = 0.f, sp = 0.f;
  float prev = fetch(0), cur = fetch(1);
  constexpr int CH = NR < 8 ? NR : 8;
#pragma unroll
  for (int r0 = 0; r0 < NR; r0 += CH) {
    float nxt[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) nxt[j] = fetch(r0 + j + 2);
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      sm += pow_abs<PMODE>(u[r0 + j] - prev, p, p_int);
      s0 += pow_abs<PMODE>(u[r0 + j] - cur, p, p_int);
      sp += pow_abs<PMODE>(u[r0 + j] - nxt[j], p, p_int);
      prev = cur;
      cur = nxt[j];
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  cm = wave_sum_uniform(sm, lane & 63);
  c0 = wave_sum_uniform(s0, lane & 63);
  cp = wave_sum_uniform(sp, lane & 63);
}

// c(kk) alone for n == 64*EPT (shift_cost1 in the addressing of shift_costs3_full): the window starts at kk instead of
// k - 1 and is EPT long, so the carry is 0 or 1.  A position's (column, row, turn) do not depend on where the window
// starts: the terms, their order and the reduction are those of the three-shift form.
template <int EPT, int PMODE, int NCOL = 64, int NR = EPT>
__device__ __forceinline__ float shift_cost1_full(const float (&u)[NR], const float* vbuf, int lane, int kk, float p,
                                                  int p_int, int r_base = 0) {
  constexpr int LOG = __builtin_ctz(EPT);
  const int base = kk + r_base;
  const int kl = base & (EPT - 1);
  const int kh = base >> LOG;
  int addr[2];
  float turn[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int col = lane + kh + c;
    addr[c] = (col & (NCOL - 1)) << 2;
    turn[c] = (float)(col >> __builtin_ctz(NCOL));
  }
  const char* rows = reinterpret_cast<const char*>(vbuf);
  auto fetch = [&](int j) -> float {                            // j compile-time after unrolling
    const int rj = kl + j;                                      // scalar
    const bool carry = rj >= EPT;
    return *reinterpret_cast<const float*>(rows + (carry ? addr[1] : addr[0]) + (rj & (EPT - 1)) * (NCOL * 4)) +
           (carry ? turn[1] : turn[0]);
  };
  float s = 0.f;
  constexpr int CH = NR < 8 ? NR : 8;
#pragma unroll
  for (int r0 = 0; r0 < NR; r0 += CH) {
    float v[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) v[j] = fetch(r0 + j);
#pragma unroll
    for (int j = 0; j < CH; ++j) s += pow_abs<PMODE>(u[r0 + j] - v[j], p, p_int);
    __builtin_amdgcn_sched_barrier(0);
  }
  return wave_sum_uniform(s, lane & 63);
}

// ---------------------------------------------------------------------------------------------
// The fast form again, with the sorted target fetched four rows at a time (n == 64*EPT, one wave, all EPT registers).
//
// Layout ("grouped rows"): rows 4g .. 4g + 3 of column col lie side by side, 16 bytes at byte offset g * 1024 + col * 16
// of the same 256 EPT bytes (16-byte aligned: the target row starts 128 EPT bytes into a 16-byte-aligned block, and a
// wave's block is 384 EPT bytes).  Consecutive window positions of a lane are consecutive rows of one column until the row
// index wraps, and a group aligned to 4 never straddles the wrap (4 divides EPT): with a = kl mod 4 and q0 = kl div 4 the
// window rows kl, kl + 1, ... lie in the aligned groups G = q0 + t, t = 0, 1, ...; group G is group G mod (EPT / 4) of the
// column with carry G div (EPT / 4).  One select of the address, one of the turn and one add of the wave-uniform group
// offset then serve four values from one ds_read_b128, where shift_costs3_full pays them per value; the turn is added to
// every value as before.  Window value j is element (a + j) mod 4 of group (a + j) div 4: a is wave-uniform and a
// template parameter of the unrolled body, which the caller picks with a scalar branch -- four copies of each body.
// The values, the order in which every per-lane sum takes them and the reductions are those of shift_costs3_full /
// shift_cost1_full: every result has the same bits.
// ---------------------------------------------------------------------------------------------
constexpr int kGroupRows = 4;
// Is the sorted target of ssw_forward_kernel<EPT, 1, PMODE, FULL> laid out in grouped rows?  Asked by the kernel that
// writes it and by the solve that reads it.  The headline class only: the general-power kernel (PMODE 0) spends its time
// in the powers, not in the fetch, and four copies of its loop bodies would be four times the kernel's largest block; the
// smaller full one-wave classes are not what the dispatch rule selects (dispatch.hpp: two waves per slice there).
constexpr bool shift_fetch_grouped(int ept, int waves, int pmode, bool full) {
  return full && waves == 1 && ept == 32 && pmode == 2;
}

// lane's sorted keys (rows 0 .. EPT - 1 of column `lane`) into the grouped layout: EPT / 4 ds_write_b128
template <int EPT>
__device__ __forceinline__ void write_grouped_rows(float* vbuf, int lane, const float (&key)[EPT]) {
  char* col = reinterpret_cast<char*>(vbuf) + lane * (4 * kGroupRows);
#pragma unroll
  for (int g = 0; g < EPT / kGroupRows; ++g)
    *reinterpret_cast<float4*>(col + g * (256 * kGroupRows)) =
        make_float4(key[4 * g], key[4 * g + 1], key[4 * g + 2], key[4 * g + 3]);
}

// one group: the (address, turn) pair by value, as in inc_fetch
__device__ __forceinline__ void read_group(const char* at, float turn, float (&out)[kGroupRows]) {
  const float4 v = *reinterpret_cast<const float4*>(at);
  out[0] = v.x + turn; out[1] = v.y + turn; out[2] = v.z + turn; out[3] = v.w + turn;
}

// the three per-lane sums of shift_costs3_full for a window that starts at element A of group q0 of the column with
// carry 0 (a0, t0); a1, t1 / a2, t2: the columns with carry 1 / 2
template <int EPT, int PMODE, int A>
__device__ __forceinline__ void shift_sums3_grouped(const float (&u)[EPT], const char* rows, int a0, int a1, int a2,
                                                    float t0, float t1, float t2, int q0, float p, int p_int,
                                                    float& sm, float& s0, float& sp) {
  constexpr int GW = kGroupRows;
  constexpr int GPC = EPT / GW;                                 // groups per column
  constexpr int NG = (A + EPT + 1) / GW + 1;                    // groups that hold the EPT + 2 window values: 9 or 10
  float grp[NG][GW];
  auto load = [&](int t) {                                      // t compile-time after unrolling
    const int G = q0 + t;                                       // scalar; t < GPC: carry 0 or 1, else 1 or 2
    const bool carry = (t < GPC) ? (G >= GPC) : (G >= 2 * GPC);
    const int a = (t < GPC) ? (carry ? a1 : a0) : (carry ? a2 : a1);
    const float tn = (t < GPC) ? (carry ? t1 : t0) : (carry ? t2 : t1);
    read_group(rows + a + (G & (GPC - 1)) * (256 * GW), tn, grp[t]);
  };
  // group t is first needed by window value max(0, 4 t - A); a chunk of eight rows fetches the groups that begin among
  // its eight new window values
#pragma unroll
  for (int t = 0; t < NG; ++t) if (GW * t - A <= 1) load(t);
  sm = 0.f; s0 = 0.f; sp = 0.f;
  float prev = grp[A / GW][A % GW], cur = grp[(A + 1) / GW][(A + 1) % GW];
  constexpr int CH = 8;
#pragma unroll
  for (int r0 = 0; r0 < EPT; r0 += CH) {
#pragma unroll
    for (int t = 0; t < NG; ++t) if (GW * t - A >= r0 + 2 && GW * t - A <= r0 + CH + 1) load(t);
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const float nxt = grp[(A + r0 + j + 2) / GW][(A + r0 + j + 2) % GW];
      sm += pow_abs<PMODE>(u[r0 + j] - prev, p, p_int);
      s0 += pow_abs<PMODE>(u[r0 + j] - cur, p, p_int);
      sp += pow_abs<PMODE>(u[r0 + j] - nxt, p, p_int);
      prev = cur;
      cur = nxt;
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// shift_costs3_full on grouped rows
template <int EPT, int PMODE>
__device__ __forceinline__ void shift_costs3_grouped(const float (&u)[EPT], const float* vbuf, int lane, int k, float p,
                                                     int p_int, float& cm, float& c0, float& cp) {
  static_assert(EPT % 8 == 0, "whole groups, chunks of eight rows");
  constexpr int LOG = __builtin_ctz(EPT);
  const int base = k - 1;
  const int kl = base & (EPT - 1);
  const int kh = base >> LOG;                                   // floor division (arithmetic shift)
  int addr[3];
  float turn[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int col = lane + kh + c;                              // unwrapped lane index of the atom
    addr[c] = (col & 63) << 4;                                  // byte offset of the column inside a row of groups
    turn[c] = (float)(col >> 6);                                // whole turns around the circle
  }
  const char* rows = reinterpret_cast<const char*>(vbuf);
  const int a = kl & 3, q0 = kl >> 2;                           // scalar
  float sm, s0, sp;
  if (a == 0) shift_sums3_grouped<EPT, PMODE, 0>(u, rows, addr[0], addr[1], addr[2], turn[0], turn[1], turn[2], q0, p, p_int, sm, s0, sp);
  else if (a == 1) shift_sums3_grouped<EPT, PMODE, 1>(u, rows, addr[0], addr[1], addr[2], turn[0], turn[1], turn[2], q0, p, p_int, sm, s0, sp);
  else if (a == 2) shift_sums3_grouped<EPT, PMODE, 2>(u, rows, addr[0], addr[1], addr[2], turn[0], turn[1], turn[2], q0, p, p_int, sm, s0, sp);
  else shift_sums3_grouped<EPT, PMODE, 3>(u, rows, addr[0], addr[1], addr[2], turn[0], turn[1], turn[2], q0, p, p_int, sm, s0, sp);
  cm = wave_sum_uniform(sm, lane & 63);
  c0 = wave_sum_uniform(s0, lane & 63);
  cp = wave_sum_uniform(sp, lane & 63);
}

// the per-lane sum of shift_cost1_full for a window of EPT values that starts at element A of group q0 (carry 0 or 1)
template <int EPT, int PMODE, int A>
__device__ __forceinline__ float shift_sum1_grouped(const float (&u)[EPT], const char* rows, int a0, int a1, float t0,
                                                    float t1, int q0, float p, int p_int) {
  constexpr int GW = kGroupRows;
  constexpr int GPC = EPT / GW;
  constexpr int NG = (A + EPT - 1) / GW + 1;                    // 8 or 9
  float grp[NG][GW];
  auto load = [&](int t) {                                      // t compile-time after unrolling
    const int G = q0 + t;                                       // scalar, below 2 GPC
    const bool carry = G >= GPC;
    read_group(rows + (carry ? a1 : a0) + (G & (GPC - 1)) * (256 * GW), carry ? t1 : t0, grp[t]);
  };
  float s = 0.f;
  constexpr int CH = 8;
#pragma unroll
  for (int r0 = 0; r0 < EPT; r0 += CH) {
#pragma unroll
    for (int t = 0; t < NG; ++t) {
      const int first = GW * t - A < 0 ? 0 : GW * t - A;        // the window value that needs group t first
      if (first >= r0 && first < r0 + CH) load(t);
    }
#pragma unroll
    for (int j = 0; j < CH; ++j) s += pow_abs<PMODE>(u[r0 + j] - grp[(A + r0 + j) / GW][(A + r0 + j) % GW], p, p_int);
    __builtin_amdgcn_sched_barrier(0);
  }
  return s;
}

// shift_cost1_full on grouped rows
template <int EPT, int PMODE>
__device__ __forceinline__ float shift_cost1_grouped(const float (&u)[EPT], const float* vbuf, int lane, int kk, float p,
                                                     int p_int) {
  constexpr int LOG = __builtin_ctz(EPT);
  const int kl = kk & (EPT - 1);
  const int kh = kk >> LOG;
  int addr[2];
  float turn[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int col = lane + kh + c;
    addr[c] = (col & 63) << 4;
    turn[c] = (float)(col >> 6);
  }
  const char* rows = reinterpret_cast<const char*>(vbuf);
  const int a = kl & 3, q0 = kl >> 2;                           // scalar
  float s;
  if (a == 0) s = shift_sum1_grouped<EPT, PMODE, 0>(u, rows, addr[0], addr[1], turn[0], turn[1], q0, p, p_int);
  else if (a == 1) s = shift_sum1_grouped<EPT, PMODE, 1>(u, rows, addr[0], addr[1], turn[0], turn[1], q0, p, p_int);
  else if (a == 2) s = shift_sum1_grouped<EPT, PMODE, 2>(u, rows, addr[0], addr[1], turn[0], turn[1], q0, p, p_int);
  else s = shift_sum1_grouped<EPT, PMODE, 3>(u, rows, addr[0], addr[1], turn[0], turn[1], q0, p, p_int);
  return wave_sum_uniform(s, lane & 63);
}

// Minimise the convex sequence c(k), |k| <= n (theta in [-1, 1], the reference's bracket :174-177).
// Returns k*, writes c(k*) (sum form).
// REUSE: evaluate only the new shift after a unit step (the loss kernel; the training kernels keep three per step).
// GROUPED: the caller wrote the target in grouped rows (shift_fetch_grouped), not in plain ones.
template <int EPT, int PMODE, bool FULL = false, bool REUSE = false, bool GROUPED = false>
__device__ __forceinline__ int solve_shift(const float (&u)[EPT], const float* vbuf, int lane, int n,
                                           float sum_u, float sum_v, float p, int p_int, float& best) {
  int lo = -n, hi = n;
  float guess = rintf(sum_u - sum_v);
  guess = fminf(fmaxf(guess, (float)lo), (float)hi);
  int k = __builtin_amdgcn_readfirstlane((int)guess);         // k lives in an SGPR from here on
  bool lo_tight = false, hi_tight = false;
  int step = 1;
  float cm = 0.f, c0 = 0.f, cp = 0.f;
  // a unit step (the first gallop step, or a bisection that lands next door) already knows two of its three costs:
  // c(k -/+ 1) and c(k) are the c(k) and c(k +/- 1) of the evaluation before, bit for bit (shift_cost1).  The
  // incremental evaluation of the small partial classes (shift_costs3_inc) has no one-shift form and always takes three.
  constexpr bool kReuse = REUSE && (FULL || !(SHW_SOLVE_INC && EPT <= 16));
  int kprev = k + 2;                   // no unit step before the first evaluation
  // every iteration removes k from [lo, hi]; galloping doubles, bisection halves: <= ~2 log2(2n)+2
  // iterations.  The hard cap only guards against non-finite input (comparisons all false -> exit).
  for (int it = 0; it < 64; ++it) {
    int ln = lane;                       // opaque copy: no lane-derived constants held across iterations
    asm volatile("" : "+v"(ln));
    const int d = k - kprev;             // wave-uniform
    if (kReuse && (d == 1 || d == -1)) {
      float c;
      if constexpr (FULL && GROUPED) c = shift_cost1_grouped<EPT, PMODE>(u, vbuf, ln, k + d, p, p_int);
      else if constexpr (FULL) c = shift_cost1_full<EPT, PMODE>(u, vbuf, ln, k + d, p, p_int);
      else c = shift_cost1<EPT, PMODE>(u, vbuf, ln, n, k + d, p, p_int);
      if (d == 1) { cm = c0; c0 = cp; cp = c; }
      else { cp = c0; c0 = cm; cm = c; }
    } else if constexpr (FULL && GROUPED) {
      shift_costs3_grouped<EPT, PMODE>(u, vbuf, ln, k, p, p_int, cm, c0, cp);
    } else if constexpr (FULL) {
      shift_costs3_full<EPT, PMODE>(u, vbuf, ln, k, p, p_int, cm, c0, cp);
    } else if constexpr (SHW_SOLVE_INC && EPT <= 16) {
      shift_costs3_inc<EPT, PMODE>(u, vbuf, ln, n, k, p, p_int, cm, c0, cp);
    } else {
      shift_costs3<EPT, PMODE>(u, vbuf, ln, n, k, p, p_int, cm, c0, cp);   // (diagnostic one-wave kernels of the big classes)
    }
    kprev = k;
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
    k = __builtin_amdgcn_readfirstlane(k);
  }
  best = c0;
  return k;
}

// ---------------------------------------------------------------------------------------------
// Any n (not only n == 64*EPT): the sorted target as PRE-ROTATED, EXTENDED rows.
//
// The generic evaluation (shift_costs3 / target_unrolled) pays ~15 VALU per fetched target atom for the wrap-around
// arithmetic (two conditional turns, a multiply, the slot computation).  Instead the target is written to LDS already
// rotated to the first guess kc of the shift and with the turns added:
//     ext[E] = v_ext(E - M + kc),   E in [0, n + 2M),   v_ext(q) = v[q mod n] + floor(q / n),   M = EPT,
// laid out [E mod EPT][E div EPT] with 66 columns per row (64 lanes + the halo).  A shift k = kc + d with |d| < M
// then reads ext[e + d + delta + M] for source atom e: no wrap, no turn, every address = lane*4 + a wave-uniform
// offset -- 1 VALU per fetch.  The search seldom leaves |d| < M (the first guess is exact for evenly spaced
// targets and galloping starts with steps 1, 2, 4, ...); when it does the rows are rewritten around the new k.
// ---------------------------------------------------------------------------------------------
// NCOL > 64 (cooperative kernel): NCOL lanes of NCOL/64 waves hold the slice, `lane` is the lane number within the
// slice and the writers synchronise with workgroup barriers.
template <int EPT, int NCOL = 64>
struct ExtRows {
  static constexpr int M = EPT;                 // half width of the halo = reach of the shift without a rewrite
  static constexpr int RS = NCOL + 2;           // columns per row: (NCOL*EPT + 2M) / EPT
  static constexpr int FLOATS = EPT * RS;
  static constexpr int TRASH = ((EPT - 1) * RS + NCOL + 1) * 4;   // byte offset of the last slot: never a valid E for n < NCOL*EPT
};

// v[r] = sorted target at position lane*EPT + r (anything at positions >= n).  n > M required (size classes give n > 32*EPT).
template <int EPT, int NCOL = 64>
__device__ __forceinline__ void ext_rows_write(const float (&v)[EPT], float* ext, int lane, int n, int kc) {
  typedef ExtRows<EPT, NCOL> X;
  // c1 = (M - kc) mod n and the turn s it absorbs: ext[p + c1] = v[p] - s, or, past the end, ext[p + c1 - n] = v[p] - s - 1
  const int t = X::M - kc;                                       // in [M - n, M + n]
  const int s = t < 0 ? -1 : (t >= n ? 1 : 0);
  const int c1 = t - s * n;                                      // in [0, n)
  const int c2 = c1 - n;                                         // in [-n, 0)
  const int c1h = ediv<EPT>(c1), c1l = emod<EPT>(c1);
  const int c2h = ediv<EPT>(c2), c2l = emod<EPT>(c2);            // floor division
  const float vn = (float)(-s), vw = (float)(-s - 1);
  char* bytes = reinterpret_cast<char*>(ext);
  const int lane4 = lane << 2;
  const int first_wrapped = n - c1;                              // positions p >= this wrap
#pragma unroll
  for (int r = 0; r < EPT; ++r) {
    const int a1 = r + c1l, a2 = r + c2l;                        // scalars
    const int off_n = ((emod<EPT>(a1) * X::RS) + c1h + ediv<EPT>(a1)) << 2;
    const int off_w = ((emod<EPT>(a2) * X::RS) + c2h + ediv<EPT>(a2)) << 2;
    const int pos = lane * EPT + r;
    const bool wrap = pos >= first_wrapped;
    int off = wrap ? off_w : off_n;
    off = pos < n ? off + lane4 : X::TRASH;
    *reinterpret_cast<float*>(bytes + off) = v[r] + (wrap ? vw : vn);
  }
  if constexpr (NCOL > 64) __syncthreads(); else __builtin_amdgcn_wave_barrier();
  // halo: ext[n + l] = ext[l] + 1 for l < 2M (one entry per lane; 2M <= 64)
  {
    const int src = lane, dst = n + lane;
    const int so = ((emod<EPT>(src) * X::RS) + ediv<EPT>(src)) << 2;
    const int d_o = ((emod<EPT>(dst) * X::RS) + ediv<EPT>(dst)) << 2;
    const float x = *reinterpret_cast<const float*>(bytes + so);
    *reinterpret_cast<float*>(bytes + (lane < 2 * X::M ? d_o : X::TRASH)) = x + 1.f;
  }
  if constexpr (NCOL > 64) __syncthreads(); else __builtin_amdgcn_wave_barrier();
}

// c(k-1), c(k), c(k+1) for k = kc + d, |d| < M, on registers [r_base, r_base + NR) of every lane (u holds those NR
// source atoms; atoms at positions >= n are masked out).  Sums over the wave, valid in every lane.
template <int EPT, int PMODE, int NR = EPT, int NCOL = 64>
__device__ __forceinline__ void shift_costs3_ext(const float (&u)[NR], const float* ext, int lane, int n, int d,
                                                 float p, int p_int, float& cm, float& c0, float& cp, int r_base = 0) {
  typedef ExtRows<EPT, NCOL> X;
  const int base = d - 1 + X::M + r_base;                        // >= 0, wave-uniform
  const int bl = emod<EPT>(base), bh = ediv<EPT>(base);
  const char* rows = reinterpret_cast<const char*>(ext) + (lane << 2);
  auto fetch = [&](int j) -> float {                             // j compile-time after unrolling
    const int a = bl + j;                                        // scalar
    const int off = ((emod<EPT>(a) * X::RS) + bh + ediv<EPT>(a)) << 2;
    return *reinterpret_cast<const float*>(rows + off);
  };
  const int live_regs = n - lane * EPT - r_base;                 // registers j < live_regs hold real atoms
  float sm = 0.f, s0 = 0.f, sp = 0.f;
  float prev = fetch(0), cur = fetch(1);
  constexpr int CH = chunk_of(NR);
#pragma unroll
  for (int r0 = 0; r0 < NR; r0 += CH) {
    float nxt[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) nxt[j] = fetch(r0 + j + 2);
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const float a = pow_abs<PMODE>(u[r0 + j] - prev, p, p_int);
      const float b = pow_abs<PMODE>(u[r0 + j] - cur, p, p_int);
      const float c = pow_abs<PMODE>(u[r0 + j] - nxt[j], p, p_int);
#if SHW_MASK_BY_EXEC
      // pads add nothing: a branch the compiler must keep (the empty asm), i.e. one v_cmp and an exec mask around three
      // full-rate adds -- as selects the three accumulations cost a quarter-rate v_cndmask each (op rates)
      if ((r0 + j) < live_regs) {
        asm volatile("" : "+v"(sm), "+v"(s0), "+v"(sp));
        sm += a; s0 += b; sp += c;
      }
#else
      const bool live = (r0 + j) < live_regs;
      sm += live ? a : 0.f;
      s0 += live ? b : 0.f;
      sp += live ? c : 0.f;
#endif
      prev = cur;
      cur = nxt[j];
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  cm = wave_sum_uniform(sm, lane & 63);
  c0 = wave_sum_uniform(s0, lane & 63);
  cp = wave_sum_uniform(sp, lane & 63);
}

// solve_shift on extended rows (one wave owns the slice).  v = the sorted target in registers (kept for rewrites).
template <int EPT, int PMODE>
__device__ __forceinline__ int solve_shift_ext(const float (&u)[EPT], const float (&v)[EPT], float* ext, int lane, int n,
                                               float sum_u, float sum_v, float p, int p_int, float& best) {
  typedef ExtRows<EPT> X;
  int lo = -n, hi = n;
  float guess = rintf(sum_u - sum_v);
  guess = fminf(fmaxf(guess, (float)lo), (float)hi);
  int k = __builtin_amdgcn_readfirstlane((int)guess);
  int kc = k;
  ext_rows_write<EPT>(v, ext, lane, n, kc);
  bool lo_tight = false, hi_tight = false;
  int step = 1;
  float cm, c0, cp;
  for (int it = 0; it < 64; ++it) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
    if (k - kc >= X::M || kc - k >= X::M) {                      // wave-uniform: re-centre the rows on k
      kc = k;
      ext_rows_write<EPT>(v, ext, ln, n, kc);
    }
    shift_costs3_ext<EPT, PMODE>(u, ext, ln, n, k - kc, p, p_int, cm, c0, cp);
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
    k = __builtin_amdgcn_readfirstlane(k);
  }
  best = c0;
  return k;
}

// Project the cloud onto the slice's circle: lane owns points r*64 + lane (coalesced 12-byte
// records).  Padding keys are +inf so that they sort behind every real coordinate.
// CHAINED: make the addresses of a chunk depend (through an empty asm) on the last coordinate of the chunk
// before it.  Needed where the loads are not inside a loop: the compiler otherwise issues all 3*EPT loads up
// front and the raw points take 96 registers (shw_ssw_p1_merge.hip).
// NCOL: lanes that share the cloud (64 for one wave; 64*W when W waves of a workgroup own a slice together, `lane`
// then being the index among those lanes): lane owns points r*NCOL + lane.
// FOLD: how the masked classes take coordinate-row mode, see below.
template <int EPT, bool FULL = false, bool CHAINED = false, int NCOL = kWave, bool FOLD = false>
__device__ __forceinline__ float load_coords(const float* __restrict__ X, int count, int lane,
                                             const float (&U)[6], float (&key)[EPT], int live_count = -1) {
  // `count` bounds the addresses (clamp), `live_count` (default: count) says how many of the 64*EPT slots are
  // real atoms; they differ only for the trailing chunks of the multi-wave kernel
  if (live_count < 0) live_count = count;
  float acc = 0.f;
  // coordinate-row mode (shw_circle_ot): X holds circle coordinates, one float per atom (U[0] is NaN then): a branch
  // -- or, FOLD, part of the one code path (record stride 1 or 3 and a final select).  As a branch it left both forms'
  // state live at the join in the two-wave training kernel's masked classes: 14 -> 39 spilled registers, N=2000
  // training 0.62 -> 0.80 ms; folded it costs 2 + 1 VALU per point.  (The loss kernels spill less with the branch.)
  const bool rows = U[0] != U[0];
  constexpr bool kFold = FOLD && !FULL;
  constexpr bool kScalarBase = FULL;               // how the point loads are addressed, see below
  if constexpr (!kFold) {
    if (rows) {
#pragma unroll
      for (int r = 0; r < EPT; ++r) {
        const int i = r * NCOL + lane;
        // (addressing: see the point loads below)
        const float c = kScalarBase ? (X + r * NCOL)[(size_t)(unsigned)lane] : X[FULL ? i : min(i, count - 1)];
        const bool live = FULL || (i < live_count);
        acc += live ? c : 0.f;
        key[r] = live ? c : __builtin_inff();
      }
      return acc;
    }
  }
  const int wide = (kFold && rows) ? 0 : -1;       // all ones: 12-byte records
  const int o1 = (kFold && rows) ? 0 : 1, o2 = (kFold && rows) ? 0 : 2;
  constexpr int CH = chunk_of(EPT);                // 8 points (24 loads) in flight per lane (4 or 5 for the odd classes)
#pragma unroll
  for (int r0 = 0; r0 < EPT; r0 += CH) {
    if constexpr (!FULL && !kFold) {
      // lane owns points r*NCOL + lane: from row ceil(live_count / NCOL) on EVERY lane's point is a pad -- a wave-uniform
      // test per chunk skips their loads, projections and arctangents (N=1200 in the 2048 class: a quarter of them;
      // loss 0.290 -> 0.263 ms).  Not in the indexed sort's loader (FOLD): there the branches cost the nearly full
      // classes more than they save the others (N=2000 training 0.654 -> 0.681 ms).
      if (r0 * NCOL >= live_count) {
#pragma unroll
        for (int j = 0; j < CH; ++j) key[r0 + j] = __builtin_inff();
        continue;
      }
    }
    float px[CH], py[CH], pz[CH];
    if constexpr (CHAINED) {
      if (r0 > 0) asm volatile("" : "+v"(lane) : "v"(key[r0 > 0 ? r0 - 1 : 0]));
    }
    // lane owns points r*NCOL + lane: when every point of the chunk's rows exists (uniform over the wave) the chunk is
    // the code of a full class -- no clamped addresses, no masks; only the one mixed chunk of a cloud pays for them
    const bool whole = FULL || (!is_pow2(EPT) && (r0 + CH) * NCOL <= (live_count < count ? live_count : count));   // (classes: bin_sort.hpp)
    // Addresses of a full class: a wave-uniform 64-bit base (the cloud plus the row) and ONE unsigned 32-bit offset per
    // lane, widened before the +1 / +2 so that these go into the load's immediate field and the three loads of a record
    // still merge into a dwordx3.  A signed index costs an add, a sign extension and a 64-bit shift-add per record
    // instead.  A cloud has at most 8192 points: 3 * 4 * 8192 bytes, far below 2^32.
    // (The classes with pads keep the signed index, in the clamped path too: given unsigned offsets together with the
    //  byte-offset bin map, the two-wave loss kernel lost 4..8 % at N = 1200 / 2000 -- see bin_sort.hpp; which of the two
    //  cost it was not separated -- and the 8192-point training kernel began to spill, 0 -> 36 registers.)
    if (whole) {
      const size_t o3 = (size_t)(3u * (unsigned)lane);
      (void)o3;
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        if constexpr (kFold || !kScalarBase) {
          const int i = (r0 + j) * NCOL + lane;
          const int i3 = kFold ? i + ((i & wide) << 1) : 3 * i;
          px[j] = X[i3]; py[j] = X[i3 + (kFold ? o1 : 1)]; pz[j] = X[i3 + (kFold ? o2 : 2)];
        } else {
          const float* row = X + 3 * (r0 + j) * NCOL;
          px[j] = row[o3]; py[j] = row[o3 + 1]; pz[j] = row[o3 + 2];
        }
      }
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const float a = fmaf(pz[j], U[4], fmaf(py[j], U[2], fmaf(px[j], U[0], 0.f)));
        const float b = fmaf(pz[j], U[5], fmaf(py[j], U[3], fmaf(px[j], U[1], 0.f)));
        float c = circle_coord(a, b);
        if constexpr (kFold) c = rows ? px[j] : c;
        acc += c;
        key[r0 + j] = c;
      }
    } else {
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int raw = (r0 + j) * NCOL + lane;
        const int i = min(raw, count - 1);                        // clamp: branch-free, always in bounds
        const int i3 = kFold ? i + ((i & wide) << 1) : 3 * i;     // 3 i, or i for rows of coordinates
        px[j] = X[i3]; py[j] = X[i3 + (kFold ? o1 : 1)]; pz[j] = X[i3 + (kFold ? o2 : 2)];
      }
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int i = (r0 + j) * NCOL + lane;
        // fma(x, u, +0): a sum that starts from +0 like the reference's matmul accumulator (:270), so that an
        // all-zero point projects to (+0, +0) -- never -0 -- and lands on coordinate 0 (G4 fixture)
        const float a = fmaf(pz[j], U[4], fmaf(py[j], U[2], fmaf(px[j], U[0], 0.f)));
        const float b = fmaf(pz[j], U[5], fmaf(py[j], U[3], fmaf(px[j], U[1], 0.f)));
        float c = circle_coord(a, b);
        if constexpr (kFold) c = rows ? px[j] : c;
        const bool live = i < live_count;
        acc += live ? c : 0.f;
        key[r0 + j] = live ? c : __builtin_inff();
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  return acc;
}

// ---------------------------------------------------------------------------------------------
// Rolling loader of a full class (the 2048-point one-wave loss kernel): the cloud's rows go through the projection in
// sub-chunks of SUB rows, and the loads of sub-chunk c + 1 are issued before the arithmetic of sub-chunk c, so the wave
// waits for a partial count (s_waitcnt vmcnt(SUB)) with the next records already on their way, where load_coords drains
// the queue once per chunk.  The FIRST sub-chunk is issued by the caller (issue_points), as early as it knows the cloud:
// the source's beside the frame, the target's before the source's sort.  The addresses are those of load_coords' full
// path -- rows r0 .. r0 + SUB - 1 of the cloud X, each once, r0 < EPT -- and the coordinates, the order of `acc` and the
// keys are its values bit for bit.  Rows of coordinates (U[0] NaN) take load_coords' own branch: nothing is issued ahead.
// ---------------------------------------------------------------------------------------------
template <int SUB>
struct PointChunk {
  float x[SUB], y[SUB], z[SUB];
};

// issue the loads of rows [r0, r0 + SUB) of a full cloud: lane owns points r * 64 + lane (scalar base, one unsigned
// offset per lane, the row in the immediate field: see load_coords)
template <int SUB>
__device__ __forceinline__ void issue_points(const float* __restrict__ X, int lane, int r0, PointChunk<SUB>& P) {
  const size_t o3 = (size_t)(3u * (unsigned)lane);
#pragma unroll
  for (int j = 0; j < SUB; ++j) {
    const float* row = X + 3 * (r0 + j) * kWave;
    P.x[j] = row[o3]; P.y[j] = row[o3 + 1]; P.z[j] = row[o3 + 2];
  }
}

template <int EPT, int SUB>
__device__ __forceinline__ float load_coords_rolling(const float* __restrict__ X, int lane, const float (&U)[6],
                                                     float (&key)[EPT], const PointChunk<SUB>& first) {
  static_assert(EPT % SUB == 0, "whole sub-chunks");
  if (U[0] != U[0]) return load_coords<EPT, true>(X, EPT * kWave, lane, U, key);
  float acc = 0.f;
  PointChunk<SUB> cur = first;
#pragma unroll
  for (int r0 = 0; r0 < EPT; r0 += SUB) {
    PointChunk<SUB> nxt;
    if (r0 + SUB < EPT) {                            // never past the cloud's last row
      issue_points<SUB>(X, lane, r0 + SUB, nxt);
      __builtin_amdgcn_sched_barrier(0);             // the loads stay in front of the arithmetic
    }
#pragma unroll
    for (int j = 0; j < SUB; ++j) {
      const float a = fmaf(cur.z[j], U[4], fmaf(cur.y[j], U[2], fmaf(cur.x[j], U[0], 0.f)));
      const float b = fmaf(cur.z[j], U[5], fmaf(cur.y[j], U[3], fmaf(cur.x[j], U[1], 0.f)));
      const float c = circle_coord(a, b);
      acc += c;
      key[r0 + j] = c;
    }
    __builtin_amdgcn_sched_barrier(0);
    if (r0 + SUB < EPT) cur = nxt;
  }
  return acc;
}


// ---------------------------------------------------------------------------------------------
// sort WITH the permutation (training and weighted kernels): packed 32-bit keys, see shw_ssw_grad.hip
// ---------------------------------------------------------------------------------------------
template <int EPT>
struct Packing {
  static constexpr int IDX_BITS = log2_ceil_c(EPT * kWave);
  static constexpr int QBITS = 32 - IDX_BITS;
  static constexpr unsigned IDX_MASK = (1u << IDX_BITS) - 1u;
  static __device__ __forceinline__ unsigned pack(float coord, int idx, bool live) {
    // coord in [0, 1]; 2^QBITS * coord is exact in fp32 for QBITS <= 26 and fits 32 bits
    const float scaled = coord * (float)(1u << (QBITS > 26 ? 26 : QBITS));
    unsigned q = (unsigned)scaled;
    if constexpr (QBITS > 26) q <<= (QBITS - 26);
    const unsigned qmax = (QBITS >= 32) ? 0xffffffffu : ((1u << QBITS) - 1u);
    q = q < qmax ? q : qmax;
    return live ? ((q << IDX_BITS) | (unsigned)idx) : 0xffffffffu;
  }
};

// (value, index) pair order: ascending value, ties by ascending index
__device__ __forceinline__ bool pair_after(float va, int ia, float vb, int ib) {
  return (va > vb) || (va == vb && ia > ib);
}

// Put a nearly sorted (val, idx) sequence -- sorted position lane*EPT + r -- into exact stable order.
// One round = exchange of pairs (2j, 2j+1) then (2j+1, 2j+2); rounds repeat until a round is clean.
template <int EPT>
__device__ __forceinline__ void exact_order_fixup(float (&val)[EPT], int (&idx)[EPT], int lane,
                                                  int max_rounds = EPT * kWave) {
  for (int round = 0; round < max_rounds; ++round) {        // bound: odd-even transposition sorts in n rounds
    bool any = false;
    auto exch = [&](float& va, int& ia, float& vb, int& ib) {
      const bool sw = pair_after(va, ia, vb, ib);
      const float tv = va; const int ti = ia;
      va = sw ? vb : va; ia = sw ? ib : ia;
      vb = sw ? tv : vb; ib = sw ? ti : ib;
      any |= sw;
    };
#pragma unroll
    for (int r = 0; r + 1 < EPT; r += 2) exch(val[r], idx[r], val[r + 1], idx[r + 1]);
#pragma unroll
    for (int r = 1; r + 1 < EPT; r += 2) exch(val[r], idx[r], val[r + 1], idx[r + 1]);
    {  // boundary pair: this lane's last atom against the next lane's first
      const int up = min(lane + 1, 63) << 2, dn = max(lane - 1, 0) << 2;
      const float nv = as_f(__builtin_amdgcn_ds_bpermute(up, as_i(val[0])));
      const int ni = __builtin_amdgcn_ds_bpermute(up, idx[0]);
      const float pv = as_f(__builtin_amdgcn_ds_bpermute(dn, as_i(val[EPT - 1])));
      const int pi = __builtin_amdgcn_ds_bpermute(dn, idx[EPT - 1]);
      const bool sw_up = (lane < 63) && pair_after(val[EPT - 1], idx[EPT - 1], nv, ni);
      const bool sw_dn = (lane > 0) && pair_after(pv, pi, val[0], idx[0]);
      if constexpr (EPT == 1) {
        // a lane's single atom can be wanted by both neighbours: alternate even / odd boundaries
        const bool even_phase = (round & 1) == 0;
        const bool do_up = sw_up && (((lane & 1) == 0) == even_phase);
        const bool do_dn = sw_dn && (((lane & 1) == 1) == even_phase);
        val[0] = do_up ? nv : (do_dn ? pv : val[0]);
        idx[0] = do_up ? ni : (do_dn ? pi : idx[0]);
        any |= sw_up || sw_dn;
      } else {
        val[EPT - 1] = sw_up ? nv : val[EPT - 1]; idx[EPT - 1] = sw_up ? ni : idx[EPT - 1];
        val[0] = sw_dn ? pv : val[0]; idx[0] = sw_dn ? pi : idx[0];
        any |= sw_up || sw_dn;
      }
    }
    if (__builtin_amdgcn_readfirstlane((int)(__ballot(any) != 0ull)) == 0) break;
  }
}

// From the sorted packed words to (exact coordinate, original index) in exact stable order: gather the fp32
// coordinates by index from `orig` (coordinates by ORIGINAL index, pads +inf) and repair the order of atoms whose
// quantised coordinates collide.  Shared by the network sort (sorted_with_indices) and the distribution sort
// (bin_sort_idx.hpp).
// FULL: count == 64*EPT (no pads): the pad tests fold away.
template <int EPT, bool FULL = false>
__device__ __forceinline__ void unpack_sorted_words(const unsigned (&pk)[EPT], const float* orig, int count, int lane,
                                                    float (&val)[EPT], int (&idx)[EPT]) {
  typedef Packing<EPT> PK;
  // A pad is recognised by its index field (all ones, >= count whenever pads exist), NOT by the key value:
  // the real atom with index 64*EPT-1 and a coordinate in the top quantisation cell packs to the same word
  // 0xffffffff when the row is full.
  // Equal quantised coordinate on adjacent atoms?  (`chain`: on three in a row -- only then can one repair round be
  // not enough.)
  bool collide = false, chain = false;
  bool prev_eq;
  {
    const unsigned nxt = (unsigned)__builtin_amdgcn_ds_bpermute(min(lane + 1, 63) << 2, (int)pk[0]);
    const unsigned prv = (unsigned)__builtin_amdgcn_ds_bpermute(max(lane - 1, 0) << 2, (int)pk[EPT - 1]);
    collide = (lane < 63) && (((pk[EPT - 1] ^ nxt) >> PK::IDX_BITS) == 0) &&
              (FULL || (int)(pk[EPT - 1] & PK::IDX_MASK) < count);
    prev_eq = (lane > 0) && (((pk[0] ^ prv) >> PK::IDX_BITS) == 0) && (FULL || (int)(pk[0] & PK::IDX_MASK) < count);
  }
  const bool next_eq = collide;                           // (last atom of this lane, first atom of the next)
#pragma unroll
  for (int r = 1; r < EPT; ++r) {
    const bool eq = (((pk[r] ^ pk[r - 1]) >> PK::IDX_BITS) == 0) && (FULL || (int)(pk[r] & PK::IDX_MASK) < count);
    chain |= eq && prev_eq;
    collide |= eq;
    prev_eq = eq;
  }
  chain |= prev_eq && next_eq;                            // ... (EPT-2, EPT-1, first of the next lane)
  if constexpr (EPT == 1) chain |= collide;               // one atom per lane: every collision touches a lane boundary
  // (the packed words are dead from here on: index and gathered coordinate take their registers)
#pragma unroll
  for (int r = 0; r < EPT; ++r) {
    idx[r] = (int)(pk[r] & PK::IDX_MASK);
    val[r] = (!FULL && idx[r] >= count) ? __builtin_inff() : orig[FULL ? idx[r] : min(idx[r], count - 1)];
  }
#ifndef SHW_ABL_NO_EXACTFIX
  if (__builtin_amdgcn_readfirstlane((int)(__ballot(collide) != 0ull)) != 0) {
    // one round repairs every colliding PAIR (ties inside a pair are already in index order: the packed order); longer
    // chains of equal quantised coordinates (rare) get the loop-until-clean form
    const bool chained = __builtin_amdgcn_readfirstlane((int)(__ballot(chain) != 0ull)) != 0;
    exact_order_fixup<EPT>(val, idx, lane, chained ? EPT * kWave : 1);
  }
#endif
  __builtin_amdgcn_wave_barrier();
}

// project one cloud, sort it (packed keys), recover exact sorted coordinates + original indices
template <int EPT>
__device__ __forceinline__ float sorted_with_indices(const float* __restrict__ X, int count, int lane,
                                                     const float (&U)[6], float* orig, float (&val)[EPT],
                                                     int (&idx)[EPT]) {
  typedef Packing<EPT> PK;
  unsigned pk[EPT];
  float part;
  {
    float key[EPT];
    part = load_coords<EPT>(X, count, lane, U, key);
    // pin the coordinate sum HERE: left alone, the compiler sinks the 64*EPT additions below the sort and
    // keeps every unsorted coordinate alive in a register across it
    asm volatile("" : "+v"(part));
#pragma unroll
    for (int r = 0; r < EPT; ++r) {
      const int i = r * kWave + lane;
      orig[i] = key[r];                                  // exact coordinate by ORIGINAL index (pads: +inf)
      pk[r] = PK::pack(key[r], i, i < count);
    }
  }
  wave_sort<EPT>(pk, lane);
  __builtin_amdgcn_wave_barrier();
  unpack_sorted_words<EPT>(pk, orig, count, lane, val, idx);
  return part;
}

}  // namespace shw
