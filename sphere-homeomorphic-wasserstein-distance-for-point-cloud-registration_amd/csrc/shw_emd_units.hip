// shw_emd_units.hip -- exact Wasserstein cost between two uniform clouds of DIFFERENT sizes for MI355X (gfx950).
//
// Replaces ot.emd2 where the reference's trainers give source and target different point counts (train_W_COS.py:292-293,
// 334-336 --source_p_n / --target_p_n; train_RUNNER.py:193-218: 128 source points against 256 and 512 target points)
// and the loss is the exact one (Cos_disimilarity_W, Geodesic_distance_W).
//
// With g = gcd(n, m), ks = m / g, kt = n / g and U = lcm(n, m) = n ks = m kt, every source carries ks UNITS of mass 1 / U
// and every target has kt SLOTS for one unit each.  Supplies and demands are integers in units, so the transport polytope
// has integral vertices and the transport optimum is the optimum of the U x U assignment problem between units and slots
// with c(unit q, slot r) = C(x[q / ks], y[r / kt]).  That problem is solved by the rule of shw_emd.hip (eps-scaling
// forward auction on fixed-point costs, Jacobi rounds, one 64-bit LDS max per bid, the same tie rules, phases and caps;
// DESIGN.md, "Exact W for clouds of different sizes") with units bidding for slots -- without expanding anything:
//
//   * both clouds sit in LDS at their own sizes; a bidding unit evaluates C once per TARGET (m evaluations, not U) and
//     then walks the kt slot prices of that target.  Least and second least are taken over all slots: the second least may
//     be another slot of the same target.
//   * the per-unit / per-slot arrays (price, bid word, own word, holder, two queues, own slot) take 40 bytes per unit, the
//     clouds 12 bytes per point: emd_units_lds_bytes.  A pair is served when U <= 4096 (12 id bits in a bid word) and
//     that footprint fits the CU's LDS next to the static arrays: every pair with lcm(n, m) <= 2048, and above that
//     e.g. (768, 1024) and (1024, 1536), U = 3072.  A pair such as (1000, 1024), U = 128 000, is refused.
//   * every loop is bounded: a pair that needs more than emd_units_round_cap(U) rounds writes NaN and stops.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/shw.h"
#include "dispatch.hpp"
#include "emd_common.hpp"

namespace shw {

constexpr int kEmdUnitsMax = 1 << kEmdIdBits;                  // units: a bid word names its bidder in 12 bits
// dynamic LDS a pair may ask for: the CU's 160 KB less 1 KB for the kernel's static arrays (560 bytes)
constexpr size_t kEmdUnitsLdsMax = 160 * 1024 - 1024;

// the cap of shw_emd.hip (emd_round_cap) taken at U: the largest rounds / U seen is 122 (a registration-like pair of
// 1024 against 2048 points, angle cost; the restatement's cases stay below 72)
__host__ __device__ inline int emd_units_round_cap(int U) { return 1024 * U + 4096; }

__host__ __device__ inline size_t emd_units_stride(int v) { return (size_t)((v + 3) & ~3); }
// prices, bid words, own bids (8 bytes each), holder, two queues, own slot (4 bytes each) per unit; 3 floats per point
__host__ __device__ inline size_t emd_units_lds_bytes(int U, int n, int m) {
  return emd_units_stride(U) * (3 * 8 + 4 * 4) + (emd_units_stride(n) + emd_units_stride(m)) * (3 * 4);
}

// U = lcm(n, m) when the pair is served, else 0.  Host arithmetic only.
inline int emd_units_of(int n, int m) {
  if (n < 1 || m < 1 || n > kEmdMaxPoints || m > kEmdMaxPoints) return 0;
  const long U = (long)n * (m / gcd(n, m));
  if (U > kEmdUnitsMax) return 0;
  return emd_units_lds_bytes((int)U, n, m) <= kEmdUnitsLdsMax ? (int)U : 0;
}

// The bound on every cost of a pair, as emd_auction_kernel (shw_emd.hip) takes it inline, from each thread's bounding
// boxes of the points it staged (box: x min, x max, y min, y max, three floats each; red: kEmdWaves * 12 floats of LDS).
// KIND 0: |x_d - y_d| <= max(x max - y min, y max - x min) in every coordinate (rounded subtraction is monotone).
// KIND 1: pi^p.  Holds a barrier for KIND 0.
template <int KIND, int PM>
__device__ __forceinline__ float emd_cost_bound(float (&box)[12], float* red, float p) {
  if constexpr (KIND == 0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const bool is_min = (k % 6) < 3;
#pragma unroll
      for (int w = 1; w < 64; w <<= 1) {
        const float o = __shfl_xor(box[k], w);
        box[k] = is_min ? fminf(box[k], o) : fmaxf(box[k], o);
      }
      if (lane == 0) red[wave * 12 + k] = box[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const bool is_min = (k % 6) < 3;
      float v = red[k];
      for (int w = 1; w < kEmdWaves; ++w) v = is_min ? fminf(v, red[w * 12 + k]) : fmaxf(v, red[w * 12 + k]);
      box[k] = v;
    }
    float t[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float span = fmaxf(box[3 + d] - box[6 + d], box[9 + d] - box[d]);
      t[d] = PM == 2 ? span * span : (PM == 1 ? span : powf(span, p));
    }
    return (t[0] + t[1]) + t[2];
  } else {
    return PM == 1 ? 3.14159274f : powf(3.14159274f, p);
  }
}

// s dC(a, b)/da, the formulas of emd_backward_kernel (shw_emd.hip), restated here because moving them out of that kernel
// changed its instruction schedule.  Both costs are symmetric in (a, b): one function serves either side.
template <int KIND, int PM>
__device__ __forceinline__ void emd_cost_grad(float ax, float ay, float az, float bx, float by, float bz, float p, float s,
                                              float& gx, float& gy, float& gz) {
  if constexpr (KIND == 0) {
    // C = sum_d |a_d - b_d|^p is symmetric in (a, b): the derivative in the own point is p |d|^(p-1) sgn(d), d = a - b
    const float d[3] = {ax - bx, ay - by, az - bz};
    float g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float sg = d[k] > 0.f ? 1.f : (d[k] < 0.f ? -1.f : 0.f);
      if constexpr (PM == 2) g[k] = 2.f * d[k];
      else if constexpr (PM == 1) g[k] = sg;
      else g[k] = d[k] == 0.f ? 0.f : p * powf(fabsf(d[k]), p - 1.f) * sg;
    }
    gx = s * g[0]; gy = s * g[1]; gz = s * g[2];
  } else {
    // theta = atan2(S, c), S = |a x b|, c = a . b:  d theta / da = (c (b x nu) - S b) / (|a|^2 |b|^2), nu = (a x b) / S
    // (also symmetric in (a, b)).  Where S = 0 or a point has zero length the angle has no derivative: 0 is written
    // (the reference's acos gives inf / NaN there).
    float cx, cy, cz;
    emd_cross(ax, ay, az, bx, by, bz, cx, cy, cz);
    const float S = sqrtf(fmaf(cz, cz, fmaf(cy, cy, cx * cx)));
    const float c = fmaf(az, bz, fmaf(ay, by, ax * bx));
    const float na = fmaf(az, az, fmaf(ay, ay, ax * ax)), nb = fmaf(bz, bz, fmaf(by, by, bx * bx));
    if (S == 0.f || na == 0.f || nb == 0.f) {
      gx = gy = gz = 0.f;
    } else {
      const float th = atan2f(S, c);
      const float f = PM == 2 ? 2.f * th : (PM == 1 ? 1.f : p * powf(th, p - 1.f));
      const float iS = 1.f / S, nx = cx * iS, ny = cy * iS, nz = cz * iS;
      const float ux = fmaf(by, nz, -(bz * ny)), uy = fmaf(bz, nx, -(bx * nz)), uz = fmaf(bx, ny, -(by * nx));   // b x nu
      const float k = s * f / (na * nb);
      gx = k * fmaf(c, ux, -(S * bx)); gy = k * fmaf(c, uy, -(S * by)); gz = k * fmaf(c, uz, -(S * bz));
    }
  }
}

struct EmdUnitsLds {
  long long* price;             // price of each slot
  unsigned long long* word;     // highest bid each slot has seen: (price << 12) | (4095 - unit)
  unsigned long long* mybid;    // by queue position: the word this round's bidder offered
  int* holder;                  // unit that holds each slot in this phase, -1 = none
  int *queue0, *queue1;         // unassigned units of this round / of the next, swapping roles every round
  int* myslot;                  // by queue position: the slot bid for
  float *xx, *xy, *xz, *yx, *yy, *yz;
};

__device__ __forceinline__ EmdUnitsLds emd_units_carve(unsigned char* raw, int U, int n, int m) {
  const size_t su = emd_units_stride(U), sn = emd_units_stride(n), sm = emd_units_stride(m);
  EmdUnitsLds L;
  L.price = reinterpret_cast<long long*>(raw);
  L.word = reinterpret_cast<unsigned long long*>(raw) + su;
  L.mybid = L.word + su;
  int* q = reinterpret_cast<int*>(L.mybid + su);
  L.holder = q; L.queue0 = q + su; L.queue1 = q + 2 * su; L.myslot = q + 3 * su;
  float* f = reinterpret_cast<float*>(q + 4 * su);               // (16-byte aligned: every stride is a multiple of 4)
  L.xx = f; L.xy = f + sn; L.xz = f + 2 * sn;
  f += 3 * sn;
  L.yx = f; L.yy = f + sm; L.yz = f + 2 * sm;
  return L;
}

// unit u (queue position q) offers price + (second least - least) + eps for its best slot: the word goes to the slot's
// 64-bit max, and is kept by queue position so that the bidder can see after the barrier whether it stands
__device__ __forceinline__ void emd_units_place_bid(const EmdUnitsLds& L, EmdBest B, int q, int u, long long eps) {
  if (B.m2 == INT64_MAX) B.m2 = B.m1;                                // U == 1: no second slot
  long long offer = L.price[B.a1] + (B.m2 - B.m1) + eps;
  offer = offer < kEmdPriceCap ? offer : kEmdPriceCap;
  const unsigned long long w = ((unsigned long long)offer << kEmdIdBits) | (unsigned)(4095 - u);
  L.myslot[q] = B.a1;
  L.mybid[q] = w;
  atomicMax(&L.word[B.a1], w);
}

// u / ks for a unit u < 4096 without the integer division, which sits on every round's critical path (Q -> source ->
// its point -> costs).  magic = ceil(2^32 / ks) = (2^32 + e) / ks with 0 <= e < ks, so u magic / 2^32 = u / ks + u e / (ks 2^32),
// and the excess is below u / 2^32 <= 2^-20 while the fraction of u / ks is at most 1 - 1 / ks <= 1 - 2^-11: the floor is
// exact.  ks == 1 (magic would be 2^32) is the identity.
struct EmdUnitsSource {
  unsigned magic;
  __device__ __forceinline__ explicit EmdUnitsSource(int ks)
      : magic(ks == 1 ? 0u : (unsigned)((0x100000000ull + (unsigned)ks - 1) / (unsigned)ks)) {}
  __device__ __forceinline__ int operator()(int u) const { return magic ? (int)__umulhi((unsigned)u, magic) : u; }
};

// the kt slots of target j, whose integer cost for this bidder is c.  KT1: kt == 1, slot j is target j
template <bool KT1>
__device__ __forceinline__ void emd_units_take_slots(EmdBest& B, const long long* price, long long c, int j, int kt) {
  if constexpr (KT1) {
    B.take(c + price[j], j);
  } else {
    const int r0 = j * kt;
    for (int s = 0; s < kt; ++s) B.take(c + price[r0 + s], r0 + s);
  }
}

// grid: (pairs); block: kEmdThreads; dynamic LDS: emd_units_lds_bytes(U, n, m).  U = n ks = m kt.
// KT1: kt == 1 (n divides m: the runner's 128 against 256 / 512, and n == m): a target is its one slot, and the bidding
// loops are those of emd_auction_kernel, prices read two per 16-byte load -- the general form's inner slot loop cost 3 to
// 11 % at these shapes.
template <int KIND, int PM, bool KT1>
__global__ __launch_bounds__(kEmdThreads) void emd_units_auction_kernel(
    const float* __restrict__ x, const float* __restrict__ y, int n, int m, int ks, int kt, float p,
    int32_t* __restrict__ ws_unit_target, int32_t* __restrict__ ws_slot_source, int32_t* __restrict__ ws_ok,
    float* __restrict__ cost, int32_t* __restrict__ targets, int32_t* __restrict__ rounds_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  __shared__ float red[kEmdWaves * 12];
  __shared__ long long part_m1[kEmdWaves], part_m2[kEmdWaves];      // per-wave summaries of a bidder spread over waves
  __shared__ int part_a1[kEmdWaves];
  __shared__ int cnt[2];
  __shared__ int overflow;
  const int U = n * ks;
  const EmdUnitsSource source_of(ks);
  const EmdUnitsLds L = emd_units_carve(lds_raw, U, n, m);
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* X = x + (long)b * n * 3;
  const float* Y = y + (long)b * m * 3;

  // ---- stage both clouds (SoA) and take their bounding boxes
  const float inf = __builtin_inff();
  float box[12] = {inf, inf, inf, -inf, -inf, -inf, inf, inf, inf, -inf, -inf, -inf};   // x min, x max, y min, y max
  for (int i = tid; i < n; i += kEmdThreads) {
    const float ax = X[3 * i], ay = X[3 * i + 1], az = X[3 * i + 2];
    L.xx[i] = ax; L.xy[i] = ay; L.xz[i] = az;
    box[0] = fminf(box[0], ax); box[1] = fminf(box[1], ay); box[2] = fminf(box[2], az);
    box[3] = fmaxf(box[3], ax); box[4] = fmaxf(box[4], ay); box[5] = fmaxf(box[5], az);
  }
  for (int j = tid; j < m; j += kEmdThreads) {
    const float bx = Y[3 * j], by = Y[3 * j + 1], bz = Y[3 * j + 2];
    L.yx[j] = bx; L.yy[j] = by; L.yz[j] = bz;
    box[6] = fminf(box[6], bx); box[7] = fminf(box[7], by); box[8] = fminf(box[8], bz);
    box[9] = fmaxf(box[9], bx); box[10] = fmaxf(box[10], by); box[11] = fmaxf(box[11], bz);
  }
  for (int r = tid; r < U; r += kEmdThreads) {
    L.price[r] = 0;
    L.word[r] = 0;
  }
  const float bound = emd_cost_bound<KIND, PM>(box, red, p);
  // K = 2^e >= 1.001 bound (the margin covers the rounding of the bound itself); scale = 2^26 / K
  const bool all_zero = !(bound > 0.f);                  // every cost is 0 (or the inputs hold nothing finite)
  bool failed = !all_zero && !(bound < inf);
  int e = 0;
  (void)frexpf(bound * 1.001f, &e);
  e = e < -100 ? -100 : e;
  const float scale = ldexpf(1.f, kEmdFracBits - e);
  const int cap = emd_units_round_cap(U);

  int rounds = 0;
  if (tid == 0) overflow = 0;
  if (all_zero || failed) {
    for (int r = tid; r < U; r += kEmdThreads) L.holder[r] = r;      // the identity: unit q in slot q
  } else {
    for (long long eps = kEmdEpsFirst; eps >= 1 && !failed; eps >>= kEmdEpsShift) {
      __syncthreads();
      for (int r = tid; r < U; r += kEmdThreads) {
        L.holder[r] = -1;
        L.queue0[r] = r;
      }
      if (tid == 0) { cnt[0] = 0; cnt[1] = 0; }
      int count = U, cur = 0;
      __syncthreads();
      while (count > 0) {
        if (rounds >= cap) { failed = true; break; }                 // (block-uniform)
        ++rounds;
        const int* Q = cur ? L.queue1 : L.queue0;
        // lanes per bidder: as many as the block has to spare
        int g = 1;
        while (g < kEmdThreads && count * (2 * g) <= kEmdThreads) g <<= 1;
        if (g == 1) {
          // many bidders: one thread each; the targets stream from LDS as broadcast reads, four at a time, each followed
          // by its kt slot prices
          for (int q = tid; q < count; q += kEmdThreads) {
            const int u = Q[q], i = source_of(u);
            const float ax = L.xx[i], ay = L.xy[i], az = L.xz[i];
            EmdBest B = {INT64_MAX, INT64_MAX, 0};
            int j = 0;
            for (; j + 4 <= m; j += 4) {
              const float4 vx = *reinterpret_cast<const float4*>(L.yx + j);
              const float4 vy = *reinterpret_cast<const float4*>(L.yy + j);
              const float4 vz = *reinterpret_cast<const float4*>(L.yz + j);
              if constexpr (KT1) {
                const longlong2 p01 = *reinterpret_cast<const longlong2*>(L.price + j);
                const longlong2 p23 = *reinterpret_cast<const longlong2*>(L.price + j + 2);
                B.take(emd_cost_fixed<KIND, PM>(ax, ay, az, vx.x, vy.x, vz.x, p, scale) + p01.x, j);
                B.take(emd_cost_fixed<KIND, PM>(ax, ay, az, vx.y, vy.y, vz.y, p, scale) + p01.y, j + 1);
                B.take(emd_cost_fixed<KIND, PM>(ax, ay, az, vx.z, vy.z, vz.z, p, scale) + p23.x, j + 2);
                B.take(emd_cost_fixed<KIND, PM>(ax, ay, az, vx.w, vy.w, vz.w, p, scale) + p23.y, j + 3);
              } else {
                const long long c0 = emd_cost_fixed<KIND, PM>(ax, ay, az, vx.x, vy.x, vz.x, p, scale);
                const long long c1 = emd_cost_fixed<KIND, PM>(ax, ay, az, vx.y, vy.y, vz.y, p, scale);
                const long long c2 = emd_cost_fixed<KIND, PM>(ax, ay, az, vx.z, vy.z, vz.z, p, scale);
                const long long c3 = emd_cost_fixed<KIND, PM>(ax, ay, az, vx.w, vy.w, vz.w, p, scale);
                emd_units_take_slots<false>(B, L.price, c0, j, kt);
                emd_units_take_slots<false>(B, L.price, c1, j + 1, kt);
                emd_units_take_slots<false>(B, L.price, c2, j + 2, kt);
                emd_units_take_slots<false>(B, L.price, c3, j + 3, kt);
              }
            }
            for (; j < m; ++j)
              emd_units_take_slots<KT1>(B, L.price, emd_cost_fixed<KIND, PM>(ax, ay, az, L.yx[j], L.yy[j], L.yz[j], p, scale),
                                        j, kt);
            emd_units_place_bid(L, B, q, u, eps);
          }
        } else {
          // few bidders: g lanes each, striding the TARGETS (a lane walks all slots of its targets), merged by a butterfly
          // inside the wave and, from 4 bidders down (g = 128, 256, 512: 2, 4, 8 waves per bidder), across the group's
          // waves through LDS.  count * g <= the block, so one pass; a lane without a bidder works on queue position 0 and
          // writes nothing
          const int q = tid / g, sub = tid & (g - 1);
          const bool active = q < count;
          const int u = Q[active ? q : 0], i = source_of(u);
          const float ax = L.xx[i], ay = L.xy[i], az = L.xz[i];
          EmdBest B = {INT64_MAX, INT64_MAX, 0};
          if constexpr (KT1) {
#pragma unroll 4
            for (int j = sub; j < m; j += g)
              B.take(emd_cost_fixed<KIND, PM>(ax, ay, az, L.yx[j], L.yy[j], L.yz[j], p, scale) + L.price[j], j);
          } else {
            for (int j = sub; j < m; j += g)
              emd_units_take_slots<false>(B, L.price, emd_cost_fixed<KIND, PM>(ax, ay, az, L.yx[j], L.yy[j], L.yz[j], p, scale),
                                          j, kt);
          }
          const int in_wave = g < 64 ? g : 64;
          for (int w = 1; w < in_wave; w <<= 1) {
            const long long o1 = __shfl_xor(B.m1, w), o2 = __shfl_xor(B.m2, w);
            const int oa = __shfl_xor(B.a1, w);
            B.merge(o1, o2, oa);
          }
          if (g > 64) {                                              // (block-uniform)
            if (lane == 0) { part_m1[wave] = B.m1; part_m2[wave] = B.m2; part_a1[wave] = B.a1; }
            __syncthreads();
            if (sub == 0)
              for (int w = wave + 1; w < wave + g / 64; ++w) B.merge(part_m1[w], part_m2[w], part_a1[w]);
          }
          if (active && sub == 0) emd_units_place_bid(L, B, q, u, eps);
        }
        __syncthreads();
        // the bidder whose word stands takes the slot and sends its holder back to the queue; the others queue again.
        // Words only grow (an accepted bid is above the price it was made at), so they are never cleared.
        int* Qn = cur ? L.queue0 : L.queue1;
        for (int q = tid; q < count; q += kEmdThreads) {
          const int u = Q[q], r = L.myslot[q];
          const unsigned long long w = L.mybid[q];
          int back = u;
          if (L.word[r] == w) {
            back = L.holder[r];
            L.holder[r] = u;
            L.price[r] = (long long)(w >> kEmdIdBits);
            if ((long long)(w >> kEmdIdBits) >= kEmdPriceCap) overflow = 1;
          }
          if (back >= 0) Qn[atomicAdd(&cnt[cur ^ 1], 1)] = back;
        }
        __syncthreads();
        count = cnt[cur ^ 1];
        if (overflow) { failed = true; break; }
        if (tid == 0) cnt[cur] = 0;
        cur ^= 1;
      }
    }
  }
  __syncthreads();

  // ---- outputs: the target of each unit, the source of each slot, the mean cost over the units (fixed order: strided
  // partial sums, a butterfly per wave, the waves in order)
  int32_t* out_targets = targets + (long)b * U;
  int32_t* out_unit = ws_unit_target + (long)b * U;
  int32_t* out_slot = ws_slot_source + (long)b * U;
  if (failed) {
    for (int r = tid; r < U; r += kEmdThreads) { out_targets[r] = r / kt; out_unit[r] = r / kt; out_slot[r] = r / ks; }
    if (tid == 0) {
      cost[b] = __builtin_nanf("");
      rounds_out[b] = cap;
      ws_ok[b] = 0;
    }
    return;
  }
  int* slot_of = L.queue0;
  for (int r = tid; r < U; r += kEmdThreads) {
    const int u = L.holder[r];
    slot_of[u] = r;
    out_slot[r] = source_of(u);
  }
  __syncthreads();
  float acc = 0.f;
  for (int u = tid; u < U; u += kEmdThreads) {
    const int i = source_of(u), j = slot_of[u] / kt;
    out_targets[u] = j;
    out_unit[u] = j;
    acc += emd_cost<KIND, PM>(L.xx[i], L.xy[i], L.xz[i], L.yx[j], L.yy[j], L.yz[j], p);
  }
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) acc += __shfl_xor(acc, w);
  __syncthreads();
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    for (int w = 0; w < kEmdWaves; ++w) s += red[w];
    cost[b] = s / (float)U;
    rounds_out[b] = rounds;
    ws_ok[b] = 1;
  }
}

// d/dx_i of w_b (1/U) sum_q C(x[q / ks], y[target(q)]) and d/dy_j likewise over the slots of y_j: the plan is locally
// constant, so this is what ot.emd2's autograd gives through C.  OWNER-COMPUTED: thread (z, row) sums the k couples of its
// row in unit (slot) order and writes that row of one gradient and nothing else -- no atomics, the same bits on every run.
// A pair that was given up (cost NaN) gets zeros.
// grid: (ceil(max(n, m) / 256), pairs, 2): z = 0 rows of grad_x (ks units each), z = 1 rows of grad_y (kt slots each)
template <int KIND, int PM>
__global__ __launch_bounds__(256) void emd_units_backward_kernel(
    const float* __restrict__ x, const float* __restrict__ y, const int32_t* __restrict__ ws_unit_target,
    const int32_t* __restrict__ ws_slot_source, const int32_t* __restrict__ ws_ok, const float* __restrict__ w, int n, int m,
    int ks, int kt, float p, float* __restrict__ grad_x, float* __restrict__ grad_y) {
  const int b = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x;
  const bool ys = blockIdx.z != 0;
  const int rows = ys ? m : n, others = ys ? n : m, k = ys ? kt : ks;
  if (r >= rows) return;
  const long U = (long)n * ks;
  float* G = (ys ? grad_y : grad_x) + ((long)b * rows + r) * 3;
  if (!ws_ok[b]) {
    G[0] = 0.f; G[1] = 0.f; G[2] = 0.f;
    return;
  }
  const int32_t* partner = (ys ? ws_slot_source : ws_unit_target) + (long)b * U + (long)r * k;
  const float* A = (ys ? y : x) + ((long)b * rows + r) * 3;      // the point this row belongs to
  const float* O = (ys ? x : y) + (long)b * others * 3;          // the cloud of its partners
  const float ax = A[0], ay = A[1], az = A[2];
  const float s = w[b] / (float)U;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (int e = 0; e < k; ++e) {
    int o = partner[e];
    o = o < 0 ? 0 : (o >= others ? others - 1 : o);              // (a workspace this library did not write cannot reach outside)
    float gx, gy, gz;
    emd_cost_grad<KIND, PM>(ax, ay, az, O[3 * o], O[3 * o + 1], O[3 * o + 2], p, s, gx, gy, gz);
    sx += gx; sy += gy; sz += gz;
  }
  G[0] = sx; G[1] = sy; G[2] = sz;
}

struct EmdUnitsWorkspace {
  int32_t *unit_target, *slot_source, *ok;
};
inline EmdUnitsWorkspace emd_units_workspace(void* ws, int pairs, int U) {
  int32_t* base = static_cast<int32_t*>(ws);
  return {base, base + (size_t)pairs * U, base + 2 * (size_t)pairs * U};
}

// U when every argument is in range, else 0
inline int emd_units_args_ok(int pairs, int n, int m, int kind, float p) {
  if (pairs < 0 || pairs > 65535 || (kind != 0 && kind != 1) || !(p >= 1.f)) return 0;
  return emd_units_of(n, m);
}

template <int KIND, int PM, bool KT1>
inline int emd_units_launch_auction(const float* x, const float* y, int pairs, int n, int m, int U, size_t lds, float p,
                                    const EmdUnitsWorkspace& W, float* cost, int32_t* targets, int32_t* rounds,
                                    hipStream_t stream) {
  const hipError_t e = raise_dynamic_lds<emd_units_auction_kernel<KIND, PM, KT1>>(lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((emd_units_auction_kernel<KIND, PM, KT1>), dim3(pairs), dim3(kEmdThreads), lds, stream, x, y, n, m,
                     U / n, U / m, p, W.unit_target, W.slot_source, W.ok, cost, targets, rounds);
  return (int)hipGetLastError();
}

template <int KIND, int PM>
inline int emd_units_launch_forward(const float* x, const float* y, int pairs, int n, int m, int U, float p,
                                    const EmdUnitsWorkspace& W, float* cost, int32_t* targets, int32_t* rounds,
                                    hipStream_t stream) {
  const size_t lds = emd_units_lds_bytes(U, n, m);
  return U == m ? emd_units_launch_auction<KIND, PM, true>(x, y, pairs, n, m, U, lds, p, W, cost, targets, rounds, stream)
                : emd_units_launch_auction<KIND, PM, false>(x, y, pairs, n, m, U, lds, p, W, cost, targets, rounds, stream);
}

template <int KIND, int PM>
inline int emd_units_launch_backward(const float* x, const float* y, const EmdUnitsWorkspace& W, const float* w, int pairs,
                                     int n, int m, int U, float p, float* grad_x, float* grad_y, hipStream_t stream) {
  const int rows = n > m ? n : m;
  hipLaunchKernelGGL((emd_units_backward_kernel<KIND, PM>), dim3((rows + 255) / 256, pairs, 2), dim3(256), 0, stream, x, y,
                     W.unit_target, W.slot_source, W.ok, w, n, m, U / n, U / m, p, grad_x, grad_y);
  return (int)hipGetLastError();
}

}  // namespace shw

extern "C" {

int shw_emd_units_supported(int n, int m) { return shw::emd_units_of(n, m); }

size_t shw_emd_units_workspace_bytes(int pairs, int n, int m) {
  const int U = shw::emd_units_of(n, m);
  if (pairs < 0 || U == 0) return 0;
  return ((size_t)pairs * U * 2 + (size_t)pairs) * sizeof(int32_t);
}

int shw_emd_units_forward(const float* x, const float* y, int pairs, int n, int m, int kind, float p, void* workspace,
                          float* cost, int32_t* targets, int32_t* rounds, void* stream) {
  if (!x || !y || !workspace || !cost || !targets || !rounds) return (int)hipErrorInvalidValue;
  const int U = shw::emd_units_args_ok(pairs, n, m, kind, p);
  if (U == 0) return (int)hipErrorInvalidValue;
  if (pairs == 0) return 0;
  const shw::EmdUnitsWorkspace W = shw::emd_units_workspace(workspace, pairs, U);
  return shw::emd_with_kind(kind, p, [&](auto K, auto PM) {
    return shw::emd_units_launch_forward<decltype(K)::value, decltype(PM)::value>(x, y, pairs, n, m, U, p, W, cost, targets,
                                                                                  rounds, (hipStream_t)stream);
  });
}

int shw_emd_units_backward(const float* x, const float* y, const void* workspace, const float* w, int pairs, int n, int m,
                           int kind, float p, float* grad_x, float* grad_y, void* stream) {
  if (!x || !y || !workspace || !w || !grad_x || !grad_y) return (int)hipErrorInvalidValue;
  const int U = shw::emd_units_args_ok(pairs, n, m, kind, p);
  if (U == 0) return (int)hipErrorInvalidValue;
  if (pairs == 0) return 0;
  const shw::EmdUnitsWorkspace W = shw::emd_units_workspace(const_cast<void*>(workspace), pairs, U);
  return shw::emd_with_kind(kind, p, [&](auto K, auto PM) {
    return shw::emd_units_launch_backward<decltype(K)::value, decltype(PM)::value>(x, y, W, w, pairs, n, m, U, p, grad_x,
                                                                                   grad_y, (hipStream_t)stream);
  });
}

}  // extern "C"
