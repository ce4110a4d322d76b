// shw_emd.hip -- exact Wasserstein cost between two uniform clouds of EQUAL size for MI355X (gfx950).
//
// Replaces ot.emd2 as the reference's live loss calls it (losses/s2_wasserstein.py:13-66 Cos_disimilarity_W, :73-126
// Geodesic_distance_W; Flow_cube.ipynb cell 5 wasserstein_distance / wasserstein_distance_geo): with n = m and uniform
// weights the transport problem is a linear assignment problem, solved here by an eps-scaling forward auction on
// fixed-point costs ("Exact W for equal-size clouds").
//
//   * one workgroup per pair; both clouds live in LDS and the cost of a (source, target) couple is recomputed by ONE
//     device function (emd_cost) wherever it is needed: the bidding loop, the final sum, and -- differentiated -- the
//     backward kernel.  No cost matrix is ever stored.
//   * costs become integers c = floor(C 2^s), 2^s K = 2^26, K a power of two above the largest cost, found in the
//     kernel (bounding boxes / pi^p).  Prices and bids are int64: an accepted bid raises a price by at least eps >= 1,
//     so progress never hangs on a float ulp.
//   * Jacobi rounds: every unassigned source bids (least c + price, ties to the lowest target; increment second least -
//     least + eps); a target takes its highest bid, ties to the lowest bidder -- one LDS 64-bit max over the word
//     (new price, 4095 - bidder), which is order independent: the result is deterministic.
//   * eps = 2^24, 2^21, ..., 1; prices are kept from phase to phase, the assignment starts empty in each.
//   * every loop is bounded: a pair that needs more than emd_round_cap(n) rounds writes NaN and stops.
// The cost function, the bidder's summary and the rule's constants are in emd_common.hpp, shared with shw_emd_units.hip,
// which serves clouds of different sizes by the same rule on units of mass.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/shw.h"
#include "dispatch.hpp"
#include "emd_common.hpp"

namespace shw {

// The largest rounds / n the CPU restatement records is 73, on clouds whose costs are all equal (tests/helpers/
// emd_cases.py); the cap is more than 8 x that, and its constant term covers the 9 phases of the smallest clouds
__host__ __device__ inline int emd_round_cap(int n) { return 1024 * n + 4096; }

__host__ __device__ inline size_t emd_lds_stride(int n) { return (size_t)((n + 3) & ~3); }
// prices, bid words, own bids (8 bytes each) + both clouds (3 + 3 floats), owner, two queues, own target (4 bytes each)
__host__ __device__ inline size_t emd_lds_bytes(int n) { return emd_lds_stride(n) * (3 * 8 + 10 * 4); }

struct EmdLds {
  long long* price;             // price of each target
  unsigned long long* word;     // highest bid each target has seen: (price << 12) | (4095 - bidder)
  unsigned long long* mybid;    // by queue slot: the word this round's bidder offered
  float *yx, *yy, *yz, *xx, *xy, *xz;
  int* owner;                   // source that holds each target in this phase, -1 = none
  int *queue0, *queue1;         // unassigned sources of this round / of the next, swapping roles every round
  int* myobj;                   // by queue slot: the target bid for
};

// bidder i (queue slot q) offers price + (second least - least) + eps for its best target: the word goes to the
// target's 64-bit max, and is kept by slot so that the bidder can see after the barrier whether it stands
__device__ __forceinline__ void emd_place_bid(const EmdLds& L, EmdBest B, int q, int i, long long eps) {
  if (B.m2 == INT64_MAX) B.m2 = B.m1;                                // n == 1: no second target
  long long offer = L.price[B.a1] + (B.m2 - B.m1) + eps;
  offer = offer < kEmdPriceCap ? offer : kEmdPriceCap;
  const unsigned long long w = ((unsigned long long)offer << kEmdIdBits) | (unsigned)(4095 - i);
  L.myobj[q] = B.a1;
  L.mybid[q] = w;
  atomicMax(&L.word[B.a1], w);
}

__device__ __forceinline__ EmdLds emd_carve(unsigned char* raw, int n) {
  const size_t st = emd_lds_stride(n);
  EmdLds L;
  L.price = reinterpret_cast<long long*>(raw);
  L.word = reinterpret_cast<unsigned long long*>(raw) + st;
  L.mybid = L.word + st;
  float* f = reinterpret_cast<float*>(L.mybid + st);
  L.yx = f; L.yy = f + st; L.yz = f + 2 * st;
  L.xx = f + 3 * st; L.xy = f + 4 * st; L.xz = f + 5 * st;
  int* q = reinterpret_cast<int*>(f + 6 * st);
  L.owner = q; L.queue0 = q + st; L.queue1 = q + 2 * st; L.myobj = q + 3 * st;
  return L;
}

// grid: (pairs); block: kEmdThreads; dynamic LDS: emd_lds_bytes(n)
template <int KIND, int PM>
__global__ __launch_bounds__(kEmdThreads) void emd_auction_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                  int n, float p, int32_t* __restrict__ ws_inv,
                                                                  int32_t* __restrict__ ws_assign, int32_t* __restrict__ ws_ok,
                                                                  float* __restrict__ cost, int32_t* __restrict__ assign,
                                                                  int32_t* __restrict__ rounds_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  __shared__ float red[kEmdWaves * 12];
  __shared__ long long part_m1[kEmdWaves], part_m2[kEmdWaves];      // per-wave summaries of a bidder spread over waves
  __shared__ int part_a1[kEmdWaves];
  __shared__ int cnt[2];
  __shared__ int overflow;
  const EmdLds L = emd_carve(lds_raw, n);
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* X = x + (long)b * n * 3;
  const float* Y = y + (long)b * n * 3;

  // ---- stage both clouds (SoA) and take their bounding boxes
  const float inf = __builtin_inff();
  float box[12] = {inf, inf, inf, -inf, -inf, -inf, inf, inf, inf, -inf, -inf, -inf};   // x min, x max, y min, y max
  for (int i = tid; i < n; i += kEmdThreads) {
    const float ax = X[3 * i], ay = X[3 * i + 1], az = X[3 * i + 2];
    const float bx = Y[3 * i], by = Y[3 * i + 1], bz = Y[3 * i + 2];
    L.xx[i] = ax; L.xy[i] = ay; L.xz[i] = az;
    L.yx[i] = bx; L.yy[i] = by; L.yz[i] = bz;
    box[0] = fminf(box[0], ax); box[1] = fminf(box[1], ay); box[2] = fminf(box[2], az);
    box[3] = fmaxf(box[3], ax); box[4] = fmaxf(box[4], ay); box[5] = fmaxf(box[5], az);
    box[6] = fminf(box[6], bx); box[7] = fminf(box[7], by); box[8] = fminf(box[8], bz);
    box[9] = fmaxf(box[9], bx); box[10] = fmaxf(box[10], by); box[11] = fmaxf(box[11], bz);
    L.price[i] = 0;
    L.word[i] = 0;
  }
  float bound;
  if constexpr (KIND == 0) {
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
    // |x_d - y_d| <= max(x max - y min, y max - x min) in every coordinate (rounded subtraction is monotone)
    float t[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float span = fmaxf(box[3 + d] - box[6 + d], box[9 + d] - box[d]);
      t[d] = PM == 2 ? span * span : (PM == 1 ? span : powf(span, p));
    }
    bound = (t[0] + t[1]) + t[2];
  } else {
    bound = PM == 1 ? 3.14159274f : powf(3.14159274f, p);
  }
  // K = 2^e >= 1.001 bound (the margin covers the rounding of the bound itself); scale = 2^26 / K
  const bool all_zero = !(bound > 0.f);                  // every cost is 0 (or the inputs hold nothing finite)
  bool failed = !all_zero && !(bound < inf);
  int e = 0;
  (void)frexpf(bound * 1.001f, &e);
  e = e < -100 ? -100 : e;
  const float scale = ldexpf(1.f, kEmdFracBits - e);
  const int cap = emd_round_cap(n);

  int rounds = 0;
  if (tid == 0) overflow = 0;
  if (all_zero || failed) {
    for (int j = tid; j < n; j += kEmdThreads) L.owner[j] = j;       // the identity assignment
  } else {
    for (long long eps = kEmdEpsFirst; eps >= 1 && !failed; eps >>= kEmdEpsShift) {
      __syncthreads();
      for (int j = tid; j < n; j += kEmdThreads) {
        L.owner[j] = -1;
        L.queue0[j] = j;
      }
      if (tid == 0) { cnt[0] = 0; cnt[1] = 0; }
      int count = n, cur = 0;
      __syncthreads();
      while (count > 0) {
        if (rounds >= cap) { failed = true; break; }                 // (block-uniform)
        ++rounds;
        const int* Q = cur ? L.queue1 : L.queue0;
        // lanes per bidder: as many as the block has to spare
        int g = 1;
        while (g < kEmdThreads && count * (2 * g) <= kEmdThreads) g <<= 1;
        if (g == 1) {
          // many bidders: one thread each, the targets stream from LDS as broadcast reads, four at a time
          for (int q = tid; q < count; q += kEmdThreads) {
            const int i = Q[q];
            const float ax = L.xx[i], ay = L.xy[i], az = L.xz[i];
            EmdBest B = {INT64_MAX, INT64_MAX, 0};
            int j = 0;
            for (; j + 4 <= n; j += 4) {
              const float4 vx = *reinterpret_cast<const float4*>(L.yx + j);
              const float4 vy = *reinterpret_cast<const float4*>(L.yy + j);
              const float4 vz = *reinterpret_cast<const float4*>(L.yz + j);
              const longlong2 p01 = *reinterpret_cast<const longlong2*>(L.price + j);
              const longlong2 p23 = *reinterpret_cast<const longlong2*>(L.price + j + 2);
              B.take(emd_cost_fixed<KIND, PM>(ax, ay, az, vx.x, vy.x, vz.x, p, scale) + p01.x, j);
              B.take(emd_cost_fixed<KIND, PM>(ax, ay, az, vx.y, vy.y, vz.y, p, scale) + p01.y, j + 1);
              B.take(emd_cost_fixed<KIND, PM>(ax, ay, az, vx.z, vy.z, vz.z, p, scale) + p23.x, j + 2);
              B.take(emd_cost_fixed<KIND, PM>(ax, ay, az, vx.w, vy.w, vz.w, p, scale) + p23.y, j + 3);
            }
            for (; j < n; ++j)
              B.take(emd_cost_fixed<KIND, PM>(ax, ay, az, L.yx[j], L.yy[j], L.yz[j], p, scale) + L.price[j], j);
            emd_place_bid(L, B, q, i, eps);
          }
        } else {
          // few bidders: g lanes each, striding the targets, merged by a butterfly inside the wave and, from 4 bidders
          // down (g = 128, 256, 512: 2, 4, 8 waves per bidder), across the group's waves through LDS.  count * g <= the
          // block, so one pass; a lane without a bidder works on slot 0 and writes nothing
          const int q = tid / g, sub = tid & (g - 1);
          const bool active = q < count;
          const int i = Q[active ? q : 0];
          const float ax = L.xx[i], ay = L.xy[i], az = L.xz[i];
          EmdBest B = {INT64_MAX, INT64_MAX, 0};
#pragma unroll 4
          for (int j = sub; j < n; j += g)
            B.take(emd_cost_fixed<KIND, PM>(ax, ay, az, L.yx[j], L.yy[j], L.yz[j], p, scale) + L.price[j], j);
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
          if (active && sub == 0) emd_place_bid(L, B, q, i, eps);
        }
        __syncthreads();
        // the bidder whose word stands takes the target and sends its holder back to the queue; the others queue again.
        // Words only grow (an accepted bid is above the price it was made at), so they are never cleared.
        int* Qn = cur ? L.queue0 : L.queue1;
        for (int q = tid; q < count; q += kEmdThreads) {
          const int i = Q[q], j = L.myobj[q];
          const unsigned long long w = L.mybid[q];
          int back = i;
          if (L.word[j] == w) {
            back = L.owner[j];
            L.owner[j] = i;
            L.price[j] = (long long)(w >> kEmdIdBits);
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

  // ---- outputs: the assignment, its inverse, the mean cost along it (fixed order: strided partial sums, a butterfly
  // per wave, the waves in order)
  int32_t* out_assign = assign + (long)b * n;
  int32_t* out_inv = ws_inv + (long)b * n;
  int32_t* out_copy = ws_assign + (long)b * n;
  if (failed) {
    for (int i = tid; i < n; i += kEmdThreads) { out_assign[i] = i; out_inv[i] = i; out_copy[i] = i; }
    if (tid == 0) {
      cost[b] = __builtin_nanf("");
      rounds_out[b] = cap;
      ws_ok[b] = 0;
    }
    return;
  }
  int* sigma = L.queue0;
  for (int j = tid; j < n; j += kEmdThreads) {
    const int i = L.owner[j];
    sigma[i] = j;
    out_inv[j] = i;
  }
  __syncthreads();
  float acc = 0.f;
  for (int i = tid; i < n; i += kEmdThreads) {
    const int j = sigma[i];
    out_assign[i] = j;
    out_copy[i] = j;
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
    cost[b] = s / (float)n;
    rounds_out[b] = rounds;
    ws_ok[b] = 1;
  }
}

// d/dx_i of w_b (1/n) sum_i C(x_i, y_sigma(i)) and, through the inverse permutation, d/dy_j: the plan is locally
// constant, so this is what ot.emd2's autograd gives through C.  OWNER-COMPUTED: thread (z, i) writes row i of one
// gradient and nothing else -- no atomics, the same bits on every run.  A pair that was given up (cost NaN) gets zeros.
// grid: (ceil(n / 256), pairs, 2): z = 0 rows of grad_x, z = 1 rows of grad_y
template <int KIND, int PM>
__global__ __launch_bounds__(256) void emd_backward_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                           const int32_t* __restrict__ ws_inv,
                                                           const int32_t* __restrict__ ws_assign,
                                                           const int32_t* __restrict__ ws_ok, const float* __restrict__ w,
                                                           int n, float p, float* __restrict__ grad_x,
                                                           float* __restrict__ grad_y) {
  const int b = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const bool ys = blockIdx.z != 0;
  float* G = (ys ? grad_y : grad_x) + ((long)b * n + r) * 3;
  if (!ws_ok[b]) {
    G[0] = 0.f; G[1] = 0.f; G[2] = 0.f;
    return;
  }
  int o = (ys ? ws_inv : ws_assign)[(long)b * n + r];
  o = o < 0 ? 0 : (o >= n ? n - 1 : o);                  // (a workspace this library did not write cannot reach outside)
  const float* A = (ys ? y : x) + ((long)b * n + r) * 3;         // the point this row belongs to
  const float* O = (ys ? x : y) + ((long)b * n + o) * 3;         // its partner
  const float ax = A[0], ay = A[1], az = A[2], bx = O[0], by = O[1], bz = O[2];
  const float s = w[b] / (float)n;
  float gx, gy, gz;
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
  G[0] = gx; G[1] = gy; G[2] = gz;
}

struct EmdWorkspace {
  int32_t *inv, *assign, *ok;
};
inline EmdWorkspace emd_workspace(void* ws, int pairs, int n) {
  int32_t* base = static_cast<int32_t*>(ws);
  return {base, base + (size_t)pairs * n, base + 2 * (size_t)pairs * n};
}

inline bool emd_sizes_ok(int pairs, int n, int kind, float p) {
  return pairs >= 0 && pairs <= 65535 && n >= 1 && n <= kEmdMaxPoints && (kind == 0 || kind == 1) && p >= 1.f;
}

template <int KIND, int PM>
inline int emd_launch_forward(const float* x, const float* y, int pairs, int n, float p, const EmdWorkspace& W, float* cost,
                              int32_t* assign, int32_t* rounds, hipStream_t stream) {
  const size_t lds = emd_lds_bytes(n);
  const hipError_t e = raise_dynamic_lds<emd_auction_kernel<KIND, PM>>(lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((emd_auction_kernel<KIND, PM>), dim3(pairs), dim3(kEmdThreads), lds, stream, x, y, n, p, W.inv,
                     W.assign, W.ok, cost, assign, rounds);
  return (int)hipGetLastError();
}

template <int KIND, int PM>
inline int emd_launch_backward(const float* x, const float* y, const EmdWorkspace& W, const float* w, int pairs, int n,
                               float p, float* grad_x, float* grad_y, hipStream_t stream) {
  hipLaunchKernelGGL((emd_backward_kernel<KIND, PM>), dim3((n + 255) / 256, pairs, 2), dim3(256), 0, stream, x, y, W.inv,
                     W.assign, W.ok, w, n, p, grad_x, grad_y);
  return (int)hipGetLastError();
}

}  // namespace shw

extern "C" {

int shw_max_points_emd(void) { return shw::kEmdMaxPoints; }

size_t shw_emd_workspace_bytes(int pairs, int n) {
  if (pairs < 0 || n < 1) return 0;
  return ((size_t)pairs * n * 2 + (size_t)pairs) * sizeof(int32_t);
}

int shw_emd_forward(const float* x, const float* y, int pairs, int n, int m, int kind, float p, void* workspace,
                    float* cost, int32_t* assign, int32_t* rounds, void* stream) {
  if (!x || !y || !workspace || !cost || !assign || !rounds) return (int)hipErrorInvalidValue;
  if (n != m || !shw::emd_sizes_ok(pairs, n, kind, p)) return (int)hipErrorInvalidValue;
  if (pairs == 0) return 0;
  const shw::EmdWorkspace W = shw::emd_workspace(workspace, pairs, n);
  return shw::emd_with_kind(kind, p, [&](auto K, auto PM) {
    return shw::emd_launch_forward<decltype(K)::value, decltype(PM)::value>(x, y, pairs, n, p, W, cost, assign, rounds,
                                                                            (hipStream_t)stream);
  });
}

int shw_emd_backward(const float* x, const float* y, const void* workspace, const float* w, int pairs, int n, int kind,
                     float p, float* grad_x, float* grad_y, void* stream) {
  if (!x || !y || !workspace || !w || !grad_x || !grad_y) return (int)hipErrorInvalidValue;
  if (!shw::emd_sizes_ok(pairs, n, kind, p)) return (int)hipErrorInvalidValue;
  if (pairs == 0) return 0;
  const shw::EmdWorkspace W = shw::emd_workspace(const_cast<void*>(workspace), pairs, n);
  return shw::emd_with_kind(kind, p, [&](auto K, auto PM) {
    return shw::emd_launch_backward<decltype(K)::value, decltype(PM)::value>(x, y, W, w, pairs, n, p, grad_x, grad_y,
                                                                             (hipStream_t)stream);
  });
}

}  // extern "C"
