// emd_common.hpp -- what the two exact-W units share: shw_emd.hip (equal sizes: sources and targets) and
// shw_emd_units.hip (n != m: units of mass and slots).  The cost of a couple, its fixed-point form, the (least, second
// least) summary of a bidder, and the constants of the auction rule.  Device code only, apart from the kind / p dispatch
// at the end.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace shw {

constexpr int kEmdMaxPoints = 2048;
constexpr int kEmdThreads = 512;
constexpr int kEmdWaves = kEmdThreads / 64;
constexpr int kEmdFracBits = 26;                       // integer costs lie in [0, 2^26]
constexpr long long kEmdEpsFirst = 1ll << 24;          // 2^26 / 4
constexpr int kEmdEpsShift = 3;                        // eps is divided by 8 from phase to phase: 9 phases
constexpr int kEmdIdBits = 12;                         // low bits of a bid word: 4095 - bidder
constexpr long long kEmdPriceCap = 1ll << 50;          // a price that reaches this gives the pair up (never seen)

// C(a, b).  KIND 0: sum_d |a_d - b_d|^p (cos_cost_matrix; L_p^p despite the name).  KIND 1: angle(a, b)^p with the angle
// from atan2(|a x b|, a . b) -- acos of the normalised dot product loses half the mantissa near 0, where registered
// clouds sit -- and pi / 2 for a zero-length point (what the reference's clamped cosine_similarity gives).
// PM: 2 -> p == 2, 1 -> p == 1, 0 -> powf.  Every product that could be contracted is written as the FMA it becomes
// (or, in emd_cross, kept from becoming one).
// a x b with both products of a component rounded before the subtraction: an FMA would keep one product exact, and
// a x a would come out as that product's rounding error instead of 0 (a cloud matched to its own copy must cost 0.0)
__device__ __forceinline__ void emd_cross(float ax, float ay, float az, float bx, float by, float bz, float& cx, float& cy,
                                          float& cz) {
#pragma clang fp contract(off)
  cx = ay * bz - az * by;
  cy = az * bx - ax * bz;
  cz = ax * by - ay * bx;
}

template <int KIND, int PM>
__device__ __forceinline__ float emd_cost(float ax, float ay, float az, float bx, float by, float bz, float p) {
  if constexpr (KIND == 0) {
    const float dx = fabsf(ax - bx), dy = fabsf(ay - by), dz = fabsf(az - bz);
    if constexpr (PM == 2) return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    else if constexpr (PM == 1) return (dx + dy) + dz;
    else return (powf(dx, p) + powf(dy, p)) + powf(dz, p);
  } else {
    float cx, cy, cz;
    emd_cross(ax, ay, az, bx, by, bz, cx, cy, cz);
    const float s = sqrtf(fmaf(cz, cz, fmaf(cy, cy, cx * cx)));
    const float c = fmaf(az, bz, fmaf(ay, by, ax * bx));
    const float na = fmaf(az, az, fmaf(ay, ay, ax * ax)), nb = fmaf(bz, bz, fmaf(by, by, bx * bx));
    const float th = (na == 0.f || nb == 0.f) ? 1.57079632679489662f : atan2f(s, c);
    if constexpr (PM == 2) return th * th;
    else if constexpr (PM == 1) return th;
    else return powf(th, p);
  }
}

// the integer cost: floor(C scale), scale = 2^26 / K a power of two (the product is exact); NaN and anything outside
// [0, 2^26] are clamped so that no input can leave the integer range
template <int KIND, int PM>
__device__ __forceinline__ long long emd_cost_fixed(float ax, float ay, float az, float bx, float by, float bz, float p,
                                                    float scale) {
  const float t = floorf(emd_cost<KIND, PM>(ax, ay, az, bx, by, bz, p) * scale);
  return (long long)(int)fminf(fmaxf(t, 0.f), 67108864.f);
}

// least and second least of c + price over a lane's targets, with the target of the least (first one among equals)
struct EmdBest {
  long long m1, m2;
  int a1;
  __device__ __forceinline__ void take(long long w, int j) {
    const bool lt = w < m1;
    const long long hi = lt ? m1 : w;           // the larger of (w, m1) is the candidate for second place
    m2 = hi < m2 ? hi : m2;
    m1 = lt ? w : m1;
    a1 = lt ? j : a1;
  }
  // joins the summary (o1, o2, oa) of a disjoint set of targets
  __device__ __forceinline__ void merge(long long o1, long long o2, int oa) {
    const bool other = o1 < m1 || (o1 == m1 && oa < a1);      // equal values: the lowest target leads
    const long long second = other ? m1 : o1;                 // the loser of the two leaders
    const long long rest = o2 < m2 ? o2 : m2;
    m2 = second < rest ? second : rest;
    m1 = other ? o1 : m1;
    a1 = other ? oa : a1;
  }
};

// kind and the form of p to the template instantiation
template <class F>
inline int emd_with_kind(int kind, float p, F f) {
  const int pm = p == 2.f ? 2 : (p == 1.f ? 1 : 0);
  if (kind == 0) {
    if (pm == 2) return f(std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{});
    if (pm == 1) return f(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
    return f(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
  }
  if (pm == 2) return f(std::integral_constant<int, 1>{}, std::integral_constant<int, 2>{});
  if (pm == 1) return f(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{});
  return f(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{});
}

}  // namespace shw
