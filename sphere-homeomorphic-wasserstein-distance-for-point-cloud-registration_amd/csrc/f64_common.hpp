// f64_common.hpp -- device helpers shared by the two float64 units (shw_ssw_f64.hip: equal sizes, uniform weights;
// shw_ssw_f64_general.hip: weighted and unequal-size clouds): the fixed-order reductions, |d|^p and its derivative, the
// circle coordinate, the binary searches, and the project-and-sort stage of one cloud.  Nothing here is shared with the
// float32 units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace shw {
namespace f64 {

constexpr int kMaxWaves = 16;
constexpr unsigned kBinLimit = 24;   // more atoms than this in one bin: the cloud is sorted by the network

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s, 64);   // butterfly: the same bits in every lane
  return v;
}

// Sum of three per-thread values over the workgroup, the same bits in every thread.  `red` holds two sets of
// 3 x kMaxWaves partials used in turn, so one barrier per call is enough: a thread can only be one call ahead of
// the slowest reader.
__device__ __forceinline__ void block_sum3(double& a, double& b, double& c, double* red, int& turn, int nwaves) {
  a = wave_sum_d(a); b = wave_sum_d(b); c = wave_sum_d(c);
  double* r = red + turn * 3 * kMaxWaves;
  turn ^= 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { r[wave] = a; r[kMaxWaves + wave] = b; r[2 * kMaxWaves + wave] = c; }
  __syncthreads();
  a = r[0]; b = r[kMaxWaves]; c = r[2 * kMaxWaves];
  for (int w = 1; w < nwaves; ++w) { a += r[w]; b += r[kMaxWaves + w]; c += r[2 * kMaxWaves + w]; }
}

__device__ __forceinline__ double pow_abs(double d, double p, int p_int) {
  const double a = fabs(d);
  if (p_int == 2) return d * d;
  if (p_int > 0) {
    double r = a;
    for (int i = 1; i < p_int; ++i) r *= a;
    return r;
  }
  return pow(a, p);
}

// d/dD |D|^p (0 at D = 0, as the float32 kernels)
__device__ __forceinline__ double dpow_abs(double d, double p, int p_int) {
  const double a = fabs(d);
  if (!(a > 0.0)) return 0.0;
  double r;
  if (p_int > 0) {
    r = 1.0;
    for (int i = 1; i < p_int; ++i) r *= a;
  } else {
    r = pow(a, p - 1.0);
  }
  return copysign(p * r, d);
}

__device__ __forceinline__ double circle_coord(double a, double b) {
  const double kPi = 3.141592653589793, kTwoPi = 6.283185307179586;
  return (atan2(-b, -a) + kPi) / kTwoPi;
}

// number of keys < val (STRICT) or <= val among the first n of the ascending array
template <bool STRICT>
__device__ __forceinline__ int count_below(const double* buf, int n, double val) {
  int lo = 0, hi = n;                  // answer in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const double probe = buf[mid];
    const bool go = STRICT ? (probe < val) : (probe <= val);
    if (go) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Bin of a coordinate among P equal bins of [0, 1] (P a power of two: the scaling is exact, the map monotone); anything
// outside, which only rows of coordinates from a caller can hold, goes to the first or last bin.
__device__ __forceinline__ int bin_of(double c, int P) {
  const int bin = (int)(c * (double)P);
  return max(0, min(P - 1, bin));
}

// Bitonic network over (coordinate, index) in LDS, all T threads; ends with a barrier.
__device__ __forceinline__ void bitonic_sort(double* key, uint16_t* idx, int P, int t, int T) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int c = t; c < (P >> 1); c += T) {
        const int i = ((c & ~(j - 1)) << 1) | (c & (j - 1));
        const int h = i | j;
        const double ka = key[i], kb = key[h];
        const uint16_t ia = idx[i], ib = idx[h];
        const bool gt = (ka > kb) || (ka == kb && ia > ib);
        const bool up = (i & k) == 0;
        if (gt == up) {
          key[i] = kb; key[h] = ka;
          idx[i] = ib; idx[h] = ia;
        }
      }
      __syncthreads();
    }
  }
}

// Project-and-sort stage of ONE cloud, all T threads of the workgroup: circle coordinates of the n atoms at X (points
// projected on the frame U when `projected`, else rows of coordinates), sorted into dst[0, P) in the total order
// (ascending coordinate, ties by original index) with the original index of every sorted position in dsti; positions
// n..P-1 hold +inf pads.  P >= n is a power of two.  A distribution sort over P equal bins of [0, 1] (count with integer
// LDS counters, scan, scatter, every bin put in order by insertion -- the result is the total order whatever order the
// counters served the atoms in); a cloud with more than kBinLimit atoms in one bin takes the bitonic network instead.
// tmp (P doubles) and hist (P counters) are scratch, wsum holds kMaxWaves scan totals, *flag must be 0 on entry.
// Returns this thread's partial sum of the coordinates; ends with a barrier.
__device__ __forceinline__ double project_and_sort(const double* X, int n, int P, const double (&U)[6], bool projected,
                                                   double* dst, uint16_t* dsti, double* tmp, unsigned* hist,
                                                   unsigned* wsum, unsigned* flag, int t, int T) {
  for (int bin = t; bin < P; bin += T) hist[bin] = 0;
  __syncthreads();
  double acc = 0.0;
  for (int e = t; e < n; e += T) {
    double c;
    if (projected) {
      const double px = X[3 * e], py = X[3 * e + 1], pz = X[3 * e + 2];
      const double a = fma(pz, U[4], fma(py, U[2], fma(px, U[0], 0.0)));
      const double bb = fma(pz, U[5], fma(py, U[3], fma(px, U[1], 0.0)));
      c = circle_coord(a, bb);
    } else {
      c = X[e] + 0.0;                                   // -0 -> +0
    }
    acc += c;
    tmp[e] = c;
    atomicAdd(&hist[bin_of(c, P)], 1u);
  }
  __syncthreads();
  // exclusive scan of the bin counts: thread t owns bins [t per, (t + 1) per)
  {
    const int per = (P + T - 1) / T, first = t * per;
    unsigned local = 0;
    for (int j = 0; j < per; ++j) {
      const unsigned c = (first + j < P) ? hist[first + j] : 0u;
      local += c;
      if (c > kBinLimit) *flag = 1;                     // a crowded bin: this cloud takes the network instead
    }
    unsigned incl = local;
#pragma unroll
    for (int sft = 1; sft < 64; sft <<= 1) {
      const unsigned up = __shfl_up(incl, sft, 64);
      if ((t & 63) >= sft) incl += up;
    }
    if ((t & 63) == 63) wsum[t >> 6] = incl;
    __syncthreads();
    unsigned run = incl - local;
    for (int w = 0; w < (t >> 6); ++w) run += wsum[w];
    for (int j = 0; j < per; ++j) {
      if (first + j < P) {
        const unsigned c = hist[first + j];
        hist[first + j] = run;
        run += c;
      }
    }
  }
  __syncthreads();
  const bool network = *flag != 0;                      // the same in every thread
  if (!network) {
    // scatter to the bins (the order inside a bin is whatever the counters gave), pads behind
    for (int e = t; e < P; e += T) {
      if (e < n) {
        const double c = tmp[e];
        const unsigned pos = atomicAdd(&hist[bin_of(c, P)], 1u);
        dst[pos] = c;
        dsti[pos] = (uint16_t)e;
      } else {
        dst[e] = __builtin_inf();
        dsti[e] = (uint16_t)e;
      }
    }
    __syncthreads();
    // every bin into the total order (coordinate, index) by insertion: hist[bin] now is the bin's end
    for (int bin = t; bin < P; bin += T) {
      const int start = bin ? (int)hist[bin - 1] : 0, end = (int)hist[bin];
      for (int i = start + 1; i < end; ++i) {
        const double k = dst[i];
        const uint16_t ki = dsti[i];
        int j = i - 1;
        while (j >= start && (dst[j] > k || (dst[j] == k && dsti[j] > ki))) {
          dst[j + 1] = dst[j];
          dsti[j + 1] = dsti[j];
          --j;
        }
        dst[j + 1] = k;
        dsti[j + 1] = ki;
      }
    }
  } else {
    for (int e = t; e < P; e += T) {
      dst[e] = (e < n) ? tmp[e] : __builtin_inf();
      dsti[e] = (uint16_t)e;
    }
    __syncthreads();
    bitonic_sort(dst, dsti, P, t, T);
  }
  __syncthreads();
  return acc;
}

// p as a small integer (1..8), else 0: selects the multiply chains of pow_abs / dpow_abs
inline int small_integer_power(double p) {
  for (int k = 1; k <= 8; ++k)
    if (p == (double)k) return k;
  return 0;
}

}  // namespace f64
}  // namespace shw
