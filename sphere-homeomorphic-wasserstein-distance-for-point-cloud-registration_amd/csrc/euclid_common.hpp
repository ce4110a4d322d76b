// euclid_common.hpp -- what the Euclidean sliced-W units (shw_esw.hip, shw_esw_dim.hip, shw_gsw.hip, shw_line_ot.hip)
// share: the key loaders, the sort step, the forward body of the equal-size kernels, and the host steps from a call's
// sizes to a template instantiation.
//
// The three equal-size forward kernels are one body, euclid_forward: one wavefront per row (or (pair, slice)); 64 * EPT key
// slots, EPT = 1 .. 64 (up to 4096 points); +inf padding keys; the second operand's sorted keys (and indices) parked in
// LDS while the first sorts; the sorted difference with coefficient rows.  A key policy says what differs:
//   row_t                   the type of a row index: int where rows are (pair, slice) of int counts, long for caller's rows
//   begin_row(s)            per-row state (the direction row, the pair's clouds) before the two loads
//   load<EPT>(which, ...)   the keys of operand `which` (0: the second operand, sorted first and parked)
//   coef<NEG>(g, key)       what is stored as the coefficient of a key with derivative g (NEG: -g, the second operand).
//                           The policy forms the negation itself, `-g / key` as one expression: handed in as an argument
//                           the division expands differently (2189 of 32141 lines of the 64-key circular kernel's
//                           assembly); formed here, that kernel's operations are the parent's
//   kRolledGeneralP         general p walks one rolled loop over both operands in LDS (twice the LDS) instead of the
//                           unrolled register epilogue
#pragma once
#include <type_traits>

#include "dispatch.hpp"
#include "ssw_common.hpp"

namespace shw {

constexpr int kMaxEuclidDim = 64;
constexpr int kMaxEuclidPoints = 4096;

// ---------------------------------------------------------------------------------------------
// key loaders
// ---------------------------------------------------------------------------------------------
// projections of one cloud on one direction of R^3; padding keys are +inf
template <int EPT>
__device__ __forceinline__ void load_projections(const float* __restrict__ X, int count, int lane,
                                                 float tx, float ty, float tz, float (&key)[EPT]) {
  constexpr int CH = EPT < 8 ? EPT : 8;
#pragma unroll
  for (int r0 = 0; r0 < EPT; r0 += CH) {
    float px[CH], py[CH], pz[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int i = min((r0 + j) * kWave + lane, count - 1);
      px[j] = X[3 * i]; py[j] = X[3 * i + 1]; pz[j] = X[3 * i + 2];
    }
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int i = (r0 + j) * kWave + lane;
      const float d = fmaf(pz[j], tz, fmaf(py[j], ty, px[j] * tx));
      key[r0 + j] = (i < count) ? d : __builtin_inff();
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// projections of one cloud (count, dim) on the wave-uniform direction row T (scalar loads); padding keys are +inf.
// Chunks of CH points x DG coordinates: the CH*DG loads of a chunk are in flight together (the R^3 loader's 8 x 3),
// then the FMAs run in coordinate order, so key = x0*t0, then fma(x_d, t_d, key) for d = 1..dim-1.  Coordinates past
// dim re-read the last one and are not used.  The equal-size kernel and the line transport both load through here, so
// they form bit-identical keys.
template <int EPT>
__device__ __forceinline__ void load_projections_dim(const float* __restrict__ X, int count, int dim, int lane,
                                                     const float* __restrict__ T, float (&key)[EPT]) {
  constexpr int CH = EPT < 8 ? EPT : 8;
  constexpr int DG = 4;
#pragma unroll
  for (int r0 = 0; r0 < EPT; r0 += CH) {
    int off[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) off[j] = min((r0 + j) * kWave + lane, count - 1) * dim;
#pragma nounroll
    for (int d0 = 0; d0 < dim; d0 += DG) {
      float xv[CH][DG];
#pragma unroll
      for (int j = 0; j < CH; ++j)
#pragma unroll
        for (int k = 0; k < DG; ++k) xv[j][k] = X[off[j] + min(d0 + k, dim - 1)];
#pragma unroll
      for (int k = 0; k < DG; ++k) {
        const int d = d0 + k;
        if (d < dim) {
          const float t = T[d];
#pragma unroll
          for (int j = 0; j < CH; ++j) key[r0 + j] = (d == 0) ? xv[j][k] * t : fmaf(xv[j][k], t, key[r0 + j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < CH; ++j)
      if ((r0 + j) * kWave + lane >= count) key[r0 + j] = __builtin_inff();
    __builtin_amdgcn_sched_barrier(0);
  }
}

// keys of one row of `count` caller-computed values; padding keys are +inf
template <int EPT>
__device__ __forceinline__ void load_row_keys(const float* __restrict__ U, int count, int lane, float (&key)[EPT]) {
#pragma unroll
  for (int j = 0; j < EPT; ++j) {
    const int i = j * kWave + lane;
    const float v = U[min(i, count - 1)];
    key[j] = i < count ? v : __builtin_inff();
  }
}

// r * theta[d] rounded on its own (the notebook forms theta * r first), never contracted into the subtraction
__device__ __forceinline__ float scaled_theta(float r, float t) { return __fmul_rn(r, t); }

// circular keys of one cloud (count, dim) against the wave-uniform row T (scalar loads).  Chunks of CH points x DG
// coordinates in flight together, as the D-generic projection loader; coordinates past dim re-read the last one and are
// not used.  key = e0*e0, then fma(e_d, e_d, key) for d = 1..dim-1, e_d = x_d - (r t_d); then the square root.
// (T carries no __restrict__: called through a key policy, with it the 16- and 32-key circular kernels take 21 and 34 more
// VGPRs and lose a wave per SIMD -- profiles/r29_euclid_refactor.txt.)
template <int EPT>
__device__ __forceinline__ void load_circular_keys(const float* __restrict__ X, int count, int dim, int lane,
                                                   const float* T, float r, float (&key)[EPT]) {
  constexpr int CH = EPT < 8 ? EPT : 8;
  constexpr int DG = 4;
#pragma unroll
  for (int r0 = 0; r0 < EPT; r0 += CH) {
    int off[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) off[j] = min((r0 + j) * kWave + lane, count - 1) * dim;
#pragma nounroll
    for (int d0 = 0; d0 < dim; d0 += DG) {
      float xv[CH][DG];
#pragma unroll
      for (int j = 0; j < CH; ++j)
#pragma unroll
        for (int k = 0; k < DG; ++k) xv[j][k] = X[off[j] + min(d0 + k, dim - 1)];
#pragma unroll
      for (int k = 0; k < DG; ++k) {
        const int d = d0 + k;
        if (d < dim) {
          const float t = scaled_theta(r, T[d]);
#pragma unroll
          for (int j = 0; j < CH; ++j) {
            const float e = xv[j][k] - t;
            key[r0 + j] = (d == 0) ? e * e : fmaf(e, e, key[r0 + j]);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < CH; ++j)
      key[r0 + j] = ((r0 + j) * kWave + lane >= count) ? __builtin_inff() : sqrtf(key[r0 + j]);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ---------------------------------------------------------------------------------------------
// the sort step
// ---------------------------------------------------------------------------------------------
// keys (slot r * 64 + lane) -> sorted keys (position lane * E + r).  IDX: with the slot each came from, as (orderable
// key, index) items; without, bare keys are sorted and idx is left alone.
template <int E, bool IDX>
__device__ __forceinline__ void sort_keys(float (&key)[E], int (&idx)[E], int lane) {
  if constexpr (IDX) {
    item_t item[E];
#pragma unroll
    for (int r = 0; r < E; ++r) item[r] = make_item(orderable(key[r]), r * kWave + lane);
    wave_sort_kv<E>(item, lane);
#pragma unroll
    for (int r = 0; r < E; ++r) {
      key[r] = from_orderable(item_key(item[r]));
      idx[r] = item_idx(item[r]);
    }
  } else {
    wave_sort<E>(key, lane);
  }
}

// ---------------------------------------------------------------------------------------------
// the forward body of the equal-size kernels
// ---------------------------------------------------------------------------------------------
// dynamic LDS floats of one wave: the parked operand (keys; with GRAD their indices), twice for the rolled general-p form
template <int EPT, int PMODE, bool GRAD, bool ROLLED>
constexpr int euclid_forward_wave_floats() {
  return ((ROLLED && PMODE != 2) ? 2 : 1) * (GRAD ? 2 : 1) * EPT * kWave;
}

template <int EPT, int WAVES, int PMODE, bool GRAD, class Key>
__device__ __forceinline__ void euclid_forward(Key K, typename Key::row_t rows, int n, int num_groups, float p,
                                               int p_int, float* sums, float* coef_a, float* coef_b) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int ROW = EPT * kWave;
  constexpr bool kRolled = Key::kRolledGeneralP && PMODE != 2;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* vbuf = lds + wave * euclid_forward_wave_floats<EPT, PMODE, GRAD, Key::kRolledGeneralP>();
  int* vidx = reinterpret_cast<int*>(vbuf + ROW);            // GRAD only

  const int vid = xcd_contiguous_id(blockIdx.x, num_groups);
  const typename Key::row_t s = (typename Key::row_t)vid * WAVES + wave;
  if (s >= rows) return;
  K.begin_row(s, n);

  float u[EPT];
  int uidx[EPT];
  bool nan_row = false;
#pragma nounroll
  for (int which = 0; which < 2; ++which) {                  // one copy of the sort serves both operands
    int ln = lane;
    asm volatile("" : "+v"(ln));
    K.template load<EPT>(which, s, n, ln, u);
    sort_keys<EPT, GRAD>(u, uidx, ln);
    // A row that holds a NaN key sums to NaN: a positive NaN sorts behind the pads, past position n, where nothing is
    // summed (a negative one sorts first and is summed like any key), so the flag is taken here, from the largest key
    // of each operand -- the last one of lane 63 -- and not in the epilogue, whose registers it would keep alive.  With
    // coefficient rows only: the (key, index) sort orders a NaN as the largest key, whereas a value-only call sorts bare
    // floats with min / max, which do not keep a NaN -- what such a call sums for a row with a NaN key is unspecified,
    // as it was, and its kernels carry no check.
    if constexpr (GRAD) nan_row |= __builtin_isnan(u[EPT - 1]);
    if (which == 0) {
#pragma unroll
      for (int r = 0; r < EPT; ++r) {
        vbuf[r * kWave + lane] = u[r];
        if constexpr (GRAD) vidx[r * kWave + lane] = uidx[r];
      }
    }
  }
  __builtin_amdgcn_wave_barrier();

  float acc = 0.f;
  float* ca = GRAD ? coef_a + (long)s * n : nullptr;
  float* cb = GRAD ? coef_b + (long)s * n : nullptr;
  // one sorted position: e = lane * EPT + r, the other operand's e sits in the same slot
  auto term = [&](int r, float uu, float v, int ia, int ib) {
    const float d = uu - v;
    if (lane * EPT + r < n) {
      acc += pow_abs<PMODE>(d, p, p_int);
      if constexpr (GRAD) {
        const float g = dpow_abs<PMODE>(d, p, p_int);
        // the one store site.  A NaN key orders after the +inf pads and would put a pad's index (>= n) here: such a
        // row stores nothing past its n coefficients, and its sum is NaN.
        if (ia < n) ca[ia] = Key::template coef<false>(g, uu);
        if (ib < n) cb[ib] = Key::template coef<true>(g, v);
      }
    }
  };
  if constexpr (!kRolled) {
#pragma unroll
    for (int r = 0; r < EPT; ++r)
      term(r, u[r], vbuf[r * kWave + lane], GRAD ? uidx[r] : 0, GRAD ? vidx[r * kWave + lane] : 0);
  } else {
    // general p: |d|^p is a loop or powf per key; unrolled EPT = 64 times it spills.  The sorted first operand goes to
    // LDS as well and one rolled loop walks both.
    float* ubuf = vbuf + (GRAD ? 2 : 1) * ROW;
    int* uixb = reinterpret_cast<int*>(ubuf + ROW);          // GRAD only
#pragma unroll
    for (int r = 0; r < EPT; ++r) {
      ubuf[r * kWave + lane] = u[r];
      if constexpr (GRAD) uixb[r * kWave + lane] = uidx[r];
    }
    __builtin_amdgcn_wave_barrier();
#pragma nounroll
    for (int r = 0; r < EPT; ++r)
      term(r, ubuf[r * kWave + lane], vbuf[r * kWave + lane], GRAD ? uixb[r * kWave + lane] : 0,
           GRAD ? vidx[r * kWave + lane] : 0);
  }
  // ... and its sum is NaN (nan_row, taken from the sorted keys above).
  if constexpr (GRAD) {
    if (lane == kWave - 1 && nan_row) acc = __builtin_nanf("");
  }
  acc = wave_sum(acc, lane);
  if (lane == 0) sums[s] = acc;
}

// ---------------------------------------------------------------------------------------------
// host: from a call's sizes to a template instantiation (in the style of with_pmode / with_full, dispatch.hpp)
// ---------------------------------------------------------------------------------------------
// one check for "(pairs, n[, m], dim, slices, theta stride)": max_pairs is 65535 where the pairs are a grid's y
inline bool euclid_sizes_ok(long max_pairs, int pairs, int n, int m, int dim, int slices, long theta_pair_stride) {
  if (dim < 1 || dim > kMaxEuclidDim) return false;
  if (n < 1 || n > kMaxEuclidPoints || m < 1 || m > kMaxEuclidPoints) return false;
  if (pairs < 0 || pairs > max_pairs || slices < 0) return false;
  if (theta_pair_stride != 0 && theta_pair_stride < (long)slices * dim) return false;
  return true;
}
constexpr long kAnyPairs = 0x7fffffffL, kGridYPairs = 65535;

template <int V> using int_c = std::integral_constant<int, V>;

// size class -> <EPT, WAVES>: f(int_c<EPT>, int_c<WAVES>) returns the launch's code
template <class F>
inline int with_ept_waves(int ept, F f) {
  switch (ept) {
    case 1: return f(int_c<1>{}, int_c<4>{});
    case 2: return f(int_c<2>{}, int_c<4>{});
    case 4: return f(int_c<4>{}, int_c<4>{});
    case 8: return f(int_c<8>{}, int_c<4>{});
    case 16: return f(int_c<16>{}, int_c<4>{});
    case 32: return f(int_c<32>{}, int_c<2>{});
    case 64: return f(int_c<64>{}, int_c<1>{});
    default: return (int)hipErrorInvalidValue;
  }
}

// PMODE x GRAD: f(int_c<PMODE>, bool constant)
template <class F>
inline void with_pmode_grad(int p_int, bool grad, F f) {
  with_pmode(p_int, [&](auto pm) {
    if (grad) f(pm, std::true_type{});
    else f(pm, std::false_type{});
  });
}

// coordinates per workgroup of the gradient kernels: 4, 8, or 16 with the rest of dim split over the grid's z:
// f(int_c<DC>, grid z)
template <class F>
inline void with_coord_chunk(int dim, F f) {
  if (dim <= 4) f(int_c<4>{}, 1u);
  else if (dim <= 8) f(int_c<8>{}, 1u);
  else f(int_c<16>{}, (unsigned)(dim + 15) / 16);
}

// The points gradient of the D-generic projections, n source and m target points (the equal-size entry passes m = n):
// defined in shw_line_ot.hip, the one unit that instantiates line_esw_backward_points_kernel<DC>.
int launch_line_esw_backward_points(const float* thetas, const float* coef_s, const float* coef_t, const float* slice_w,
                                    int pairs, int n, int m, int dim, int slices, long theta_pair_stride, float* grad_xs,
                                    float* grad_xt, hipStream_t stream);

// The forward launch of a unit whose kernel wraps euclid_forward: `rows` rows in workgroups of WAVES, the class's LDS,
// then launch(int_c<EPT>, int_c<WAVES>, int_c<PMODE>, bool constant GRAD, grid, block, lds bytes).
template <bool ROLLED, class Launch>
inline int launch_euclid_forward(long rows, int n, int p_int, bool grad, int& num_groups, Launch launch) {
  return with_ept_waves(ept_for(n, n), [&](auto ept, auto waves) {
    constexpr int EPT = decltype(ept)::value, WAVES = decltype(waves)::value;
    const long groups = (rows + WAVES - 1) / WAVES;
    if (groups > 0x7fffffffL) return (int)hipErrorInvalidValue;
    num_groups = (int)groups;
    with_pmode_grad(p_int, grad, [&](auto pm, auto g) {
      constexpr int floats = euclid_forward_wave_floats<EPT, decltype(pm)::value, decltype(g)::value, ROLLED>();
      launch(ept, waves, pm, g, dim3((unsigned)groups), dim3(WAVES * 64), (size_t)WAVES * floats * sizeof(float));
    });
    return (int)hipGetLastError();
  });
}

}  // namespace shw
