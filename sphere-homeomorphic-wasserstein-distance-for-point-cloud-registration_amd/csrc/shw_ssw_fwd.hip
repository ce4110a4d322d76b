// shw_ssw_fwd.hip -- loss-only kernel for p != 1 (key-only register sort).  See ssw_common.hpp.
#include "ssw_common.hpp"
#include "coop_sort.hpp"

#ifndef SHW_BINSORT
#define SHW_BINSORT 1      // 1: distribution sort through LDS (bin_sort.hpp) for >= 8 keys per lane; 0: bitonic network only
#endif
#ifndef SHW_FWD_MINW
#define SHW_FWD_MINW 3     // waves per SIMD asked of the register allocator at 2048 points (bin sort)
#endif
#ifndef SHW_BINSORT_NB_PER_EPT
#define SHW_BINSORT_NB_PER_EPT 32   // bins = this * keys-per-lane (32: two keys per bin on average)
#endif
#ifndef SHW_FWD_WAVES
#define SHW_FWD_WAVES 1    // wavefronts per workgroup of the one-wave-per-slice kernel
#endif

namespace shw {

// register budget: the LDS footprint (EPT*256 B per wave) admits 20 waves per CU at EPT = 32, so
// ask the allocator for 5 waves per SIMD there (<= 96 VGPRs); larger EPT take what they need.
// The general-power variant (powf) is left at 4.  At EPT = 64 the unconstrained allocator takes all 256
// registers (1 wave per SIMD); asked for 3 waves it needs 144 with no spill, which is what 16 KB of LDS per
// wave can use.
constexpr int min_waves_per_simd(int ept, int pmode) {
  return ept <= 16 ? (pmode == 2 ? 6 : 4) : (ept == 32 ? (pmode == 2 ? 5 : 3) : (ept == 64 ? 3 : 1));
}

constexpr bool forward_uses_bins(int ept) { return SHW_BINSORT != 0 && ept >= 8; }
// LDS floats per wave: the sorted target row (64*EPT) and, with the bin sort, its 32*EPT counters in front of it
constexpr int forward_lds_floats(int ept) { return forward_uses_bins(ept) ? (64 + SHW_BINSORT_NB_PER_EPT) * ept : 64 * ept; }
#ifndef SHW_FWD_MINW_PARTIAL
#define SHW_FWD_MINW_PARTIAL 2     // clouds that do not fill the size class: 2 waves per SIMD, no spills (measured 0.371 -> 0.307 ms at N=2000)
#endif
constexpr int forward_min_waves(int ept, int pmode, bool full = true) {
  if (forward_uses_bins(ept) && ept == 32 && !full) return SHW_FWD_MINW_PARTIAL;
  // bin sort: 12 KB of LDS per wave at EPT = 32 -> 13 waves per CU: ask the register allocator for 3 per SIMD
  return forward_uses_bins(ept) ? (ept == 32 ? SHW_FWD_MINW : (ept == 16 ? 5 : 6)) : min_waves_per_simd(ept, pmode);
}

// FULL: n == m == 64*EPT (no padding atoms): mask-free projection and the fast shift evaluation.
template <int EPT, int WAVES, int PMODE, bool FULL>
__global__ __launch_bounds__(WAVES * 64, forward_min_waves(EPT, PMODE, FULL)) void ssw_forward_kernel(SswArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr bool BINS = forward_uses_bins(EPT);
  constexpr bool GROUPED = shift_fetch_grouped(EPT, WAVES, PMODE, FULL);       // sorted target in groups of four rows
  const int lane = threadIdx.x & 63;
  // (one wave per workgroup: a literal 0 makes the LDS addresses of the sort constants -- the counter of a key is then
  //  ds_add(off) with no base to add)
  const int wave = WAVES == 1 ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* scratch = lds + wave * forward_lds_floats(EPT);
  float* vbuf = BINS ? scratch + SHW_BINSORT_NB_PER_EPT * EPT : scratch;       // the staging buffer of the sort becomes the target row

  const int vid = xcd_contiguous_id(blockIdx.x, A.num_groups);
  const int s = vid * WAVES + wave;
  if (s >= A.pairs * A.slices) return;            // wave-uniform
  const int b = s / A.slices, l = s - b * A.slices;

  float U[6];
  load_frame(A.dirs, (long)b * A.u_pair_stride + (long)l * 6, U);   // (3,2) row-major: U[2*d + k]

  float key[EPT], u[EPT];
  float sum_v = 0.f, sum_u = 0.f;
  // The full 32-keys-per-lane class takes the rolling loader (ssw_common.hpp): sub-chunks of 8 rows, the next one in
  // flight while one is computed, and the first one of each cloud issued ahead of the loader -- the source's here, beside
  // the frame (the addresses do not depend on it), the target's before the source's sort.  `pre` passes from the
  // source's pass to the target's (through the `which` loop where it is one: PMODE 0, whose code is emitted once; 168
  // VGPRs, 3 waves per SIMD, no spill).
  constexpr bool ROLL = EPT == 32 && FULL;
  constexpr int SUB = 8;
  PointChunk<SUB> pre;
#ifndef SHW_ABL_NO_COORDS
  if constexpr (ROLL) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
    if (A.dirs) issue_points<SUB>(A.xs + (long)b * A.n * A.pstride, ln, 0, pre);
  }
#endif
#ifdef SHW_DBG_RUNLEN
  int dbg_run = 0;
#endif
  // TWO_PASS: the headline class runs the source's pass and the target's as straight-line code, one behind the other
  // (the loop below unrolled by two).  The source's fix-up then leaves its keys in the registers the solve reads as u[]
  // (inside the loop the sort is emitted once, and the sorted source has to leave the registers the target's sort reuses:
  // 32 v_mov_b32), the target's feeds write_grouped_rows directly, and the fix-up can run its odd phases first
  // (bin_sort.hpp, REM_FIRST).  138 VGPRs instead of 168, no spill; the kernel's text grows from 42 268 to 75 312 bytes
  // (8023 -> 13 904 instructions: 3515 of the added ones are the second copy of the network fallback, about 2400 lie on
  // the executed path; profiles/r23_forward_summary.txt).  Every other class keeps the loop: the general-power kernel
  // <32,1,0,true> is 148 KB of text as it is.
  constexpr bool TWO_PASS = ROLL && PMODE == 2;
  // ... and its sort's counters lie under the staging buffer: 64 * 20 = 1280 bins in the same 12 KB (bin_sort.hpp,
  // wave_sort_binned; 0: counters in front of the buffer, 1024 bins, as in every other class).  vbuf and the LDS request do
  // not move.  20 bins per lane of the scan, measured against 12 .. 36 (profiles/r28_forward_summary.txt): a lane stride of
  // 80 B keeps the scan's ds_read_b128 free of bank conflicts; 128 B (32 per lane) does not and costs 27 %.
  constexpr int kAliasBPL = TWO_PASS ? 20 : 0;
  static_assert(64 * kAliasBPL <= forward_lds_floats(EPT), "the counters must fit the wave's LDS block");
  constexpr int kUnroll = TWO_PASS ? 2 : 1;        // 1: not unrolled
#pragma unroll kUnroll
  for (int which = 0; which < 2; ++which) {        // 0: source -> registers, 1: target -> LDS
    const float* X = which == 0 ? A.xs + (long)b * A.n * A.pstride : A.xt + (long)b * A.m * A.pstride;
    const int count = which == 0 ? A.n : A.m;
    // Opaque copy of the lane id: keeps the compiler from hoisting the lane-dependent constants of the sort (and
    // the point offsets) out of this loop and holding them in VGPRs.
    int ln = lane;
    asm volatile("" : "+v"(ln));
#ifdef SHW_ABL_NO_COORDS       // developer ablation: pseudo-random keys instead of load + project + atan2
    float part = 0.f;
#pragma unroll
    for (int r = 0; r < EPT; ++r) {
      unsigned h = (unsigned)(ln * 2654435761u) ^ (unsigned)((r + 33 * which + s) * 40503u);
      h ^= h >> 13; h *= 0x5bd1e995u; h ^= h >> 15;
      key[r] = (float)(h >> 8) * (1.0f / 16777216.0f);
      part += key[r];
    }
#else
    float part;
    if constexpr (ROLL) {
      part = load_coords_rolling<EPT, SUB>(X, ln, U, key, pre);
      // the target's first rows travel while the source is sorted (which == 0 only: never past the pair's target; rows
      // of coordinates, dirs == NULL, issue nothing ahead)
      if (which == 0 && A.dirs) issue_points<SUB>(A.xt + (long)b * A.m * A.pstride, ln, 0, pre);
    } else {
      part = load_coords<EPT, FULL>(X, count, ln, U, key);
    }
#endif
#ifdef SHW_DBG_RUNLEN          // developer build (tools/nonuniform_time.py): slice_shift reports the longest equal-bin run
    if constexpr (BINS) dbg_run = max(dbg_run, wave_sort_binned<EPT, FULL, TWO_PASS, kAliasBPL>(key, ln, count, scratch, A.dirs == nullptr));
    else wave_sort<EPT>(key, ln);
#else
    if constexpr (BINS) wave_sort_binned<EPT, FULL, TWO_PASS, kAliasBPL>(key, ln, count, scratch, A.dirs == nullptr);
    else wave_sort<EPT>(key, ln);
#endif
    if (which == 0) {
      sum_u = wave_sum(part, lane);
#pragma unroll
      for (int r = 0; r < EPT; ++r) u[r] = key[r];
    } else {
      sum_v = wave_sum(part, lane);
      if constexpr (GROUPED) {
        write_grouped_rows<EPT>(vbuf, lane, key);
      } else if constexpr (FULL || !BINS) {
#pragma unroll
        for (int r = 0; r < EPT; ++r) vbuf[r * kWave + lane] = key[r];
      }
    }
  }
  __builtin_amdgcn_wave_barrier();

  float best;
#ifdef SHW_ABL_NO_SOLVE
  best = u[0] + vbuf[lane] + sum_u - sum_v;
  const int k = 0;
#else
  int k;
  if constexpr (FULL || !BINS) {
    k = solve_shift<EPT, PMODE, FULL, true, GROUPED>(u, vbuf, lane, A.n, sum_u, sum_v, A.p, A.p_int, best);
  } else {
    // any n: pre-rotated extended rows over the sort's scratch (counters + staging buffer are dead), target kept in
    // registers for the rare rewrite
    static_assert(ExtRows<EPT>::FLOATS <= forward_lds_floats(EPT), "extended rows must fit the sort's scratch");
    k = solve_shift_ext<EPT, PMODE>(u, key, scratch, lane, A.n, sum_u, sum_v, A.p, A.p_int, best);
  }
#endif
  if (lane == 0) {
    A.slice_cost[s] = best / (float)A.n;
    if (A.slice_shift) A.slice_shift[s] = k;
#ifdef SHW_DBG_RUNLEN
    if (A.slice_shift) A.slice_shift[s] = dbg_run;
#endif
  }
}

// ---------------------------------------------------------------------------------------------
// Multi-wave form for 2048 < n <= 8192: W = 2 or 4 wavefronts of one workgroup share a slice.  Each wave
// sorts its chunk of 2048 keys in registers exactly as above; the chunks are then merged by the remaining
// levels of the same bitonic network (coop_bitonic of coop_sort.hpp, the fallback of the cooperative sorts), whose
// first stages pair elements of DIFFERENT waves: those go through
// one LDS exchange each (write 32 registers, barrier, read the partner wave's slot, barrier), and because the
// "lower / upper" role of such a stage is the same for a whole wave they are plain v_min / v_max.  The stages
// below the wave level are the single-wave code (xlane_stages, lane_stages).  The source is sorted first and
// stays in registers while the target is sorted; the exchange buffer then becomes the sorted target, so LDS
// stays at 8 KB per wave and registers at the 2048-point budget (the one-wave kernels for these sizes need 64
// and 128 keys per lane: 1 wave per SIMD, and spills at 8192).  The shift solve runs in every wave on its own
// 2048 source atoms; the three partial sums are added across waves in wave order through LDS, so all waves
// take identical decisions.
// ---------------------------------------------------------------------------------------------
template <int W, int PMODE, bool FULL>
__global__ __launch_bounds__(W * 64, 4) void ssw_forward_mw_kernel(SswArgs A) {
  constexpr int EPT = 32, NCOL = 64 * W, CHUNK = EPT * kWave;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* buf = lds;                                            // [EPT][NCOL]: exchange buffer, then sorted target
  float* red = lds + EPT * NCOL;                               // [W][4] partial sums
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int s = xcd_contiguous_id(blockIdx.x, A.num_groups);  // one workgroup per (pair, slice)
  const int b = s / A.slices, l = s - b * A.slices;
  const int n = A.n;
  float U[6];
  load_frame(A.dirs, (long)b * A.u_pair_stride + (long)l * 6, U);   // (3,2) row-major: U[2*d + k]

  float u[EPT], key[EPT];
  float part_u = 0.f, part_v = 0.f;
  const int first = wave * CHUNK;                              // first point of this wave's chunk
  const int chunk_live = max(0, min(CHUNK, n - first));
#pragma nounroll
  for (int which = 0; which < 2; ++which) {                    // 0: source -> registers, 1: target -> LDS
    const float* X = (which == 0 ? A.xs : A.xt) + (long)b * n * A.pstride;
    const int base = min(first, n - 1);                        // keep the addresses of an empty chunk in bounds
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const float part = load_coords<EPT, FULL>(X + (long)base * A.pstride, n - base, ln, U, key, chunk_live);
    coop_bitonic<EPT, W>(key, buf, wave, ln);
    if (which == 0) {
      part_u = wave_sum_uniform(part, lane);
#pragma unroll
      for (int r = 0; r < EPT; ++r) u[r] = key[r];
    } else {
      part_v = wave_sum_uniform(part, lane);
#pragma unroll
      for (int r = 0; r < EPT; ++r) buf[r * NCOL + wave * 64 + lane] = key[r];
    }
  }
  if (lane == 0) { red[wave * 4] = part_u; red[wave * 4 + 1] = part_v; }
  __syncthreads();
  float sum_u = 0.f, sum_v = 0.f;
#pragma unroll
  for (int w = 0; w < W; ++w) { sum_u += red[w * 4]; sum_v += red[w * 4 + 1]; }
  __syncthreads();

  // minimise the convex sequence c(k), |k| <= n: solve_shift with the partial sums added across waves
  int lo = -n, hi = n;
  float guess = rintf(sum_u - sum_v);
  guess = fminf(fmaxf(guess, (float)lo), (float)hi);
  int k = __builtin_amdgcn_readfirstlane((int)guess);
  bool lo_tight = false, hi_tight = false;
  int step = 1;
  float cm = 0.f, c0 = 0.f, cp = 0.f;
  const int glane = wave * 64 + lane;
  for (int it = 0; it < 64; ++it) {
    int gl = glane;
    asm volatile("" : "+v"(gl));
    float pm, p0, pp;
    if constexpr (FULL) shift_costs3_full<EPT, PMODE, NCOL>(u, buf, gl, k, A.p, A.p_int, pm, p0, pp);
    else shift_costs3<EPT, PMODE, NCOL>(u, buf, gl, n, k, A.p, A.p_int, pm, p0, pp);
    if (lane == 0) { red[wave * 4] = pm; red[wave * 4 + 1] = p0; red[wave * 4 + 2] = pp; }
    __syncthreads();
    cm = c0 = cp = 0.f;
#pragma unroll
    for (int w = 0; w < W; ++w) { cm += red[w * 4]; c0 += red[w * 4 + 1]; cp += red[w * 4 + 2]; }
    cm = as_f(__builtin_amdgcn_readfirstlane(as_i(cm)));
    c0 = as_f(__builtin_amdgcn_readfirstlane(as_i(c0)));
    cp = as_f(__builtin_amdgcn_readfirstlane(as_i(cp)));
    __syncthreads();
    const bool right = (cp < c0) && (k < hi);
    const bool left = !right && (cm < c0) && (k > lo);
    if (!right && !left) break;
    if (right) {
      lo = k + 1; lo_tight = true;
      if (hi_tight) { k = lo + ((hi - lo) >> 1); } else { k = min(k + step, hi); step <<= 1; }
    } else {
      hi = k - 1; hi_tight = true;
      if (lo_tight) { k = lo + ((hi - lo) >> 1); } else { k = max(k - step, lo); step <<= 1; }
    }
    k = __builtin_amdgcn_readfirstlane(k);
  }
  if (threadIdx.x == 0) {
    A.slice_cost[s] = c0 / (float)n;
    if (A.slice_shift) A.slice_shift[s] = k;
  }
}

template <int W>
static int launch_forward_mw(SswArgs& A, bool full, hipStream_t stream) {
  if (!problem_groups(A.pairs, A.slices, 1, A.num_groups)) return (int)hipErrorInvalidValue;
  const size_t lds = (size_t)(32 * 64 * W + 4 * W) * sizeof(float);
  const dim3 grid((unsigned)A.num_groups), block(W * 64);
  with_pmode(A.p_int, [&](auto pm) { with_full(full, [&](auto fl) {
    hipLaunchKernelGGL((ssw_forward_mw_kernel<W, decltype(pm)::value, decltype(fl)::value>), grid, block, lds, stream, A);
  }); });
  return (int)hipGetLastError();
}

template <int EPT, int WAVES>
static int launch_forward_class(SswArgs& A, bool full, hipStream_t stream) {
  if (!problem_groups(A.pairs, A.slices, WAVES, A.num_groups)) return (int)hipErrorInvalidValue;
  size_t lds = (size_t)WAVES * forward_lds_floats(EPT) * sizeof(float);
#ifdef SHW_DEV_OCCUPANCY_EXPERIMENT   // developer build only: pad the LDS request to lower the waves per CU
  if (const char* extra = getenv("SHW_DEV_EXTRA_LDS")) lds += (size_t)atoi(extra);
#endif
  const dim3 grid((unsigned)A.num_groups), block(WAVES * 64);
  with_pmode(A.p_int, [&](auto pm) { with_full(full, [&](auto fl) {
    hipLaunchKernelGGL((ssw_forward_kernel<EPT, WAVES, decltype(pm)::value, decltype(fl)::value>), grid, block, lds, stream, A);
  }); });
  return (int)hipGetLastError();
}

int launch_forward(SswArgs& A, const Plan& P, hipStream_t stream) {
  switch (P.kpl) {
#ifdef SHW_DEV_ONLY_EPT   // developer switch: compile a single size class quickly
#ifndef SHW_DEV_FWD_WAVES
#define SHW_DEV_FWD_WAVES (SHW_DEV_ONLY_EPT <= 32 ? SHW_FWD_WAVES : (SHW_DEV_ONLY_EPT == 64 ? 2 : 1))
#endif
    case SHW_DEV_ONLY_EPT: return launch_forward_class<SHW_DEV_ONLY_EPT, SHW_DEV_FWD_WAVES>(A, P.full, stream);
#else
    case 1: return launch_forward_class<1, 4>(A, P.full, stream);
    case 2: return launch_forward_class<2, 4>(A, P.full, stream);
    case 4: return launch_forward_class<4, 4>(A, P.full, stream);
    case 8: return launch_forward_class<8, 4>(A, P.full, stream);
    case 16: return launch_forward_class<16, 4>(A, P.full, stream);
    case 32: return launch_forward_class<32, SHW_FWD_WAVES>(A, P.full, stream);
    case 64: return launch_forward_mw<2>(A, P.full, stream);            // 2049..4096 points: two waves per slice
    case 128: return launch_forward_mw<4>(A, P.full, stream);           // 4097..8192 points: four waves per slice
#endif
    default: return (int)hipErrorInvalidValue;
  }
}

}  // namespace shw
