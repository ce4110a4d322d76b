// bin_sort.hpp -- one-pass distribution sort of <= 64*EPT circle coordinates by ONE wavefront (gfx950), through LDS.
//
// Why: on MI355X every v_min/v_max/v_med3/v_cmp (f32 or integer) issues at 1.78 ns per wave-instruction per SIMD,
// add/fma/xor at 1.0 ns (tools/ubench/op_rate.hip, round 2).  The register bitonic network of wave_sort.hpp costs
// 66 stages x 32 keys = 2112 slow-rate instructions + 672 crossbar moves per 2048-key sort, and two of them are
// 70 % of the loss kernel.  Circle coordinates are numbers in [0, 1] -- a key's value says where it belongs:
//
//   1. histogram   off = 4 * bin(key), a monotone map of the key onto the counters that is already the counter's byte
//                  offset (binsort_off: one FMA and one AND);  ds_add(cnt + off, 4)       (NB = 32*EPT bins: 2 keys per
//                                                                                          bin on average)
//   2. scan        exclusive prefix sum over the NB counters (16 per lane in-lane, then a wave scan).  The counters count
//                  BYTES (4 per key), so the scan leaves the byte position of every bin's first key; the largest
//                  counter / 4 = g is the longest run of keys that share a bin
//   3. scatter     buf[perm(ds_add_rtn(cnt + off, 4))] = key   (keys are now ordered by bin; inside a bin in arrival
//                  order).  `off` is NOT recomputed: the compiler keeps the EPT offsets of step 1 in registers across the
//                  scan (registers, not instructions: the loss kernel stays spill-free).  No other per-key word lives
//                  from 1 to 3: the one-wave loss kernel sorts the target while it holds the sorted source in registers,
//                  and a rank per key beside both made it spill.
//   4. read back   32 consecutive positions per lane (sorted position of x[r] in lane `lane` is lane*EPT + r, the
//                  layout wave_sort leaves)
//   5. fix-up      g phases of odd-even transposition (in-lane compare-exchanges + one exchange across each lane
//                  boundary per odd phase): every run of equal-bin keys is at most g long and no key has to leave its
//                  run, so g phases put every run -- hence the whole array -- into exact ascending order.
//
// Per key, steps 1-4: 2 full-rate VALU (FMA, AND) + ds_add in the histogram, 3 full-rate VALU (shift, AND, XOR: the
// staging address from the byte position) + ds_add_rtn + ds_write in the placement, a quarter of a ds_read_b128; then, per
// lane and per loop trip of two phases (31 in-lane compare-exchanges + the one across the lane boundary = 64 v_min /
// v_max at the source level), as compiled for the headline kernel: up to round 6 130 slow-rate v_min / v_max, 66 of
// them `v_max x, y, y` canonicalisations of the operands (see F32KeysRaw below; the "33 per phase" of earlier rounds was
// the source-level count); in round 7, in the full classes, the 64 + 31 full-rate v_mov that rotated the loop's
// registers; since round 8 the full classes' loop runs four phases per trip, which needs no rotation, and exchanges the
// keys across the lane boundary by two DPP wave shifts instead of two ds_bpermute and two selects: per trip 124 v_min /
// v_max + 4 v_min / v_max with DPP + 4 v_mov (binsort_read_back_and_fix; profiles/r08_forward_summary.txt).  The g mod 4
// odd phases are straight-line code: behind the loop in rounds 8 - 22, at the price of 16 v_mov_b64 at the loop's exit and
// 16 / 32 more for a remainder of two / three phases, once per sort, where paths of different length met in different
// registers; since round 23 the headline loss kernel runs them FIRST, each remainder behind its own copy of the
// read-back, and pays none of these copies (REM_FIRST; profiles/r23_forward_summary.txt) -- the other full classes keep
// the earlier order, which costs them fewer registers.
// With g ~ 9 (uniformly spread coordinates) a quarter of the network's VALU work and an eighth of its crossbar traffic.
// The result is the exact ascending order of the fp32 keys whatever order the atomics were served in.
// Data with long runs (clustered clouds, duplicates, an all-zero cloud: g > SHW_BINSORT_MAX_RUN) is detected
// after step 2 -- before any key has moved -- and the caller sorts it with the network instead (wave-uniform branch).
// So are rows of caller-supplied coordinates with a value outside [0, 1] (binsort_keys_fit): the map does not saturate.
// The above is the form of the FULL classes (n == 64*EPT).  Classes with pads keep the earlier form -- bin =
// min(floor(key * NB), NB-1) by a saturating v_cvt, counters in keys, pads steered by selects -- because the new one
// made their kernels slower (see below, "the classes with pads").
//
// The steps as functions: 1 binsort_histogram_full / binsort_histogram, which end in 2 binsort_scan; 3 binsort_place_full /
// binsort_place; 4-5 binsort_read_back_and_fix (full classes: four phases per trip) and oddeven_fixup (classes with pads).
// Shared by the sorts built on this one (bin_sort_idx.hpp, coop_sort.hpp, coop_sort_kv.hpp): wave_inclusive_scan_dpp and
// wave_inclusive_max_dpp (step 2), binsort_boundary<KEYS> (step 5) and the address map binsort_addr.
//
// LDS per wave: NB counters (128*EPT bytes) + a 64*EPT-float staging buffer (256*EPT bytes).  LDS operations of one
// wave execute in order and nothing here is shared with another wave: no barrier.
// The headline loss kernel (2048 points, one wave, p = 2) asks for the same block and lays it out otherwise (round 28;
// wave_sort_binned, ALIAS_BPL): 1280 counters, 5120 bytes, start where the 1024 did and run on UNDER the first 1024 bytes of
// the staging buffer, which has not moved (bytes 4096 .. 12 287).  A counter and a staged key are never alive together:
// the placement takes all 32 positions of a lane before it writes the first key (binsort_place_full_two_step), and the
// next sort zeroes the counters behind this one's read-back.  More bins, shorter runs: g ~ 7.6 instead of 8.4 phases; the
// counters are scanned 20 per lane -- a lane stride of 80 bytes, on which the scan's ds_read_b128 meet no bank conflict
// (at 128 bytes, 2048 bins, they do, and the kernel is 27 % slower: profiles/r28_forward_summary.txt).
#pragma once
#include <hip/hip_runtime.h>

#include "wave_sort.hpp"

#ifndef SHW_BINSORT_NB_PER_EPT
#define SHW_BINSORT_NB_PER_EPT 32
#endif
// Longest equal-bin run the one-wave sorts fix up by odd-even phases (one phase, when this was measured, ~ 65 slow-rate
// instructions per lane as compiled; rounds 7 and 8 brought that to 32 in the full classes and did not re-measure the
// threshold)
// before they prefer the bitonic network (~4.4 us per 2048-key sort, after the histogram has been paid): round 2
// used 24, which sent 23 % of the slices of the notebooks' cube-surface clouds and 95 % of tightly clustered clouds to
// the network (profiles/r03_nonuniform.txt).  Measured break-even: ~45 phases (at 64 clouds of 32-fold duplicate
// points took 0.68 instead of 0.53 ms per launch, at 24 sixteen tight clusters 0.56 instead of 0.52).
#ifndef SHW_BINSORT_MAX_RUN
#define SHW_BINSORT_MAX_RUN 40
#endif
// the cooperative sorts (several waves per slice) finish a run that straddles two waves inside a 64-key window: < 32
#ifndef SHW_COOP_MAX_RUN
#define SHW_COOP_MAX_RUN 24
#endif

namespace shw {

// a counter by its 32-bit LDS address (kept per key from the histogram pass to the placement pass)
typedef __attribute__((address_space(3))) unsigned lds_u32;
__device__ __forceinline__ unsigned lds_address(const void* p) {
  return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}
__device__ __forceinline__ lds_u32* lds_counter(unsigned address) { return (lds_u32*)(uintptr_t)address; }

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// bins of the key-only sort: 32 per key slot of a lane (two keys per bin) for the power-of-two classes; otherwise the next
// count whose share per lane in the scan is a multiple of four (128-bit accesses): 768 for 20 and 24 keys per lane, 1024 for 28
template <int EPT>
constexpr int binsort_bins() {
  return is_pow2(EPT) ? SHW_BINSORT_NB_PER_EPT * EPT : 64 * ((((EPT + 1) / 2) + 3) / 4 * 4);
}

// byte address of sorted position `pos` in the staging buffer: rows of 32 floats (one lane's read-back), the eight
// 16-byte chunks of a row XOR-permuted by bits 1..3 of the row number so that the 16 lanes a ds_read_b128 serves
// together touch 16 different bank groups (lane stride is 128 B: without the permutation 8 lanes share each group)
template <int EPT>
__device__ __forceinline__ unsigned binsort_addr(unsigned pos) {
  // a row is EPT floats = EPT/4 chunks; lanes 2^k apart (k = 1 at EPT 32, 2 at 16, 3 at 8) share bank groups, and
  // bit 6 of pos is bit k of the row number in every size class: (pos >> 2) puts it on the chunk-index bits
  return (pos << 2) ^ ((pos >> 2) & (unsigned)((EPT / 4 - 1) << 4));
}
// the same address from the BYTE position p4 = 4 pos, which is what the scanned counters hand out: no shift to bytes
template <int EPT>
__device__ __forceinline__ unsigned binsort_addr4(unsigned p4) {
  return p4 ^ ((p4 >> 4) & (unsigned)((EPT / 4 - 1) << 4));
}

// inclusive prefix sum over the lanes of a wave (row_shr DPP steps inside rows of 16, then the two row broadcasts)
__device__ __forceinline__ int wave_inclusive_scan_dpp(int v) {
  // classic GCN scan: row_shr:1,2,3 / 4 / 8 then row_bcast:15 and row_bcast:31 with the matching row masks
  int t;
  t = __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false); v += t;            // row_shr:1
  t = __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false); v += t;            // row_shr:2
  t = __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false); v += t;            // row_shr:4
  t = __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false); v += t;            // row_shr:8
  t = __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false); v += t;            // row_bcast:15 -> rows 1, 3
  t = __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false); v += t;            // row_bcast:31 -> rows 2, 3
  return v;
}
// inclusive prefix maximum of non-negative values by the same six steps: lane 63 ends up with the maximum of the wave
__device__ __forceinline__ int wave_inclusive_max_dpp(int v) {
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false));
  return v;
}

// Step 2 of a one-wave sort: exclusive prefix sum over the 64 BPL counters, in place (lane owns counters
// [lane*BPL, (lane+1)*BPL)).  Returns the largest counter (wave-uniform), in the counters' own unit.
template <int BPL>
__device__ __forceinline__ int binsort_scan(unsigned* cnt, int lane) {
  unsigned c[BPL];
#pragma unroll
  for (int j = 0; j < BPL / 4; ++j) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(cnt + lane * BPL + j * 4);
    c[4 * j] = v.x; c[4 * j + 1] = v.y; c[4 * j + 2] = v.z; c[4 * j + 3] = v.w;
  }
  unsigned run = 0, total = 0;
#pragma unroll
  for (int j = 0; j < BPL; ++j) {
    run = c[j] > run ? c[j] : run;
    const unsigned t = c[j];
    c[j] = total;                                        // exclusive inside the lane
    total += t;
  }
  const int incl = wave_inclusive_scan_dpp((int)total);
  const unsigned base = (unsigned)incl - total;
#pragma unroll
  for (int j = 0; j < BPL / 4; ++j)
    *reinterpret_cast<u32x4*>(cnt + lane * BPL + j * 4) =
        u32x4{c[4 * j] + base, c[4 * j + 1] + base, c[4 * j + 2] + base, c[4 * j + 3] + base};
  __builtin_amdgcn_wave_barrier();
  return __builtin_amdgcn_readlane(wave_inclusive_max_dpp((int)run), 63);
}

// The same scan for the counters that lie under the staging buffer (the headline loss kernel: 20 per lane), the lane's
// sum first: sum and largest counter two counters at a time (v_add3_u32, v_max3_u32), the wave scan of the sums gives the
// lane's base, and the running sum that is written back STARTS at the base -- one add per counter where binsort_scan pays
// the in-lane prefix and then the base (per counter: an add and half a v_add3 / v_max3 against two adds and a v_max).
// `total` = the sum over all counters (wave-uniform).
template <int BPL>
__device__ __forceinline__ int binsort_scan_sum_first(unsigned* cnt, int lane, unsigned& total) {
  unsigned c[BPL];
  unsigned run = 0, sum = 0;
#pragma unroll
  for (int j = 0; j < BPL / 4; ++j) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(cnt + lane * BPL + j * 4);
    c[4 * j] = v.x; c[4 * j + 1] = v.y; c[4 * j + 2] = v.z; c[4 * j + 3] = v.w;
    sum += v.x + v.y; sum += v.z + v.w;
    run = max(max(v.x, v.y), run); run = max(max(v.z, v.w), run);
  }
  const int incl = wave_inclusive_scan_dpp((int)sum);
  total = (unsigned)__builtin_amdgcn_readlane(incl, 63);
  unsigned at = (unsigned)incl - sum;
#pragma unroll
  for (int j = 0; j < BPL / 4; ++j) {
    u32x4 w;
    w.x = at; at += c[4 * j]; w.y = at; at += c[4 * j + 1]; w.z = at; at += c[4 * j + 2]; w.w = at; at += c[4 * j + 3];
    *reinterpret_cast<u32x4*>(cnt + lane * BPL + j * 4) = w;
  }
  __builtin_amdgcn_wave_barrier();
  return __builtin_amdgcn_readlane(wave_inclusive_max_dpp((int)run), 63);
}

// Byte offset of a key's counter: 4 * bin, bin in [0, NB), monotone non-decreasing in the key over [0, 1].
//     off = bits(fma(key, 4 NB - 1, 2^23)) & (next_pow2(4 NB) - 4)
// For key in [0, 1] the sum lies in [2^23, 2^23 + 4 NB - 1]: there an fp32 ulp is 1, so the rounding of the FMA leaves
// round(key (4 NB - 1)) in the low mantissa bits (rounding is monotone); the mask drops the exponent and the two low
// bits (monotone again), leaving a multiple of 4 that is at most 4 NB - 4 (also where 4 NB is no power of two: 768
// bins, mask 4092, value at most 3071 -- tests/test_bin_map_cpu.py -- though no such class uses it today).  One FMA + one AND, both full rate, against v_mul + v_cvt_u32 +
// v_min_u32 (quarter rate) + a shift to bytes for min(floor(key NB), NB - 1).  Any monotone map sorts exactly: the
// fix-up phases order every equal-bin run, and g is measured on the bins actually used.
//   * -0 and denormals -> bin 0;  1 and the float above it -> bin NB - 1  (round((1 + 2^-23)(4 NB - 1)) = 4 NB - 1);
//   * NaN -> the low bits of a NaN: 0 for the canonical quiet NaN, always a multiple of 4 below 4 NB (full classes are
//     powers of two), i.e. inside the counters (in bounds; NaN input has no defined order anyway);
//   * the map does NOT saturate: 1.5 -> bin (NB - 1) / 2, -0.25 -> NB / 2, +inf -> 0.  Keys outside [0, 1] must not come
//     here.  Projected coordinates never are: circle_coord (ssw_common.hpp) returns P +- (r' - 1/8) with P one of 1/8, 3/8,
//     5/8, 7/8 exactly and r' - 1/8 in [-1/8, +0], so the largest value is 1.0 exactly and the smallest +0.  Pads (+inf)
//     do not exist in the full classes, the only ones that use this map.  Rows of caller-supplied coordinates
//     (shw_circle_ot) are tested by binsort_keys_fit and take the network when a value is out of range (wave_sort_binned).
template <int NB>
__device__ __forceinline__ unsigned binsort_off(float key) {
  constexpr unsigned kMask = (unsigned)next_pow2_c(4 * NB) - 4u;
  return (unsigned)as_i(__builtin_fmaf(key, (float)(4 * NB - 1), 8388608.f)) & kMask;
}

// Rows of circle coordinates come from the caller (coordinate-row mode), who may pass values outside [0, 1]; the exact
// order of such a row is still owed.  Wave-uniform: true when every key of the wave lies in [0, 1] (NaN: false).
// Only evaluated in coordinate-row mode -- the projection path pays one scalar branch per sort for it.
template <int EPT>
__device__ __forceinline__ bool binsort_keys_fit(const float (&key)[EPT]) {
  bool bad = false;
#pragma unroll
  for (int r = 0; r < EPT; ++r) bad |= !(key[r] >= 0.f && key[r] <= 1.f);
  return __ballot(bad) == 0ull;
}

// value of `x` held by lane `src` (ds_bpermute)
__device__ __forceinline__ float from_lane(int src, float x) { return as_f(__builtin_amdgcn_ds_bpermute(src << 2, as_i(x))); }
__device__ __forceinline__ unsigned from_lane(int src, unsigned x) { return (unsigned)__builtin_amdgcn_ds_bpermute(src << 2, (int)x); }

// one compare-exchange between the last key of every lane and the first key of the next lane; the two ends of the wave
// meet the highest / lowest key of the policy (KEYS::bound) and keep their own.  Needs EPT >= 2.
template <class KEYS, int EPT>
__device__ __forceinline__ void binsort_boundary(typename KEYS::type (&x)[EPT], int lane) {
  const typename KEYS::type nxt = from_lane(min(lane + 1, 63), x[0]);
  const typename KEYS::type prv = from_lane(max(lane - 1, 0), x[EPT - 1]);
  x[EPT - 1] = KEYS::lo(x[EPT - 1], lane < 63 ? nxt : KEYS::bound(true));
  x[0] = KEYS::hi(x[0], lane > 0 ? prv : KEYS::bound(false));
}

// g phases of odd-even transposition over the keys of a wave, two phases per loop trip (wave-uniform trip count): pairs
// (2i, 2i+1) inside a lane; then pairs (2i+1, 2i+2) and the pair across every lane boundary.  The loop of the classes
// with pads (binsort_place).  The full classes have their own, four phases per trip (binsort_read_back_and_fix).  The sort
// with indices and the cooperative sorts write this same loop out in place around binsort_boundary: called as a function
// it compiles to other code there (profiles/r12_sort_dedup.txt) -- a change to this loop goes to those three as well.
template <class KEYS, int EPT>
__device__ __forceinline__ void oddeven_fixup(typename KEYS::type (&key)[EPT], int lane, int g) {
  for (int phase = 0; phase < g; phase += 2) {
#pragma unroll
    for (int r = 0; r + 1 < EPT; r += 2) cmp_swap<KEYS>(key[r], key[r + 1]);
    if (phase + 1 < g) {
#pragma unroll
      for (int r = 1; r + 1 < EPT; r += 2) cmp_swap<KEYS>(key[r], key[r + 1]);
      binsort_boundary<KEYS, EPT>(key, lane);
    }
  }
}

// Key policy of the fix-up phases of the FULL classes: the v_min_f32 / v_max_f32 of F32Keys and nothing else.  The
// kernels run in IEEE mode, where minnum / maxnum must quiet a signalling NaN, and the keys of the fix-up loop are
// loop-carried values that came out of ds_read_b128: the compiler cannot know them canonical and puts a
// `v_max_f32 x, y, y` in front of BOTH operands of EVERY compare-exchange.  One loop trip of the headline kernel (two
// phases: 64 v_min / v_max that do the work) compiled to 130 slow-rate instructions, 66 of them canonicalisations;
// written as asm the two instructions stand alone: 64 slow-rate instructions per trip (round 7).
// They are the instructions F32Keys compiles to, so for every key that is no signalling NaN -- -0, denormals (fp32
// denormals are on), +inf pads, quiet NaNs -- the result has the same bits as before; a signalling NaN is quieted by the
// v_min / v_max itself, and rows with NaNs have no defined order.  Plain VALU: no wait states, nothing for s_waitcnt; not
// volatile, so the compiler schedules and removes them like any other pure operation.
// The classes with pads (binsort_place) and the cooperative sort (coop_sort.hpp) keep F32Keys: not measured with this.
// (Round 7 exchanged the keys across the lane boundary with these two instructions behind two ds_bpermute and two
// +-inf selects; round 8 replaced that by binsort_boundary_dpp.)
struct F32KeysRaw {
  typedef float type;
  static __device__ __forceinline__ float lo(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
  }
  static __device__ __forceinline__ float hi(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
  }
};

// binsort_boundary on F32KeysRaw without LDS traffic and without selects: the neighbour's key comes through a DPP wave
// shift (two ds_bpermute and two selects otherwise).
//   hi = v_min_f32_dpp(x[0] of lane + 1, x[EPT-1])   wave_shl:1     lo = v_max_f32_dpp(x[EPT-1] of lane - 1, x[0])   wave_shr:1
// No bound_ctrl: a lane without a source (63 for the first, 0 for the second) is switched off for that instruction and
// keeps its destination, which holds its own key on entry ("+" operands) -- what the +-inf selects of binsort_boundary
// give.  Both instructions read the keys as they stand after the odd phase: the destinations are early-clobber copies,
// never the registers of x[0] / x[EPT-1] themselves.  A DPP operand written by the VALU instruction just before needs two
// wait states, which the compiler cannot see into an asm block to provide: the s_nop 1 does.  Not volatile, plain "v"
// operands: scheduled like F32KeysRaw.
template <int EPT>
__device__ __forceinline__ void binsort_boundary_dpp(float (&x)[EPT]) {
  float hi = x[EPT - 1], lo = x[0];
  asm("s_nop 1\n\t"
      "v_min_f32_dpp %0, %2, %0 wave_shl:1 row_mask:0xf bank_mask:0xf\n\t"
      "v_max_f32_dpp %1, %3, %1 wave_shr:1 row_mask:0xf bank_mask:0xf"
      : "+&v"(hi), "+&v"(lo)
      : "v"(x[0]), "v"(x[EPT - 1]));
  x[EPT - 1] = hi;
  x[0] = lo;
}

// the two phases of the odd-even transposition: pairs (2i, 2i+1) inside a lane; pairs (2i+1, 2i+2) and the pair across
// every lane boundary
template <int EPT>
__device__ __forceinline__ void binsort_even_phase(float (&key)[EPT]) {
#pragma unroll
  for (int r = 0; r + 1 < EPT; r += 2) cmp_swap<F32KeysRaw>(key[r], key[r + 1]);
}
template <int EPT>
__device__ __forceinline__ void binsort_odd_phase(float (&key)[EPT]) {
#pragma unroll
  for (int r = 1; r + 1 < EPT; r += 2) cmp_swap<F32KeysRaw>(key[r], key[r + 1]);
  binsort_boundary_dpp<EPT>(key);
}

// Step 4: read back EPT consecutive positions per lane
template <int EPT>
__device__ __forceinline__ void binsort_read_back(float (&key)[EPT], int lane, const char* bytes) {
#pragma unroll
  for (int j = 0; j < EPT / 4; ++j) {
    const unsigned pos0 = (unsigned)lane * EPT + 4u * j;          // logical chunk j of row `lane`
    const f32x4 v = *reinterpret_cast<const f32x4*>(bytes + binsort_addr<EPT>(pos0));
    key[4 * j] = v.x; key[4 * j + 1] = v.y; key[4 * j + 2] = v.z; key[4 * j + 3] = v.w;
  }
}

// Steps 4-5: read back EPT consecutive positions per lane, then g phases of odd-even transposition (wave-uniform trip
// count).  Four phases per loop trip: a compare-exchange needs a temporary, so the keys leave a phase one register over;
// after two phases the compiler copies them back at the loop's back edge (31 v_mov per trip, round 7), after four it finds
// an assignment that needs no copy.  Where the g mod 4 odd phases run decides what the paths of different length cost:
//   * REM_FIRST = false (rounds 8 - 22; every class but the headline's): the loop first, the remainder behind it as
//     straight-line code behind wave-uniform branches.  The keys of the paths meet in different registers: 16 v_mov_b64 at
//     the loop's exit, 16 more for a remainder of two phases and 32 more for one of three -- once per sort.
//   * REM_FIRST = true (round 23; the headline loss kernel): the remainder first -- 1: odd;  2: even, odd;  3: odd, even,
//     odd -- then the trips, which begin with an even phase, so the alternation is unbroken.  g alternating phases sort a
//     run of g keys whichever parity comes first (tests/test_fixup_schedule_cpu.py: every 0/1 filling of every run).  Each
//     remainder has its OWN copy of the read-back (the differing asm comments keep the compiler from merging the four
//     again): the destinations of the ds_read_b128 are free, so every path is allocated backwards from the registers the
//     loop header expects, and the loop has one exit.  No copy between the read-back and the loop, none behind the back
//     edge.  Only where the caller's sorts are straight-line code (the headline kernel's two passes): inside a `which`
//     loop the same form spills (3 - 5 VGPRs in ssw_forward_kernel<32,1,2,true> and <32,1,0,true>) and costs
//     ssw_forward_kernel<16,4,2,true> a wave per SIMD (80 -> 84 VGPRs), so those keep the form above.
template <int EPT, bool REM_FIRST = false>
__device__ __forceinline__ void binsort_read_back_and_fix(float (&key)[EPT], int lane, int g, float* buf) {
  char* bytes = reinterpret_cast<char*>(buf);
  if constexpr (REM_FIRST) {
    int ln = lane;
    switch (g & 3) {
      case 0:
        asm volatile("; fix-up remainder 0" : "+v"(ln));
        binsort_read_back<EPT>(key, ln, bytes);
        break;
      case 1:
        asm volatile("; fix-up remainder 1" : "+v"(ln));
        binsort_read_back<EPT>(key, ln, bytes);
        binsort_odd_phase<EPT>(key);
        break;
      case 2:
        asm volatile("; fix-up remainder 2" : "+v"(ln));
        binsort_read_back<EPT>(key, ln, bytes);
        binsort_even_phase<EPT>(key);
        binsort_odd_phase<EPT>(key);
        break;
      default:
        asm volatile("; fix-up remainder 3" : "+v"(ln));
        binsort_read_back<EPT>(key, ln, bytes);
        binsort_odd_phase<EPT>(key);
        binsort_even_phase<EPT>(key);
        binsort_odd_phase<EPT>(key);
        break;
    }
    for (int trips = g >> 2; trips > 0; --trips) {
      binsort_even_phase<EPT>(key);
      binsort_odd_phase<EPT>(key);
      binsort_even_phase<EPT>(key);
      binsort_odd_phase<EPT>(key);
    }
  } else {
    // (the read-back written out in place: through binsort_read_back the two-wave kernels ssw_forward2_kernel<32,*,true>
    //  compile to other code, 108 and 128 bytes longer)
#pragma unroll
    for (int j = 0; j < EPT / 4; ++j) {
      const unsigned pos0 = (unsigned)lane * EPT + 4u * j;          // logical chunk j of row `lane`
      const f32x4 v = *reinterpret_cast<const f32x4*>(bytes + binsort_addr<EPT>(pos0));
      key[4 * j] = v.x; key[4 * j + 1] = v.y; key[4 * j + 2] = v.z; key[4 * j + 3] = v.w;
    }
    int phase = 0;
    for (; phase + 4 <= g; phase += 4) {
      binsort_even_phase<EPT>(key);
      binsort_odd_phase<EPT>(key);
      binsort_even_phase<EPT>(key);
      binsort_odd_phase<EPT>(key);
    }
    if (phase < g) {
      binsort_even_phase<EPT>(key);
      if (phase + 1 < g) {
        binsort_odd_phase<EPT>(key);
        if (phase + 2 < g) binsort_even_phase<EPT>(key);
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
}

// ---- the full classes (n == 64*EPT, no pads): byte-offset map, counters in bytes --------------------------------------
// Steps 1-2.  Returns the longest equal-bin run g (wave-uniform); on return cnt[] holds the exclusive prefix sums (the
// first sorted position of every bin, in bytes).  key[r] belongs to point r*64 + lane.  No rank is returned:
// binsort_place_full takes the position from an atomic on the scanned starts.  slot[r] = LDS address of the counter of
// key[r], kept for binsort_place_full.
// NB: the bin count -- binsort_bins<EPT>() everywhere but in the headline loss kernel, whose counters lie under the staging
// buffer and may be more (wave_sort_binned, ALIAS_BPL).
template <int EPT, int NB = binsort_bins<EPT>()>
__device__ __forceinline__ int binsort_histogram_full(const float (&key)[EPT], int lane, unsigned* cnt, unsigned (&slot)[EPT]) {
  constexpr int BPL = NB / 64;                          // bins per lane in the scan (EPT/2: 16 at EPT = 32)
  static_assert(BPL >= 4 && BPL % 4 == 0 && NB == 64 * BPL, "bin sort needs >= 4 bins per lane, a multiple of four");
  // zero the counters: every ds_write_b128 covers 1 KB of consecutive addresses (conflict-free)
#pragma unroll
  for (int j = 0; j < BPL / 4; ++j)
    *reinterpret_cast<u32x4*>(cnt + j * 256 + lane * 4) = u32x4{0u, 0u, 0u, 0u};
  __builtin_amdgcn_wave_barrier();
  const unsigned cb = lds_address(cnt);                  // the counters by byte address
  constexpr int CH = chunk_of(EPT);                      // rows per chunk (the placement's atomics in flight per lane)
#pragma unroll
  for (int r0 = 0; r0 < EPT; r0 += CH) {
#pragma unroll
    for (int j = 0; j < CH; ++j) {                       // result unused: ds_add_u32, nothing to wait for
      slot[r0 + j] = cb + binsort_off<NB>(key[r0 + j]);
      // held in a register for the placement pass: the empty asm makes the offset opaque.  Left alone the compiler
      // recomputes the FMA and the AND per key there (2 x 64 more VALU instructions per slice, 34 fewer VGPRs)
      asm volatile("" : "+v"(slot[r0 + j]));
      __hip_atomic_fetch_add(lds_counter(slot[r0 + j]), 4u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  __builtin_amdgcn_wave_barrier();
  if constexpr (NB == binsort_bins<EPT>()) {
    return binsort_scan<BPL>(cnt, lane) >> 2;            // the largest counter, counted in bytes: four per key
  } else {
    unsigned total;
    const int g = binsort_scan_sum_first<BPL>(cnt, lane, total) >> 2;
    // Where 4 NB is no power of two the mask of binsort_off lets the low bits of a NaN name a word behind the last
    // counter (every key in [0, 1] stays below 4 NB; the mask stays inside the wave's block: wave_sort_binned).  Such a
    // key is missing from the sum over the NB counters: the slice takes the network, which needs no counter, before any
    // key has moved.
    if constexpr (!is_pow2(NB)) return total == 256u * EPT ? g : SHW_BINSORT_MAX_RUN + 1;
    return g;
  }
}

// Steps 3-5 of a full class (only after binsort_histogram_full returned g <= SHW_BINSORT_MAX_RUN).  The byte position of
// a key is what ds_add_rtn(4) returns on its bin's scanned start (cnt[] holds the bin ends afterwards); inside a bin the
// keys land in the order the atomics are served, which the fix-up phases make irrelevant.
template <int EPT, bool REM_FIRST = false>
__device__ __forceinline__ void binsort_place_full(float (&key)[EPT], const unsigned (&slot)[EPT], int lane, int g,
                                                   float* buf) {
  char* bytes = reinterpret_cast<char*>(buf);
  constexpr int CH = chunk_of(EPT);
#pragma unroll
  for (int r0 = 0; r0 < EPT; r0 += CH) {
    unsigned pos[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j)
      pos[j] = __hip_atomic_fetch_add(lds_counter(slot[r0 + j]), 4u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
#pragma unroll
    for (int j = 0; j < CH; ++j) *reinterpret_cast<float*>(bytes + binsort_addr4<EPT>(pos[j])) = key[r0 + j];
    __builtin_amdgcn_sched_barrier(0);
  }
  __builtin_amdgcn_wave_barrier();
  binsort_read_back_and_fix<EPT, REM_FIRST>(key, lane, g, buf);
}

// The placement in two steps, for counters that lie UNDER the staging buffer (the headline loss kernel: wave_sort_binned,
// ALIAS_BPL): all EPT atomics first, their byte positions kept in the registers that held the counters' addresses, then
// the EPT writes.  Nothing reads a counter after the last atomic, so the first write may land on one.  LDS operations of one
// wave execute in order; the compiler is held to the same order by the memory clobber and the scheduling barrier between
// the steps (an atomic on `unsigned` and a store of `float` do not alias by their types).  Always REM_FIRST.
template <int EPT>
__device__ __forceinline__ void binsort_place_full_two_step(float (&key)[EPT], unsigned (&slot)[EPT], int lane, int g,
                                                            float* buf) {
  char* bytes = reinterpret_cast<char*>(buf);
#pragma unroll
  for (int r = 0; r < EPT; ++r)
    slot[r] = __hip_atomic_fetch_add(lds_counter(slot[r]), 4u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int r = 0; r < EPT; ++r) *reinterpret_cast<float*>(bytes + binsort_addr4<EPT>(slot[r])) = key[r];
  __builtin_amdgcn_wave_barrier();
  binsort_read_back_and_fix<EPT, true>(key, lane, g, buf);
}

// ---- the classes with pads (n < 64*EPT): the saturating map, counters in keys -----------------------------------------
// Kept as they were.  With the byte-offset map, byte counters and unsigned point offsets together the two-wave loss kernel of
// the partly filled classes lost on MI355X (N = 2000: 0.2823 -> 0.3037 ms per step, N = 1200: 0.1692 -> 0.1759, B = 64,
// L = 512; registers 168 -> 116 at 32 keys per lane: the compiler no longer overlaps the chunks' loads), while every full
// class gained (N = 2048: 0.2076 -> 0.1991, N = 1024: 0.1054 -> 0.1018).  The map below saturates, so these classes also
// need no range test in coordinate-row mode.
// bin of a key: v_cvt_u32_f32 saturates (NaN -> 0, +inf -> 0xffffffff), so the bin is always inside [0, NB).  The
// histogram and the placement both compute it with this one function: a key lands in the bin it was counted in.
template <int NB>
__device__ __forceinline__ unsigned binsort_bin(float key) {
  const unsigned t = (unsigned)(key * (float)NB);
  return t < (unsigned)(NB - 1) ? t : (unsigned)(NB - 1);
}

// Steps 1-2.  Returns the longest equal-bin run g (wave-uniform); on return cnt[] holds the exclusive prefix sums (the
// first sorted position of every bin).  `n` = number of live keys; key[r] belongs to point r*64 + lane.  Nothing per key
// survives the counting pass (no rank is returned): binsort_place recomputes the bin and takes the position from an
// atomic on the scanned starts, so the sorted source carried across the target's sort is the only per-key state.
template <int EPT, bool FULL>
__device__ __forceinline__ int binsort_histogram(const float (&key)[EPT], int lane, int n, unsigned* cnt) {
  constexpr int NB = binsort_bins<EPT>();
  constexpr int BPL = NB / 64;                          // bins per lane in the scan (EPT/2: 16 at EPT = 32)
  static_assert(BPL >= 4 && BPL % 4 == 0, "bin sort needs >= 4 bins per lane");
  // zero the counters: every ds_write_b128 covers 1 KB of consecutive addresses (conflict-free)
#pragma unroll
  for (int j = 0; j < BPL / 4; ++j)
    *reinterpret_cast<u32x4*>(cnt + j * 256 + lane * 4) = u32x4{0u, 0u, 0u, 0u};
  __builtin_amdgcn_wave_barrier();
  constexpr int CH = chunk_of(EPT);                      // rows per chunk (the placement's atomics in flight per lane)
#pragma unroll
  for (int r0 = 0; r0 < EPT; r0 += CH) {
    // key[r] belongs to point r*64 + lane: the pads of a class that is not full are its LAST rows -- a chunk of rows is
    // entirely live (no masks: the code of a full class), entirely pads (nothing to count) or the one mixed chunk;
    // which of the three is uniform over the wave
    // (measured, N = 1200 / 2000 at B = 64, L = 512: the branches pay in the classes of 12 .. 28 keys per lane -- the loads
    //  are no longer hoisted together, 150 -> 111 VGPRs, a fourth wave per SIMD -- and cost 6 % at 32, where LDS holds the
    //  occupancy at three: power-of-two classes keep the masked form)
    constexpr bool kByChunk = !is_pow2(EPT);
    const bool all_live = FULL || (kByChunk && (r0 + CH) * kWave <= n);
    const bool none_live = !FULL && kByChunk && r0 * kWave >= n;
    if (none_live) {
      // nothing to count: the placement puts these pads at their own index
    } else if (all_live) {
#pragma unroll
      for (int j = 0; j < CH; ++j)                       // result unused: ds_add_u32, nothing to wait for
        __hip_atomic_fetch_add(cnt + binsort_bin<NB>(key[r0 + j]), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    } else {
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const bool live = (r0 + j) * kWave + lane < n;
        // pads add 0 (no divergent branch around the atomic), to 64 different counters: 64 atomics on ONE address would
        // be served one after the other
        __hip_atomic_fetch_add(cnt + (live ? binsort_bin<NB>(key[r0 + j]) : (unsigned)lane), live ? 1u : 0u,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  __builtin_amdgcn_wave_barrier();
  return binsort_scan<BPL>(cnt, lane);
}

// Steps 3-5 (only after binsort_histogram returned g <= SHW_BINSORT_MAX_RUN).  The position of a live key is what
// ds_add_rtn returns on its bin's scanned start (cnt[] holds the bin ends afterwards); inside a bin the keys land in the
// order the atomics are served, which the fix-up phases make irrelevant.
template <int EPT, bool FULL>
__device__ __forceinline__ void binsort_place(float (&key)[EPT], int lane, int n, int g, unsigned* cnt, float* buf) {
  constexpr int NB = binsort_bins<EPT>();
  char* bytes = reinterpret_cast<char*>(buf);
  constexpr int CH = chunk_of(EPT);
#pragma unroll
  for (int r0 = 0; r0 < EPT; r0 += CH) {
    constexpr bool kByChunk = !is_pow2(EPT);                       // (see binsort_histogram)
    const bool all_live = FULL || (kByChunk && (r0 + CH) * kWave <= n);
    const bool none_live = !FULL && kByChunk && r0 * kWave >= n;
    if (none_live) {
      // pads (key +inf, original index i >= n) go to position i: the positions behind the n live keys, each once
#pragma unroll
      for (int j = 0; j < CH; ++j)
        *reinterpret_cast<float*>(bytes + binsort_addr<EPT>((unsigned)((r0 + j) * kWave + lane))) = key[r0 + j];
    } else if (all_live) {
      unsigned pos[CH];
#pragma unroll
      for (int j = 0; j < CH; ++j)
        pos[j] = __hip_atomic_fetch_add(cnt + binsort_bin<NB>(key[r0 + j]), 1u, __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_WAVEFRONT);
#pragma unroll
      for (int j = 0; j < CH; ++j) *reinterpret_cast<float*>(bytes + binsort_addr<EPT>(pos[j])) = key[r0 + j];
    } else {
      unsigned pos[CH];
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const bool live = (r0 + j) * kWave + lane < n;
        pos[j] = __hip_atomic_fetch_add(cnt + (live ? binsort_bin<NB>(key[r0 + j]) : (unsigned)lane), live ? 1u : 0u,
                                        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
      }
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const unsigned i = (unsigned)((r0 + j) * kWave + lane);
        *reinterpret_cast<float*>(bytes + binsort_addr<EPT>((int)i < n ? pos[j] : i)) = key[r0 + j];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int j = 0; j < EPT / 4; ++j) {
    const unsigned pos0 = (unsigned)lane * EPT + 4u * j;          // logical chunk j of row `lane`
    const f32x4 v = *reinterpret_cast<const f32x4*>(bytes + binsort_addr<EPT>(pos0));
    key[4 * j] = v.x; key[4 * j + 1] = v.y; key[4 * j + 2] = v.z; key[4 * j + 3] = v.w;
  }
  oddeven_fixup<F32Keys, EPT>(key, lane, g);
  __builtin_amdgcn_wave_barrier();
}

// The bitonic network for a class that is not a power of two (the rare fallback of such a class): sort next_pow2(EPT) keys
// per lane with +inf / all-ones behind the real ones, then take the 64 EPT smallest through the staging buffer into the
// layout "sorted position lane*EPT + r".  MAXKEY sorts behind every real key.
template <int EPT, class T>
__device__ __forceinline__ void wave_sort_relayout(T (&key)[EPT], int lane, T maxkey, void* buf) {
  constexpr int P2 = next_pow2_c(EPT);
  T tmp[P2];
#pragma unroll
  for (int r = 0; r < P2; ++r) tmp[r] = r < EPT ? key[r < EPT ? r : 0] : maxkey;
  wave_sort<P2>(tmp, lane);
  char* bytes = reinterpret_cast<char*>(buf);
#pragma unroll
  for (int r = 0; r < P2; ++r) {
    const unsigned pos = (unsigned)(lane * P2 + r);
    if (pos < (unsigned)(kWave * EPT)) *reinterpret_cast<T*>(bytes + binsort_addr<EPT>(pos)) = tmp[r];
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int r = 0; r < EPT; ++r) key[r] = *reinterpret_cast<const T*>(bytes + binsort_addr<EPT>((unsigned)(lane * EPT + r)));
  __builtin_amdgcn_wave_barrier();
}

// Sort the 64*EPT keys of a wave ascending (pads = +inf behind the n live keys).  Falls back to the bitonic network
// when the data has runs longer than SHW_BINSORT_MAX_RUN, or -- full classes -- when `rows` (wave-uniform: the keys are
// caller-supplied coordinates, not projections) and a key lies outside [0, 1], the domain of the byte-offset map.
// scratch: binsort_bins<EPT>() counters with the 64*EPT floats of the staging buffer directly behind them (one block).
// Returns the longest run of keys that share a bin (> SHW_BINSORT_MAX_RUN: the slice took the network).
// REM_FIRST (full classes): the phase order of binsort_read_back_and_fix.
// ALIAS_BPL (full classes with REM_FIRST; 0: off): 64 * ALIAS_BPL counters that start at `scratch` as always and run on
// UNDER the staging buffer, which stays where it is, binsort_bins<EPT>() floats in: the block is no larger, the bins may be
// up to three times as many.  The counters are dead before the first key is written (binsort_place_full_two_step), and the
// caller's next sort zeroes them only after this one's read-back.
template <int EPT, bool FULL, bool REM_FIRST = false, int ALIAS_BPL = 0>
__device__ __forceinline__ int wave_sort_binned(float (&key)[EPT], int lane, int n, float* scratch, bool rows) {
  unsigned* cnt = reinterpret_cast<unsigned*>(scratch);
  float* buf = scratch + binsort_bins<EPT>();
  int g = SHW_BINSORT_MAX_RUN + 1;
  if constexpr (FULL && ALIAS_BPL != 0) {
    static_assert(REM_FIRST && ALIAS_BPL % 4 == 0, "counters under the buffer: the headline kernel's form");
    constexpr int NB = 64 * ALIAS_BPL;
    // counters [0, 4 NB) and buffer [4 bins, 4 bins + 256 EPT) both end inside the one block of (bins + 64 EPT) floats
    static_assert(4 * NB <= 4 * (binsort_bins<EPT>() + 64 * EPT), "the counters must end inside the wave's block");
    // ... and so does whatever word the mask of binsort_off can name for a key that is no number (binsort_histogram_full)
    static_assert(next_pow2_c(4 * NB) <= 4 * (binsort_bins<EPT>() + 64 * EPT), "the map's mask must stay inside the block");
    unsigned slot[EPT];
    if (!rows || binsort_keys_fit<EPT>(key)) g = binsort_histogram_full<EPT, NB>(key, lane, cnt, slot);
    if (g <= SHW_BINSORT_MAX_RUN) {
      binsort_place_full_two_step<EPT>(key, slot, lane, g, buf);
      return g;
    }
  } else if constexpr (FULL) {
    unsigned slot[EPT];
    if (!rows || binsort_keys_fit<EPT>(key)) g = binsort_histogram_full<EPT>(key, lane, cnt, slot);
    if (g <= SHW_BINSORT_MAX_RUN) {
      binsort_place_full<EPT, REM_FIRST>(key, slot, lane, g, buf);
      return g;
    }
  } else {
    g = binsort_histogram<EPT, FULL>(key, lane, n, cnt);
    if (g <= SHW_BINSORT_MAX_RUN) {
      binsort_place<EPT, FULL>(key, lane, n, g, cnt, buf);
      return g;
    }
  }
#ifndef SHW_ABL_NO_FALLBACK
  if constexpr (is_pow2(EPT)) wave_sort<EPT>(key, lane);
  else wave_sort_relayout<EPT, float>(key, lane, __builtin_inff(), buf);
#endif
  return g;
}

}  // namespace shw
