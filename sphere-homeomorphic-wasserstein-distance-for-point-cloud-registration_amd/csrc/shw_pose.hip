// shw_pose.hip -- what a refinement iteration of PCRNet does after the trunk (include/shw.h shw_pose_*):
//
//   pose head    (B, emb), (B, emb) -> (B, 7): six linear layers 2 emb -> w1 -> ... -> w5 -> 7 on the concatenation (never
//                formed), a ReLU after the first five.  Parameters: one flat buffer W1 (w1, 2 emb) row-major, b1, ..., W6, b6.
//   pose update  q = v[0:4] / max(|v[0:4]|, 1e-12), t = v[4:7], rot(x) = x + 2 (w u x x + u x (u x x)), R = [rot(e_j)]:
//                est_R' = R est_R, est_t' = est_t R^T + t, source'_n = rot(source_n) + t.
//
// HEAD LAYOUT.  A layer is a skinny product, batch x K against O x K.  Every product of the unit -- forward Z = W X,
// backward data G = W^T dZ, backward weights dW = dZ X^T -- runs on 32 x 32 tiles of v_mfma_f32_32x32x2_f32, the exact
// f32 instruction: lane (i, h) = (lane & 31, lane >> 5) gives A[row i][k = 2 s + h] and B[k = 2 s + h][col i] of step s,
// and accumulator register r holds row (r & 3) + 8 (r >> 2) + 4 h of column i.  A wave is a workgroup and owns one tile
// over one slice of the summed index; the slices' partial tiles are written as SLABS [slice][feature][batch] and the
// consumer adds them in ascending slice order while it loads its operand, with the bias and the ReLU (forward) or the
// ReLU mask (backward).  So bias, ReLU and mask cost no launch, every sum has one fixed order and there are no atomics.
// Between the layers everything is stored [feature][batch] with the batch padded to 32 (Bp): the batch is then the
// lane index of every operand load and every slab store, which are 128-byte rows; only the weight operand of the
// forward is a gather (a lane walks its own row of W, a cache line serves sixteen steps).
//
// The forward saves the five hidden activations (after the ReLU, [feature][Bp]): the backward takes X and the mask from them.
#include <hip/hip_runtime.h>

#include "../../include/shw.h"
#include "wave_reduce.hpp"

namespace shw {

typedef float pose_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kHeadLayers = 6, kHeadOut = 7, kHeadTile = 32;
constexpr int kHeadMinWidth = 32, kHeadMaxWidth = 2048;
constexpr int kHeadMaxSlabs = 16;       // slices of the summed index per tile: the consumer pays one load per slab
constexpr int kHeadWaves = 512;         // waves a launch aims at: two per CU

struct HeadShape {
  int in[kHeadLayers], out[kHeadLayers];
  long offW[kHeadLayers], offB[kHeadLayers], params;
  bool ok;
};

inline bool head_width_ok(int w) { return w >= kHeadMinWidth && w <= kHeadMaxWidth && w % kHeadTile == 0; }

inline HeadShape head_shape(int emb, int w1, int w2, int w3, int w4, int w5) {
  HeadShape s;
  const int w[5] = {w1, w2, w3, w4, w5};
  s.ok = head_width_ok(emb);
  for (int l = 0; l < 5; ++l) s.ok = s.ok && head_width_ok(w[l]);
  long off = 0;
  for (int l = 0; l < kHeadLayers; ++l) {
    s.in[l] = l == 0 ? 2 * emb : w[l - 1];
    s.out[l] = l == 5 ? kHeadOut : w[l];
    s.offW[l] = off;
    off += s.ok ? (long)s.in[l] * s.out[l] : 0;
    s.offB[l] = off;
    off += s.ok ? s.out[l] : 0;
  }
  s.params = off;
  return s;
}

// the summed index, `chunks` tiles of 32 long, is cut into slices of `per` chunks for a product of `tiles` output tiles
struct Slicing { int slices, per; };
inline Slicing head_slicing(int tiles, int chunks) {
  int want = kHeadWaves / tiles;
  if (want > kHeadMaxSlabs) want = kHeadMaxSlabs;
  if (want > chunks) want = chunks;
  if (want < 1) want = 1;
  Slicing s;
  s.per = (chunks + want - 1) / want;
  s.slices = (chunks + s.per - 1) / s.per;
  return s;
}
inline int tiles_of(int n) { return (n + kHeadTile - 1) / kHeadTile; }
inline long head_padded_batch(long clouds) { return (clouds + kHeadTile - 1) / kHeadTile * kHeadTile; }

// floats of one slab buffer of the forward (layer outputs) and of the backward (layer inputs), largest layer
inline long head_slab_floats(const HeadShape& s, long Bp, bool backward) {
  long most = 0;
  for (int l = 0; l < kHeadLayers; ++l) {
    const Slicing c = backward ? head_slicing(tiles_of(s.in[l]), tiles_of(s.out[l]))
                               : head_slicing(tiles_of(s.out[l]), tiles_of(s.in[l]));
    const long n = (long)c.slices * (backward ? s.in[l] : s.out[l]) * Bp;
    if (n > most) most = n;
  }
  return most;
}
inline long head_saved_floats(const HeadShape& s, long Bp) {
  long n = 0;
  for (int l = 0; l < 5; ++l) n += (long)s.out[l] * Bp;
  return n;
}

// A [feature][batch] matrix as an operand: where its entry (f, b) comes from
enum : int {
  kSrcPlain = 0,     // p[f fs + b bs]
  kSrcConcat = 1,    // f < split ? p[b split + f] : q[b split + f - split]: the two feature tensors, row-major
  kSrcAct = 2,       // relu(sum over the slabs p[t stride + f fs + b] + bias[f]): a hidden activation
  kSrcGrad = 3       // mask[f fs + b] > 0 ? sum over the slabs : 0: the gradient at a hidden pre-activation
};
struct Src {
  const float* p;
  const float* q;
  const float* bias;
  const float* mask;
  long fs, bs, stride;
  int kind, slabs, features, split;
};

// sixteen entries at once: (f0 + j fstep, b0 + j bstep), j = 0..15 -- the operand values of sixteen MFMA steps.  All
// loads of one slab are issued before any is used, so a chunk of sixteen steps waits for memory once per slab and not once
// per step.  An entry outside the matrix is 0 and is not loaded.
__device__ __forceinline__ void fetch16(const Src& s, int f0, int fstep, long b0, int bstep, long batch, float (&v)[16]) {
  bool ok[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) ok[j] = f0 + j * fstep < s.features && b0 + j * bstep < batch;
  if (s.kind == kSrcPlain) {
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = ok[j] ? s.p[(f0 + j * fstep) * s.fs + (b0 + j * bstep) * s.bs] : 0.f;
    return;
  }
  if (s.kind == kSrcConcat) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int f = f0 + j * fstep;
      const long b = b0 + j * bstep;
      v[j] = !ok[j] ? 0.f : f < s.split ? s.p[b * s.split + f] : s.q[b * s.split + f - s.split];
    }
    return;
  }
  const long first = f0 * s.fs + b0, step = fstep * s.fs + bstep;
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = ok[j] ? s.p[first + j * step] : 0.f;
  for (int t = 1; t < s.slabs; ++t) {
    const float* __restrict__ slab = s.p + t * s.stride;
    float add[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) add[j] = ok[j] ? slab[first + j * step] : 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] += add[j];
  }
  if (s.kind == kSrcAct) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float z = v[j] + (ok[j] ? s.bias[f0 + j * fstep] : 0.f);
      v[j] = z < 0.f ? 0.f : z;
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = ok[j] && s.mask[first + j * step] > 0.f ? v[j] : 0.f;
}

__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ pose_f32x16 zero16() {
  pose_f32x16 a;
#pragma unroll
  for (int r = 0; r < 16; ++r) a[r] = 0.f;
  return a;
}

// ------------------------------------------------------------------------------------------------ head, forward
struct HeadForwardArgs {
  const float* W;       // (O, K) row-major
  Src x;                // the layer's input [K][batch]
  float* slab;          // out: [slices][O][Bp]
  float* save;          // out or null: x as [K][Bp], written by the waves of output tile 0
  long batch, Bp;
  int O, K, slices, per;
};

__global__ __launch_bounds__(64) void pose_head_forward_kernel(const HeadForwardArgs a) {
  const int i = threadIdx.x & 31, h = threadIdx.x >> 5;
  const int tile = blockIdx.x / a.slices, slice = blockIdx.x % a.slices;
  const int k0 = slice * a.per * kHeadTile;
  const int k1 = min(a.K, k0 + a.per * kHeadTile);
  const int o = tile * kHeadTile + i;
  const bool live = o < a.O;
  const float* __restrict__ wrow = a.W + (long)(live ? o : 0) * a.K;
  const bool saves = a.save != nullptr && tile == 0;
  for (long b0 = 0; b0 < a.Bp; b0 += kHeadTile) {
    pose_f32x16 acc = zero16();
    for (int kc = k0; kc < k1; kc += kHeadTile) {     // K is a multiple of 32: no chunk is partial
      float w[16], v[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) w[j] = live ? wrow[kc + 2 * j + h] : 0.f;
      fetch16(a.x, kc + h, 2, b0 + i, 0, a.batch, v);
      if (saves) {
#pragma unroll
        for (int j = 0; j < 16; ++j) a.save[(kc + 2 * j + h) * a.Bp + b0 + i] = v[j];
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j], v[j], acc, 0, 0, 0);
    }
    float* __restrict__ out = a.slab + (long)slice * a.O * a.Bp + b0 + i;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = tile * kHeadTile + acc_row(r, h);
      if (row < a.O) out[row * a.Bp] = acc[r];
    }
  }
}

// out (batch, 7) = the last layer's slabs added in ascending order, plus its bias
__global__ __launch_bounds__(256) void pose_head_finish_kernel(const float* __restrict__ slab, const float* __restrict__ bias,
                                                             int slabs, long batch, long Bp, float* __restrict__ out) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= batch * kHeadOut) return;
  const long b = id / kHeadOut;
  const int o = (int)(id % kHeadOut);
  float v = slab[o * Bp + b];
  for (int t = 1; t < slabs; ++t) v += slab[((long)t * kHeadOut + o) * Bp + b];
  out[id] = v + bias[o];
}

// ------------------------------------------------------------------------------------------------ head, backward
struct HeadBackwardArgs {
  const float* W;       // (O, K) row-major
  Src dz;               // gradient at the layer's pre-activation [O][batch]
  Src x;                // the layer's input [K][batch]
  float* gslab;         // out: gradient at the layer's input, [slices][K][Bp]
  float* dW;            // out or null: (O, K)
  float* db;            // out: (O), with dW
  long batch, Bp;
  int O, K, slices, per, data_blocks;
};

// workgroups [0, data_blocks): G[k][b] = sum over o of W[o][k] dz[o][b], one 32 x 32 tile of G over one slice of o;
// the rest: dW[o][k] = sum over b of dz[o][b] x[k][b], one tile over the whole batch, and db from the tiles of k-tile 0
__global__ __launch_bounds__(64) void pose_head_backward_kernel(const HeadBackwardArgs a) {
  const int i = threadIdx.x & 31, h = threadIdx.x >> 5;
  if ((int)blockIdx.x < a.data_blocks) {
    const int tile = blockIdx.x / a.slices, slice = blockIdx.x % a.slices;
    const int o0 = slice * a.per * kHeadTile;
    const int o1 = min(a.O, o0 + a.per * kHeadTile);
    const float* __restrict__ wcol = a.W + tile * kHeadTile + i;
    for (long b0 = 0; b0 < a.Bp; b0 += kHeadTile) {
      pose_f32x16 acc = zero16();
      for (int oc = o0; oc < o1; oc += kHeadTile) {   // o1 is a.O or a multiple of 32: dz is 0 from a.O on
        float w[16], v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = oc + 2 * j + h < a.O ? wcol[(long)(oc + 2 * j + h) * a.K] : 0.f;
        fetch16(a.dz, oc + h, 2, b0 + i, 0, a.batch, v);
#pragma unroll
        for (int j = 0; j < 16; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j], v[j], acc, 0, 0, 0);
      }
      float* __restrict__ out = a.gslab + ((long)slice * a.K + tile * kHeadTile) * a.Bp + b0 + i;
#pragma unroll
      for (int r = 0; r < 16; ++r) out[acc_row(r, h) * a.Bp] = acc[r];
    }
    return;
  }
  const int id = blockIdx.x - a.data_blocks;
  const int ktiles = a.K / kHeadTile;
  const int otile = id / ktiles, ktile = id % ktiles;
  pose_f32x16 acc = zero16();
  float bias = 0.f;
  for (long bc = 0; bc < a.batch; bc += kHeadTile) {
    float d[16], v[16];
    fetch16(a.dz, otile * kHeadTile + i, 0, bc + h, 2, a.batch, d);
    fetch16(a.x, ktile * kHeadTile + i, 0, bc + h, 2, a.batch, v);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      bias += d[j];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(d[j], v[j], acc, 0, 0, 0);
    }
  }
  float* __restrict__ out = a.dW + (long)otile * kHeadTile * a.K + ktile * kHeadTile + i;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = acc_row(r, h);
    if (otile * kHeadTile + row < a.O) out[(long)row * a.K] = acc[r];
  }
  if (ktile == 0) {
    bias += __shfl_xor(bias, 32);                       // the even clouds' sum plus the odd clouds' sum
    if (h == 0 && otile * kHeadTile + i < a.O) a.db[otile * kHeadTile + i] = bias;
  }
}

// gtf (batch, emb), gsf (batch, emb): the first layer's input-gradient slabs added in ascending order; either may be null
__global__ __launch_bounds__(256) void pose_head_feature_grad_kernel(const float* __restrict__ gslab, int slabs, long batch,
                                                                    long Bp, int emb, float* __restrict__ gtf,
                                                                    float* __restrict__ gsf) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= batch * 2 * emb) return;
  const long b = id / (2 * emb);
  const int f = (int)(id % (2 * emb));
  float* __restrict__ out = f < emb ? gtf : gsf;
  if (!out) return;
  float v = gslab[f * Bp + b];
  for (int t = 1; t < slabs; ++t) v += gslab[((long)t * 2 * emb + f) * Bp + b];
  out[b * emb + (f < emb ? f : f - emb)] = v;
}

// ------------------------------------------------------------------------------------------------ pose update
constexpr int kPoseBlock = 256;
constexpr int kPoseMaxBlocks = 64;      // backward: workgroups per cloud = partial sums per cloud
constexpr int kPoseSums = 12;           // sum g (3), sum g x^T (9, row-major)
constexpr float kPoseEps = 1e-12f;      // F.normalize's clamp

inline int pose_backward_blocks(long points) {
  const long tiles = (points + kPoseBlock - 1) / kPoseBlock;
  return (int)(tiles < kPoseMaxBlocks ? tiles : kPoseMaxBlocks);
}

struct Quat { float w, u[3], t[3], norm; };             // the unit quaternion, the translation, |v[0:4]|

__device__ __forceinline__ Quat load_pose(const float* __restrict__ v) {
  Quat q;
  q.norm = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
  const float d = fmaxf(q.norm, kPoseEps);
  q.w = v[0] / d;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    q.u[c] = v[1 + c] / d;
    q.t[c] = v[4 + c];
  }
  return q;
}

__device__ __forceinline__ void cross3(const float (&a)[3], const float (&b)[3], float (&o)[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// x + 2 (w u x x + u x (u x x))
__device__ __forceinline__ void rotate(const Quat& q, const float (&x)[3], float (&o)[3]) {
  float uv[3], uuv[3];
  cross3(q.u, x, uv);
  cross3(q.u, uv, uuv);
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = x[c] + 2.f * (q.w * uv[c] + uuv[c]);
}

// R[c][j] = rot(e_j)[c]
__device__ __forceinline__ void rotation_matrix(const Quat& q, float (&R)[3][3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float e[3] = {j == 0 ? 1.f : 0.f, j == 1 ? 1.f : 0.f, j == 2 ? 1.f : 0.f};
    float col[3];
    rotate(q, e, col);
#pragma unroll
    for (int c = 0; c < 3; ++c) R[c][j] = col[c];
  }
}

struct Point3 { float c[3]; };

__global__ __launch_bounds__(kPoseBlock) void pose_update_forward_kernel(const float* __restrict__ vector,
                                                                        const float* __restrict__ est_R,
                                                                        const float* __restrict__ est_t,
                                                                        const float* __restrict__ source, long points,
                                                                        float* __restrict__ est_R_out,
                                                                        float* __restrict__ est_t_out,
                                                                        float* __restrict__ source_out) {
  const long b = blockIdx.y;
  const Quat q = load_pose(vector + b * 7);
  if (blockIdx.x == 0 && threadIdx.x < 12) {
    float R[3][3];
    rotation_matrix(q, R);
    // lane 3 c + j writes est_R'[c][j] = (R est_R)[c][j], lane 9 + c writes est_t'[c] = (est_t R^T + t)[c]; the row of R
    // is picked by selects, so R stays in registers with compile-time indices
    const int e = threadIdx.x, c = e < 9 ? e / 3 : e - 9;
    float row[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) row[m] = c == 0 ? R[0][m] : c == 1 ? R[1][m] : R[2][m];
    const float* __restrict__ in = e < 9 ? est_R + b * 9 + e % 3 : est_t + b * 3;
    const int stride = e < 9 ? 3 : 1;
    float acc = 0.f;
#pragma unroll
    for (int m = 0; m < 3; ++m) acc = fmaf(row[m], in[m * stride], acc);
    if (e < 9)
      est_R_out[b * 9 + e] = acc;
    else
      est_t_out[b * 3 + c] = acc + (c == 0 ? q.t[0] : c == 1 ? q.t[1] : q.t[2]);
  }
  const long n = (long)blockIdx.x * kPoseBlock + threadIdx.x;
  if (n >= points) return;
  const Point3 x = reinterpret_cast<const Point3*>(source)[b * points + n];
  Point3 y;
  rotate(q, x.c, y.c);
#pragma unroll
  for (int c = 0; c < 3; ++c) y.c[c] += q.t[c];
  reinterpret_cast<Point3*>(source_out)[b * points + n] = y;
}

// workgroup (x, b): g_source = R^T g over its point tiles x, x + gridDim.x, ...; its sums of g and of g x^T go to
// partial[b][x][12].  The per-lane sums run in tile order, the wave's by transpose_reduce, the four waves' in wave order.
__global__ __launch_bounds__(kPoseBlock) void pose_update_backward_points_kernel(const float* __restrict__ vector,
                                                                                const float* __restrict__ source,
                                                                                const float* __restrict__ g_out,
                                                                                long points, float* __restrict__ g_source,
                                                                                float* __restrict__ partial) {
  __shared__ float sh[kPoseBlock / 64][16];
  const long b = blockIdx.y;
  const Quat q = load_pose(vector + b * 7);
  float R[3][3];
  rotation_matrix(q, R);
  float sums[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) sums[e] = 0.f;
  for (long n = (long)blockIdx.x * kPoseBlock + threadIdx.x; n < points; n += (long)gridDim.x * kPoseBlock) {
    const Point3 g = reinterpret_cast<const Point3*>(g_out)[b * points + n];
    if (g_source) {
      Point3 o;
#pragma unroll
      for (int j = 0; j < 3; ++j) o.c[j] = R[0][j] * g.c[0] + R[1][j] * g.c[1] + R[2][j] * g.c[2];
      reinterpret_cast<Point3*>(g_source)[b * points + n] = o;
    }
    if (partial) {
      const Point3 x = reinterpret_cast<const Point3*>(source)[b * points + n];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        sums[c] += g.c[c];
#pragma unroll
        for (int j = 0; j < 3; ++j) sums[3 + 3 * c + j] = fmaf(g.c[c], x.c[j], sums[3 + 3 * c + j]);
      }
    }
  }
  if (!partial) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float r = transpose_reduce<16>(sums, lane);
  if (lane < 16) sh[wave][lane] = r;
  __syncthreads();
  if (threadIdx.x < kPoseSums) {
    float t = sh[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kPoseBlock / 64; ++w) t += sh[w][threadIdx.x];
    partial[(b * gridDim.x + blockIdx.x) * kPoseSums + threadIdx.x] = t;
  }
}

// one lane per cloud: the partial sums in ascending order, the cotangents of est_R' and est_t' folded in, then the
// gradient of the seven numbers through the rotation, the quaternion and its normalisation, and those of est_R, est_t
__global__ __launch_bounds__(64) void pose_update_backward_pose_kernel(const float* __restrict__ vector,
                                                                      const float* __restrict__ est_R,
                                                                      const float* __restrict__ est_t,
                                                                      const float* __restrict__ g_R_out,
                                                                      const float* __restrict__ g_t_out,
                                                                      const float* __restrict__ partial, int blocks,
                                                                      long clouds, float* __restrict__ g_vector,
                                                                      float* __restrict__ g_est_R,
                                                                      float* __restrict__ g_est_t) {
  const long b = (long)blockIdx.x * 64 + threadIdx.x;
  if (b >= clouds) return;
  const float* __restrict__ v = vector + b * 7;
  const Quat q = load_pose(v);
  float R[3][3];
  rotation_matrix(q, R);
  float gt[3] = {0.f, 0.f, 0.f}, G[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  if (partial)
    for (int k = 0; k < blocks; ++k) {
      const float* __restrict__ p = partial + (b * blocks + k) * kPoseSums;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        gt[c] += p[c];
#pragma unroll
        for (int j = 0; j < 3; ++j) G[c][j] += p[3 + 3 * c + j];
      }
    }
  float gR[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}}, gto[3] = {0.f, 0.f, 0.f};
  if (g_R_out) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int j = 0; j < 3; ++j) gR[c][j] = g_R_out[b * 9 + 3 * c + j];
  }
  if (g_t_out) {
#pragma unroll
    for (int c = 0; c < 3; ++c) gto[c] = g_t_out[b * 3 + c];
  }
  if (g_est_R) {                                        // R^T g_est_R'
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
      for (int j = 0; j < 3; ++j) g_est_R[b * 9 + 3 * m + j] = R[0][m] * gR[0][j] + R[1][m] * gR[1][j] + R[2][m] * gR[2][j];
  }
  if (g_est_t) {                                        // g_est_t' R
#pragma unroll
    for (int m = 0; m < 3; ++m) g_est_t[b * 3 + m] = gto[0] * R[0][m] + gto[1] * R[1][m] + gto[2] * R[2][m];
  }
  if (!g_vector) return;
  // the gradient of R: sum g x^T + g_est_R' est_R^T + g_est_t'^T est_t
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    gt[c] += gto[c];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      float acc = G[c][m];
#pragma unroll
      for (int j = 0; j < 3; ++j) acc = fmaf(gR[c][j], est_R[b * 9 + 3 * m + j], acc);
      G[c][m] = fmaf(gto[c], est_t[b * 3 + m], acc);
    }
  }
  // R = I + 2 w [u]x + 2 (u u^T - |u|^2 I):  d/dw = 2 u . a,  d/du = 2 w a + 2 (G + G^T) u - 4 tr(G) u,
  // a = (G21 - G12, G02 - G20, G10 - G01)
  const float a[3] = {G[2][1] - G[1][2], G[0][2] - G[2][0], G[1][0] - G[0][1]};
  const float trace = G[0][0] + G[1][1] + G[2][2];
  float gq[4];
  gq[0] = 2.f * (q.u[0] * a[0] + q.u[1] * a[1] + q.u[2] * a[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float sym = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) sym = fmaf(G[k][j] + G[j][k], q.u[j], sym);
    gq[1 + k] = 2.f * (q.w * a[k] + sym) - 4.f * trace * q.u[k];
  }
  // through q = v / max(|v|, eps): (g - q (q . g)) / |v| above the clamp, g / eps at or below it
  const float qh[4] = {q.w, q.u[0], q.u[1], q.u[2]};
  if (q.norm > kPoseEps) {
    const float dot = qh[0] * gq[0] + qh[1] * gq[1] + qh[2] * gq[2] + qh[3] * gq[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) g_vector[b * 7 + k] = (gq[k] - qh[k] * dot) / q.norm;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) g_vector[b * 7 + k] = gq[k] / kPoseEps;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) g_vector[b * 7 + 4 + c] = gt[c];
}

inline Src plain_src(const float* p, long fs, long bs, int features) {
  Src s = {p, nullptr, nullptr, nullptr, fs, bs, 0, kSrcPlain, 1, features, 0};
  return s;
}

}  // namespace shw

extern "C" {

int shw_pose_head_supported(int emb, int w1, int w2, int w3, int w4, int w5) {
  return shw::head_shape(emb, w1, w2, w3, w4, w5).ok ? 1 : 0;
}

size_t shw_pose_head_param_count(int emb, int w1, int w2, int w3, int w4, int w5) {
  const shw::HeadShape s = shw::head_shape(emb, w1, w2, w3, w4, w5);
  return s.ok ? (size_t)s.params : 0;
}

size_t shw_pose_head_workspace_bytes(long clouds, int emb, int w1, int w2, int w3, int w4, int w5, int which) {
  const shw::HeadShape s = shw::head_shape(emb, w1, w2, w3, w4, w5);
  if (!s.ok || clouds < 1 || which < 0 || which > 2) return 0;
  const long Bp = shw::head_padded_batch(clouds);
  if (which == 2) return (size_t)shw::head_saved_floats(s, Bp) * sizeof(float);
  return (size_t)2 * shw::head_slab_floats(s, Bp, which == 1) * sizeof(float);
}

int shw_pose_head_forward(const float* tf, const float* sf, const float* params, long clouds, int emb, int w1, int w2, int w3,
                          int w4, int w5, float* out, float* saved, void* workspace, void* stream) {
  const shw::HeadShape s = shw::head_shape(emb, w1, w2, w3, w4, w5);
  if (!s.ok || clouds < 1 || clouds > 0x7fffffffL / 16 || !tf || !sf || !params || !out || !saved || !workspace)
    return (int)hipErrorInvalidValue;
  const hipStream_t st = (hipStream_t)stream;
  const long Bp = shw::head_padded_batch(clouds);
  const long slab_floats = shw::head_slab_floats(s, Bp, false);
  float* slab[2] = {(float*)workspace, (float*)workspace + slab_floats};
  int prev_slices = 0;
  float* act = saved;
  for (int l = 0; l < shw::kHeadLayers; ++l) {
    const shw::Slicing c = shw::head_slicing(shw::tiles_of(s.out[l]), shw::tiles_of(s.in[l]));
    shw::HeadForwardArgs a;
    a.W = params + s.offW[l];
    if (l == 0) {
      const shw::Src x = {tf, sf, nullptr, nullptr, 0, 0, 0, shw::kSrcConcat, 1, s.in[0], emb};
      a.x = x;
      a.save = nullptr;
    } else {
      const shw::Src x = {slab[(l - 1) & 1], nullptr, params + s.offB[l - 1], nullptr, Bp, 1, (long)s.in[l] * Bp,
                          shw::kSrcAct, prev_slices, s.in[l], 0};
      a.x = x;
      a.save = act;
      act += (long)s.in[l] * Bp;
    }
    a.slab = slab[l & 1];
    a.batch = clouds;
    a.Bp = Bp;
    a.O = s.out[l];
    a.K = s.in[l];
    a.slices = c.slices;
    a.per = c.per;
    hipLaunchKernelGGL(shw::pose_head_forward_kernel, dim3((unsigned)(shw::tiles_of(s.out[l]) * c.slices)), dim3(64), 0, st,
                       a);
    const int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    prev_slices = c.slices;
  }
  const long outputs = clouds * shw::kHeadOut;
  hipLaunchKernelGGL(shw::pose_head_finish_kernel, dim3((unsigned)((outputs + 255) / 256)), dim3(256), 0, st,
                     (const float*)slab[(shw::kHeadLayers - 1) & 1], params + s.offB[shw::kHeadLayers - 1], prev_slices,
                     clouds, Bp, out);
  return (int)hipGetLastError();
}

int shw_pose_head_backward(const float* tf, const float* sf, const float* params, const float* saved, const float* gout,
                           long clouds, int emb, int w1, int w2, int w3, int w4, int w5, float* gtf, float* gsf,
                           float* gparams, void* workspace, void* stream) {
  const shw::HeadShape s = shw::head_shape(emb, w1, w2, w3, w4, w5);
  if (!s.ok || clouds < 1 || clouds > 0x7fffffffL / 16 || !tf || !sf || !params || !saved || !gout || !workspace)
    return (int)hipErrorInvalidValue;
  if (!gtf && !gsf && !gparams) return 0;
  const hipStream_t st = (hipStream_t)stream;
  const long Bp = shw::head_padded_batch(clouds);
  const long slab_floats = shw::head_slab_floats(s, Bp, true);
  float* gslab[2] = {(float*)workspace, (float*)workspace + slab_floats};
  const float* act[shw::kHeadLayers];                   // act[l]: the input of layer l, [in[l]][Bp], l >= 1
  act[0] = nullptr;
  for (int l = 1; l < shw::kHeadLayers; ++l) act[l] = l == 1 ? saved : act[l - 1] + (long)s.in[l - 1] * Bp;
  int prev_slices = 0;
  for (int l = shw::kHeadLayers - 1; l >= 0; --l) {
    const bool data = l > 0 || gtf || gsf;
    if (!data && !gparams) break;
    const shw::Slicing c = shw::head_slicing(shw::tiles_of(s.in[l]), shw::tiles_of(s.out[l]));
    shw::HeadBackwardArgs a;
    a.W = params + s.offW[l];
    if (l == shw::kHeadLayers - 1) {
      a.dz = shw::plain_src(gout, 1, shw::kHeadOut, shw::kHeadOut);
    } else {                                            // the slabs the layer above wrote, masked by this layer's output
      const shw::Src dz = {gslab[(l + 1) & 1], nullptr, nullptr, act[l + 1], Bp, 1, (long)s.out[l] * Bp, shw::kSrcGrad,
                           prev_slices, s.out[l], 0};
      a.dz = dz;
    }
    if (l == 0) {
      const shw::Src x = {tf, sf, nullptr, nullptr, 0, 0, 0, shw::kSrcConcat, 1, s.in[0], emb};
      a.x = x;
    } else {
      a.x = shw::plain_src(act[l], Bp, 1, s.in[l]);
    }
    a.gslab = gslab[l & 1];
    a.dW = gparams ? gparams + s.offW[l] : nullptr;
    a.db = gparams ? gparams + s.offB[l] : nullptr;
    a.batch = clouds;
    a.Bp = Bp;
    a.O = s.out[l];
    a.K = s.in[l];
    a.slices = c.slices;
    a.per = c.per;
    a.data_blocks = data ? shw::tiles_of(s.in[l]) * c.slices : 0;
    const int weight_blocks = gparams ? shw::tiles_of(s.out[l]) * shw::tiles_of(s.in[l]) : 0;
    hipLaunchKernelGGL(shw::pose_head_backward_kernel, dim3((unsigned)(a.data_blocks + weight_blocks)), dim3(64), 0, st, a);
    const int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    prev_slices = c.slices;
  }
  if (gtf || gsf) {
    const long entries = clouds * 2 * emb;
    hipLaunchKernelGGL(shw::pose_head_feature_grad_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st,
                       (const float*)gslab[0], prev_slices, clouds, Bp, emb, gtf, gsf);
    return (int)hipGetLastError();
  }
  return 0;
}

int shw_pose_update_backward_blocks(long points) { return points <= 0 ? 0 : shw::pose_backward_blocks(points); }

size_t shw_pose_update_workspace_bytes(long clouds, long points) {
  if (clouds < 1 || points < 1) return 0;
  return (size_t)clouds * shw::pose_backward_blocks(points) * shw::kPoseSums * sizeof(float);
}

int shw_pose_update_forward(const float* vector, const float* est_R, const float* est_t, const float* source, long clouds,
                            long points, float* est_R_out, float* est_t_out, float* source_out, void* stream) {
  if (clouds < 1 || clouds > 65535 || points < 1 || points > 0x7fffffffL || !vector || !est_R || !est_t || !source ||
      !est_R_out || !est_t_out || !source_out)
    return (int)hipErrorInvalidValue;
  const long tiles = (points + shw::kPoseBlock - 1) / shw::kPoseBlock;
  hipLaunchKernelGGL(shw::pose_update_forward_kernel, dim3((unsigned)tiles, (unsigned)clouds), dim3(shw::kPoseBlock), 0,
                     (hipStream_t)stream, vector, est_R, est_t, source, points, est_R_out, est_t_out, source_out);
  return (int)hipGetLastError();
}

int shw_pose_update_backward(const float* vector, const float* est_R, const float* est_t, const float* source,
                             const float* g_est_R_out, const float* g_est_t_out, const float* g_source_out, long clouds,
                             long points, float* g_vector, float* g_est_R, float* g_est_t, float* g_source, void* workspace,
                             void* stream) {
  if (clouds < 1 || clouds > 65535 || points < 1 || points > 0x7fffffffL || !vector || !est_R || !est_t || !source)
    return (int)hipErrorInvalidValue;
  const bool sums = g_vector && g_source_out;
  if (sums && !workspace) return (int)hipErrorInvalidValue;
  const hipStream_t st = (hipStream_t)stream;
  const int blocks = shw::pose_backward_blocks(points);
  if (g_source && !g_source_out) {                      // no cotangent reaches the points
    const int rc = (int)hipMemsetAsync(g_source, 0, (size_t)clouds * points * 3 * sizeof(float), st);
    if (rc != 0) return rc;
  }
  if (g_source_out && (g_source || sums)) {
    hipLaunchKernelGGL(shw::pose_update_backward_points_kernel, dim3((unsigned)blocks, (unsigned)clouds),
                       dim3(shw::kPoseBlock), 0, st, vector, source, g_source_out, points, g_source,
                       sums ? (float*)workspace : (float*)nullptr);
    const int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
  }
  if (!g_vector && !g_est_R && !g_est_t) return 0;
  hipLaunchKernelGGL(shw::pose_update_backward_pose_kernel, dim3((unsigned)((clouds + 63) / 64)), dim3(64), 0, st, vector,
                     est_R, est_t, g_est_R_out, g_est_t_out, sums ? (const float*)workspace : (const float*)nullptr, blocks,
                     clouds, g_vector, g_est_R, g_est_t);
  return (int)hipGetLastError();
}

}  // extern "C"
