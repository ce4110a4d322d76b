// shw_pointnet.hip -- the registration network's trunk: the shared point MLP 3 -> 64 -> 64 -> 64 -> 128 -> emb of PCRNet
// (1x1 convolutions with ReLU) fused with the max-pool over the points (include/shw.h shw_pointnet_*).
//
// max_i relu(z_i) = relu(max_i z_i): the last layer keeps (max, arg-max) per channel and never stores its output, and
// the backward recomputes the four hidden layers on the arg-max points only -- one row per (cloud, channel).
//
// LAYOUT: channels are the MFMA rows, points (forward) or rows (backward) the MFMA columns, so an activation tile sits
// with its point on the lane and its 32 channels in the 16 accumulator registers of the two lane halves.  The exact-f32
// instruction v_mfma_f32_32x32x2_f32 takes ONE k-pair per issue, k = lane >> 5, so accumulator register r of a tile --
// channel (r & 3) + 8 (r >> 2) in the lower half, that + 4 in the upper -- is, as it stands, the B operand of one k-step
// of the next layer; the A operand is the weight W[out = lane & 31][that same channel], four consecutive floats per four
// registers.  Layers 2..5 chain with no LDS and no lane movement, in a permuted but fixed summation order.
//
// Forward: a wave is a workgroup and takes 64 points (two tiles of 32) of one cloud through layers 1..4, then walks the
// emb / 32 row tiles of layer 5; per row tile the two point tiles are folded in-lane and the 32 lanes of each half by a
// transpose-reduce on (value, index) pairs (16 exchanges for 16 registers).  Per-tile partials go to the workspace and a
// second kernel folds them in ascending tile order; ties go to the lowest index everywhere.
//
// Backward: a wave takes the 32 rows (cloud b, channels 32 g .. 32 g + 31) for a contiguous range of b.  dW5 and db5 are
// in-lane sums over b; the hidden layers' parameter gradients are contractions over the rows, done on the MFMA from an
// LDS image [channel][row] of dz and of the layer input, and added to the workgroup's own partial vector.  Fixed-order
// reduction kernels follow; the point gradient is scattered by a kernel that adds the channels of a point in ascending
// order.  No float atomics: the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/shw.h"

namespace shw {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kPnMinEmb = 32, kPnMaxEmb = 2048;
constexpr int kPnPointTiles = 2;                    // forward: 32-point tiles per wave
constexpr int kPnPoints = 32 * kPnPointTiles;       // ... = the point tile P
// packed parameters: W1 (64, 3) b1 W2 (64, 64) b2 W3 (64, 64) b3 W4 (128, 64) b4 W5 (emb, 128) b5
constexpr int kOffW1 = 0, kOffB1 = 192, kOffW2 = 256, kOffB2 = 4352, kOffW3 = 4416, kOffB3 = 8512, kOffW4 = 8576,
              kOffB4 = 16768, kOffW5 = 16896;
constexpr int kPnTrunk = kOffW5;                    // floats before W5: what the backward's partial vectors hold
constexpr long kPnBackwardBlocks = 1024;            // backward: about this many workgroups = partial vectors (69 MB)
constexpr int kPnLd = 33;                           // LDS images [channel][row]: 32 rows + 1

inline bool pointnet_shape_ok(int dim, int emb) {
  return dim == 3 && emb >= kPnMinEmb && emb <= kPnMaxEmb && emb % 32 == 0;
}
inline long pointnet_param_count(int emb) { return kPnTrunk + (long)emb * 129; }
inline long pointnet_tiles(long points) { return (points + kPnPoints - 1) / kPnPoints; }

struct PnBackwardPlan { long groups, chunk_len, chunks, blocks; };
inline PnBackwardPlan pointnet_backward_plan(long clouds, int emb) {
  PnBackwardPlan p;
  p.groups = emb / 32;
  long want = kPnBackwardBlocks / p.groups;
  want = want < 1 ? 1 : want > clouds ? clouds : want;
  p.chunk_len = (clouds + want - 1) / want;
  p.chunks = (clouds + p.chunk_len - 1) / p.chunk_len;
  p.blocks = p.groups * p.chunks;
  return p;
}
// floats of the backward's workspace regions, in order: rowdx, trunk partials, W5 partials, b5 partials
inline void pointnet_backward_regions(long clouds, int emb, const PnBackwardPlan& p, long (&n)[4]) {
  n[0] = clouds * emb * 3;
  n[1] = p.blocks * kPnTrunk;
  n[2] = p.chunks * emb * 128;
  n[3] = p.chunks * emb;
}

// channel (within its tile of 32) of accumulator register r in lane half h
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// layer 1 (K = 3) on the VALU, straight into the accumulator layout: out[j][r] = relu(W1[k] . x + b1[k]), k = 32 j + acc_row
__device__ __forceinline__ void layer1(const float* __restrict__ P, float x0, float x1, float x2, int h, f32x16 (&out)[2]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = 32 * j + 8 * q + 4 * h;
      const f32x4* __restrict__ w = reinterpret_cast<const f32x4*>(P + kOffW1 + 3 * k);
      const f32x4 w0 = w[0], w1 = w[1], w2 = w[2];
      const f32x4 b = *reinterpret_cast<const f32x4*>(P + kOffB1 + k);
      const float wv[12] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3], w2[0], w2[1], w2[2], w2[3]};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float z = fmaf(wv[3 * e + 2], x2, fmaf(wv[3 * e + 1], x1, fmaf(wv[3 * e], x0, b[e])));
        out[j][4 * q + e] = fmaxf(z, 0.f);
      }
    }
  }
}

// acc[r] = bias[row0 + acc_row(r, h)]
__device__ __forceinline__ void bias_init(const float* __restrict__ bias, int row0, int h, f32x16& acc) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 b = *reinterpret_cast<const f32x4*>(bias + row0 + 8 * q + 4 * h);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[4 * q + e] = b[e];
  }
}

// acc[u] += W[row0 .. row0 + 31][:] . in[u]: W row-major (rows, 32 KT), in[u] KT accumulator-layout tiles of PT point tiles
template <int KT, int PT>
__device__ __forceinline__ void mfma_rows(const float* __restrict__ W, int row0, int i, int h, const f32x16 (&in)[PT][KT],
                                          f32x16 (&acc)[PT]) {
  const float* __restrict__ wrow = W + (long)(row0 + i) * (32 * KT) + 4 * h;
#pragma unroll
  for (int j = 0; j < KT; ++j) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(wrow + 32 * j + 8 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int u = 0; u < PT; ++u)
          acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], in[u][j][4 * q + e], acc[u], 0, 0, 0);
      }
    }
  }
}

// acc += W^T[row0 .. row0 + 31][:] . in: W row-major (32 KT, 64); the backward's data path
template <int KT>
__device__ __forceinline__ void mfma_rows_t(const float* __restrict__ W, int row0, int i, int h, const f32x16 (&in)[KT],
                                            f32x16& acc) {
  const float* __restrict__ w = W + row0 + i + 4 * h * 64;
#pragma unroll
  for (int j = 0; j < KT; ++j) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float a = w[(32 * j + (r & 3) + 8 * (r >> 2)) * 64];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, in[j][r], acc, 0, 0, 0);
    }
  }
}

__device__ __forceinline__ f32x16 relu16(const f32x16& a) {
  f32x16 o;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = fmaxf(a[r], 0.f);
  return o;
}

// layers 1..4 of PT point tiles: h1, h2, h3 (two tiles each) and h4 (four)
template <int PT>
__device__ __forceinline__ void trunk_hidden(const float* __restrict__ P, const float (&x)[PT][3], int i, int h,
                                             f32x16 (&h1)[PT][2], f32x16 (&h2)[PT][2], f32x16 (&h3)[PT][2],
                                             f32x16 (&h4)[PT][4]) {
#pragma unroll
  for (int u = 0; u < PT; ++u) layer1(P, x[u][0], x[u][1], x[u][2], h, h1[u]);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    f32x16 acc[PT];
#pragma unroll
    for (int u = 0; u < PT; ++u) bias_init(P + kOffB2, 32 * t, h, acc[u]);
    mfma_rows<2, PT>(P + kOffW2, 32 * t, i, h, h1, acc);
#pragma unroll
    for (int u = 0; u < PT; ++u) h2[u][t] = relu16(acc[u]);
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    f32x16 acc[PT];
#pragma unroll
    for (int u = 0; u < PT; ++u) bias_init(P + kOffB3, 32 * t, h, acc[u]);
    mfma_rows<2, PT>(P + kOffW3, 32 * t, i, h, h2, acc);
#pragma unroll
    for (int u = 0; u < PT; ++u) h3[u][t] = relu16(acc[u]);
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    f32x16 acc[PT];
#pragma unroll
    for (int u = 0; u < PT; ++u) bias_init(P + kOffB4, 32 * t, h, acc[u]);
    mfma_rows<2, PT>(P + kOffW4, 32 * t, i, h, h3, acc);
#pragma unroll
    for (int u = 0; u < PT; ++u) h4[u][t] = relu16(acc[u]);
  }
}

// (value, index) b replaces a when it is larger, or equal with the lower index; a NaN on either side keeps a
__device__ __forceinline__ bool takes_over(float bv, int bi, float av, int ai) { return bv > av || (bv == av && bi < ai); }

// ------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(64) void pointnet_forward_kernel(const float* __restrict__ x, const float* __restrict__ P,
                                                             long points, long tiles, int emb,
                                                             float* __restrict__ pval, int* __restrict__ pidx) {
  constexpr int PT = kPnPointTiles;
  const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
  const long cloud = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  float xin[PT][3];
  int index[PT];
  bool valid[PT];
#pragma unroll
  for (int u = 0; u < PT; ++u) {
    const long p = tile * kPnPoints + 32 * u + i;
    valid[u] = p < points;                        // a padded column computes on the cloud's last point and never wins
    index[u] = (int)(valid[u] ? p : points - 1);
    const float* __restrict__ src = x + (cloud * points + index[u]) * 3;
    xin[u][0] = src[0];
    xin[u][1] = src[1];
    xin[u][2] = src[2];
  }
  f32x16 h1[PT][2], h2[PT][2], h3[PT][2], h4[PT][4];
  trunk_hidden<PT>(P, xin, i, h, h1, h2, h3, h4);
  const float* __restrict__ W5 = P + kOffW5;
  const float* __restrict__ b5 = W5 + (long)emb * 128;
  float* __restrict__ out_v = pval + (long)blockIdx.x * emb;
  int* __restrict__ out_i = pidx + (long)blockIdx.x * emb;
  for (int t = 0; t < emb / 32; ++t) {
    f32x16 acc[PT];
#pragma unroll
    for (int u = 0; u < PT; ++u) bias_init(b5, 32 * t, h, acc[u]);
    mfma_rows<4, PT>(W5, 32 * t, i, h, h4, acc);
    // fold the point tiles in-lane (the lower tile holds the lower indices: strictly larger takes over) ...
    float v[16];
    int ix[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      v[r] = valid[0] ? acc[0][r] : -INFINITY;
      ix[r] = index[0];
#pragma unroll
      for (int u = 1; u < PT; ++u) {
        const float vu = valid[u] ? acc[u][r] : -INFINITY;
        if (vu > v[r]) { v[r] = vu; ix[r] = index[u]; }
      }
    }
    // ... and the 32 lanes of the half: step s halves the registers over lane bit s, lane L ends with register L & 15
    int s = 0;
#pragma unroll
    for (int n = 16; n > 1; n >>= 1, ++s) {
      const bool odd = (lane >> s) & 1;
#pragma unroll
      for (int m = 0; m < n / 2; ++m) {
        const float kv = odd ? v[2 * m + 1] : v[2 * m], sv = odd ? v[2 * m] : v[2 * m + 1];
        const int ki = odd ? ix[2 * m + 1] : ix[2 * m], si = odd ? ix[2 * m] : ix[2 * m + 1];
        const float ov = __shfl_xor(sv, 1 << s);
        const int oi = __shfl_xor(si, 1 << s);
        const bool take = takes_over(ov, oi, kv, ki);
        v[m] = take ? ov : kv;
        ix[m] = take ? oi : ki;
      }
    }
    {
      const float ov = __shfl_xor(v[0], 16);
      const int oi = __shfl_xor(ix[0], 16);
      if (takes_over(ov, oi, v[0], ix[0])) { v[0] = ov; ix[0] = oi; }
    }
    if ((lane & 16) == 0) {
      const int c = 32 * t + acc_row(lane & 15, h);
      out_v[c] = v[0];
      out_i[c] = ix[0];
    }
  }
}

// the tiles of a cloud in ascending order: a later tile takes over only when strictly larger
__global__ __launch_bounds__(256) void pointnet_fold_kernel(const float* __restrict__ pval, const int* __restrict__ pidx,
                                                           long clouds, long tiles, int emb, float* __restrict__ feat,
                                                           int* __restrict__ argmax) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= clouds * emb) return;
  const long cloud = g / emb, c = g % emb;
  const long first = cloud * tiles * emb + c;
  float best = pval[first];
  int at = pidx[first];
  for (long t = 1; t < tiles; ++t) {
    const float v = pval[first + t * emb];
    if (v > best) { best = v; at = pidx[first + t * emb]; }
  }
  feat[g] = best > 0.f ? best : 0.f;
  argmax[g] = at;
}

// ------------------------------------------------------------------------------------------------ backward
// tile[j][r] -> image[(32 j + acc_row(r, h)) * kPnLd + i]
template <int KT>
__device__ __forceinline__ void store_image(float* __restrict__ image, const f32x16 (&tile)[KT], int i, int h) {
#pragma unroll
  for (int j = 0; j < KT; ++j) {
#pragma unroll
    for (int r = 0; r < 16; ++r) image[(32 * j + acc_row(r, h)) * kPnLd + i] = tile[j][r];
  }
}

// dW (32 TO, 32 TK) = sum over the 32 rows of dz (x) in, from the LDS images; db (32 TO) = row sums of dz; both added to
// (first: stored in) the workgroup's partial vector
template <int TO, int TK>
__device__ __forceinline__ void layer_param_grads(const float* __restrict__ dimg, const float* __restrict__ himg,
                                                  float* __restrict__ dW, float* __restrict__ db, int lane, bool first) {
  const int i = lane & 31, h = lane >> 5;
#pragma unroll 1
  for (int to = 0; to < TO; ++to) {
#pragma unroll 1
    for (int tk = 0; tk < TK; ++tk) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int s = 0; s < 16; ++s)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dimg[(32 * to + i) * kPnLd + 2 * s + h],
                                                   himg[(32 * tk + i) * kPnLd + 2 * s + h], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float* q = dW + (32 * to + acc_row(r, h)) * (32 * TK) + 32 * tk + i;
        *q = first ? acc[r] : *q + acc[r];
      }
    }
  }
  for (int c = lane; c < 32 * TO; c += 64) {
    float sum = 0.f;
#pragma unroll
    for (int row = 0; row < 32; ++row) sum += dimg[c * kPnLd + row];
    db[c] = first ? sum : db[c] + sum;
  }
}

template <bool WANT_P, bool WANT_X>
__global__ __launch_bounds__(64) void pointnet_backward_kernel(
    const float* __restrict__ x, const float* __restrict__ params, const float* __restrict__ feat,
    const int* __restrict__ argmax, const float* __restrict__ gfeat, long clouds, long points, int emb, long groups,
    long chunk_len, float* __restrict__ rowdx, float* __restrict__ part, float* __restrict__ w5part,
    float* __restrict__ b5part) {
  __shared__ float dimg[128 * kPnLd];
  __shared__ float himg[64 * kPnLd];
  __shared__ float ximg[3 * kPnLd];
  const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
  const long group = blockIdx.x % groups, chunk = blockIdx.x / groups;
  const long c = 32 * group + i;
  const long b0 = chunk * chunk_len, b1 = b0 + chunk_len < clouds ? b0 + chunk_len : clouds;
  float* const mine = WANT_P ? part + (long)blockIdx.x * kPnTrunk : nullptr;
  f32x16 dw5[4];
  float db5 = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int r = 0; r < 16; ++r) dw5[j][r] = 0.f;
  }
  for (long b = b0; b < b1; ++b) {
    const bool first = b == b0;
    // the weights are re-read per cloud: hoisted out of this loop they would not fit the register file
    const float* P = params;
    asm volatile("" : "+s"(P));
    const float* __restrict__ W5row = P + kOffW5 + c * 128 + 4 * h;
    const float gin = gfeat[b * emb + c];
    const bool live = feat[b * emb + c] > 0.f && gin != 0.f;      // relu passes nothing at 0
    const float g = live ? gin : 0.f;
    long at = argmax[b * emb + c];
    at = at < 0 ? 0 : at >= points ? points - 1 : at;
    const float* __restrict__ src = x + (b * points + at) * 3;
    float xin[1][3] = {{src[0], src[1], src[2]}};
    f32x16 h1[1][2], h2[1][2], h3[1][2], h4[1][4];
    trunk_hidden<1>(P, xin, i, h, h1, h2, h3, h4);
    // layer 5 is one-hot per row: dz4 = g W5[c, :] where h4 > 0, dW5[c, :] += g h4, db5[c] += g
    f32x16 dz4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(W5row + 32 * j + 8 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float a = h4[0][j][4 * q + e];
          dz4[j][4 * q + e] = live && a > 0.f ? g * w[e] : 0.f;
          if (WANT_P) dw5[j][4 * q + e] = fmaf(g, a, dw5[j][4 * q + e]);
        }
      }
    }
    db5 += g;
    f32x16 dz3[2], dz2[2], dz1[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      mfma_rows_t<4>(P + kOffW4, 32 * t, i, h, dz4, acc);
#pragma unroll
      for (int r = 0; r < 16; ++r) dz3[t][r] = h3[0][t][r] > 0.f ? acc[r] : 0.f;
    }
    if (WANT_P) {                                    // each layer's images as soon as its dz is no longer needed in registers
      __syncthreads();                               // the previous cloud's images are read out
      store_image<4>(dimg, dz4, i, h);
      store_image<2>(himg, h3[0], i, h);
      __syncthreads();
      layer_param_grads<4, 2>(dimg, himg, mine + kOffW4, mine + kOffB4, lane, first);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      mfma_rows_t<2>(P + kOffW3, 32 * t, i, h, dz3, acc);
#pragma unroll
      for (int r = 0; r < 16; ++r) dz2[t][r] = h2[0][t][r] > 0.f ? acc[r] : 0.f;
    }
    if (WANT_P) {
      __syncthreads();
      store_image<2>(dimg, dz3, i, h);
      store_image<2>(himg, h2[0], i, h);
      __syncthreads();
      layer_param_grads<2, 2>(dimg, himg, mine + kOffW3, mine + kOffB3, lane, first);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      mfma_rows_t<2>(P + kOffW2, 32 * t, i, h, dz2, acc);
#pragma unroll
      for (int r = 0; r < 16; ++r) dz1[t][r] = h1[0][t][r] > 0.f ? acc[r] : 0.f;
    }
    if (WANT_P) {
      __syncthreads();
      store_image<2>(dimg, dz2, i, h);
      store_image<2>(himg, h1[0], i, h);
      __syncthreads();
      layer_param_grads<2, 2>(dimg, himg, mine + kOffW2, mine + kOffB2, lane, first);
      __syncthreads();
      store_image<2>(dimg, dz1, i, h);
      if (h == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) ximg[d * kPnLd + i] = xin[0][d];
      }
      __syncthreads();
      {                                              // layer 1 on the VALU: lane = channel
        float sw[3] = {0.f, 0.f, 0.f}, sb = 0.f;
#pragma unroll
        for (int row = 0; row < 32; ++row) {
          const float d = dimg[lane * kPnLd + row];
          sb += d;
#pragma unroll
          for (int e = 0; e < 3; ++e) sw[e] = fmaf(d, ximg[e * kPnLd + row], sw[e]);
        }
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          float* q = mine + kOffW1 + 3 * lane + e;
          *q = first ? sw[e] : *q + sw[e];
        }
        float* q = mine + kOffB1 + lane;
        *q = first ? sb : *q + sb;
      }
    }
    if (WANT_X) {
      // dx = W1^T dz1: this half's 32 channels in register order, then the other half's
      float dx[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = 32 * j + 8 * q + 4 * h;
          const f32x4* __restrict__ w = reinterpret_cast<const f32x4*>(P + kOffW1 + 3 * k);
          const f32x4 w0 = w[0], w1 = w[1], w2 = w[2];
          const float wv[12] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3], w2[0], w2[1], w2[2], w2[3]};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int d = 0; d < 3; ++d) dx[d] = fmaf(wv[3 * e + d], dz1[j][4 * q + e], dx[d]);
          }
        }
      }
#pragma unroll
      for (int d = 0; d < 3; ++d) dx[d] += __shfl_xor(dx[d], 32);
      if (h == 0) {
        float* __restrict__ dst = rowdx + (b * emb + c) * 3;
        dst[0] = dx[0];
        dst[1] = dx[1];
        dst[2] = dx[2];
      }
    }
  }
  if (WANT_P) {
    float* __restrict__ dst = w5part + (chunk * emb + c) * 128 + 4 * h;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = dw5[j][4 * q + e];
        *reinterpret_cast<f32x4*>(dst + 32 * j + 8 * q) = o;
      }
    }
    if (h == 0) b5part[chunk * emb + c] = db5;
  }
}

// gparams[0 .. kPnTrunk) = the workgroups' partial vectors summed, in ascending order within each of 16 interleaved
// slices and then over the slices
__global__ __launch_bounds__(256) void pointnet_trunk_reduce_kernel(const float* __restrict__ partial, int vectors,
                                                                   float* __restrict__ out) {
  __shared__ float sh[16][17];
  const int c = threadIdx.x & 15, s = threadIdx.x >> 4;
  const long p = (long)blockIdx.x * 16 + c;
  float acc = 0.f;
  if (p < kPnTrunk)
    for (int b = s; b < vectors; b += 16) acc += partial[(long)b * kPnTrunk + p];
  sh[s][c] = acc;
  __syncthreads();
  if (s == 0 && p < kPnTrunk) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += sh[k][c];
    out[p] = t;
  }
}

// gparams[kOffW5 ..): dW5 (emb, 128) then db5 (emb), the cloud ranges in ascending order
__global__ __launch_bounds__(256) void pointnet_head_reduce_kernel(const float* __restrict__ w5part,
                                                                  const float* __restrict__ b5part, long chunks, int emb,
                                                                  float* __restrict__ out) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  const long nw = (long)emb * 128;
  if (p >= nw + emb) return;
  const float* __restrict__ src = p < nw ? w5part + p : b5part + (p - nw);
  const long stride = p < nw ? nw : emb;
  float acc = src[0];
  for (long k = 1; k < chunks; ++k) acc += src[k * stride];
  out[p] = acc;
}

// gx (zeroed by the caller): the lowest live channel of every arg-max point adds up the rows of that point in ascending
// channel order and stores the sum.  A thread is a channel; the cloud's arg-max row sits in LDS and is scanned four
// entries at a time, below the channel for an earlier owner of the point, above it for the rows to add.
constexpr int kPnScatterBlock = 256;
__global__ __launch_bounds__(kPnScatterBlock) void pointnet_scatter_kernel(const float* __restrict__ rowdx,
                                                                          const float* __restrict__ feat,
                                                                          const int* __restrict__ argmax,
                                                                          const float* __restrict__ gfeat, long points,
                                                                          int emb, int parts, float* __restrict__ gx) {
  __shared__ __attribute__((aligned(16))) int at[kPnMaxEmb];
  const long b = blockIdx.x / parts;
  const int c = (int)(blockIdx.x % parts) * kPnScatterBlock + threadIdx.x;
  for (int k = threadIdx.x; k < emb; k += kPnScatterBlock) {
    const long row = b * emb + k;
    const bool live = feat[row] > 0.f && gfeat[row] != 0.f;
    const int a = argmax[row];
    at[k] = live && a >= 0 && a < points ? a : -1;
  }
  __syncthreads();
  if (c >= emb) return;
  const int mine = at[c];
  if (mine < 0) return;
  const int4* __restrict__ at4 = reinterpret_cast<const int4*>(at);
  bool earlier = false;
  for (int k4 = 0; k4 < (c >> 2); ++k4) {
    const int4 a = at4[k4];
    earlier |= (a.x == mine) | (a.y == mine) | (a.z == mine) | (a.w == mine);
  }
  for (int k = c & ~3; k < c; ++k) earlier |= at[k] == mine;
  if (earlier) return;
  const float* __restrict__ rows = rowdx + b * emb * 3;
  float s0 = rows[3 * c], s1 = rows[3 * c + 1], s2 = rows[3 * c + 2];
  auto add = [&](int k) {
    s0 += rows[3 * k];
    s1 += rows[3 * k + 1];
    s2 += rows[3 * k + 2];
  };
  const int next = (c | 3) + 1;                    // emb is a multiple of 32: the group of c is whole
  for (int k = c + 1; k < next; ++k)
    if (at[k] == mine) add(k);
  for (int k4 = next >> 2; k4 < (emb >> 2); ++k4) {
    const int4 a = at4[k4];
    if ((a.x == mine) | (a.y == mine) | (a.z == mine) | (a.w == mine)) {
      if (a.x == mine) add(4 * k4);
      if (a.y == mine) add(4 * k4 + 1);
      if (a.z == mine) add(4 * k4 + 2);
      if (a.w == mine) add(4 * k4 + 3);
    }
  }
  float* __restrict__ dst = gx + (b * points + mine) * 3;
  dst[0] = s0;
  dst[1] = s1;
  dst[2] = s2;
}

inline bool pointnet_sizes_ok(long clouds, long points, int emb) {
  if (clouds < 1 || points < 1 || points > 0x7fffffffL) return false;
  const long tiles = pointnet_tiles(points);
  // every launch's grid and every element count below 2^31
  return clouds <= 0x7fffffffL / tiles && clouds * tiles <= 0x7fffffffL / emb && clouds <= 0x7fffffffL / (3L * emb) &&
         clouds <= (1L << 40) / points;
}

}  // namespace shw

extern "C" {

int shw_pointnet_supported(int dim, int emb) { return shw::pointnet_shape_ok(dim, emb) ? 1 : 0; }

size_t shw_pointnet_param_count(int emb) {
  return shw::pointnet_shape_ok(3, emb) ? (size_t)shw::pointnet_param_count(emb) : 0;
}

size_t shw_pointnet_workspace_bytes(long clouds, long points, int emb, int backward) {
  if (!shw::pointnet_shape_ok(3, emb) || !shw::pointnet_sizes_ok(clouds, points, emb)) return 0;
  if (!backward) return (size_t)(clouds * shw::pointnet_tiles(points) * emb) * (sizeof(float) + sizeof(int));
  long n[4];
  shw::pointnet_backward_regions(clouds, emb, shw::pointnet_backward_plan(clouds, emb), n);
  return (size_t)(n[0] + n[1] + n[2] + n[3]) * sizeof(float);
}

int shw_pointnet_forward(const float* x, const float* params, long clouds, long points, int emb, float* feat, int* argmax,
                         void* workspace, void* stream) {
  if (!shw::pointnet_shape_ok(3, emb) || !shw::pointnet_sizes_ok(clouds, points, emb)) return (int)hipErrorInvalidValue;
  if (!x || !params || !feat || !argmax || !workspace) return (int)hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(params) & 15) != 0) return (int)hipErrorInvalidValue;    // 16-byte weight loads
  const hipStream_t st = (hipStream_t)stream;
  const long tiles = shw::pointnet_tiles(points);
  float* pval = static_cast<float*>(workspace);
  int* pidx = reinterpret_cast<int*>(pval + clouds * tiles * emb);
  hipLaunchKernelGGL(shw::pointnet_forward_kernel, dim3((unsigned)(clouds * tiles)), dim3(64), 0, st, x, params, points,
                     tiles, emb, pval, pidx);
  int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  hipLaunchKernelGGL(shw::pointnet_fold_kernel, dim3((unsigned)((clouds * emb + 255) / 256)), dim3(256), 0, st,
                     (const float*)pval, (const int*)pidx, clouds, tiles, emb, feat, argmax);
  return (int)hipGetLastError();
}

int shw_pointnet_backward(const float* x, const float* params, const float* feat, const int* argmax, const float* gfeat,
                          long clouds, long points, int emb, float* gx, float* gparams, void* workspace, void* stream) {
  if (!shw::pointnet_shape_ok(3, emb) || !shw::pointnet_sizes_ok(clouds, points, emb)) return (int)hipErrorInvalidValue;
  if (!x || !params || !feat || !argmax || !gfeat) return (int)hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(params) & 15) != 0) return (int)hipErrorInvalidValue;
  if (!gx && !gparams) return 0;
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return (int)hipErrorInvalidValue;
  const hipStream_t st = (hipStream_t)stream;
  const shw::PnBackwardPlan plan = shw::pointnet_backward_plan(clouds, emb);
  long n[4];
  shw::pointnet_backward_regions(clouds, emb, plan, n);
  float* rowdx = static_cast<float*>(workspace);
  float* part = rowdx + n[0];
  float* w5part = part + n[1];
  float* b5part = w5part + n[2];
  const dim3 grid((unsigned)plan.blocks), block(64);
#define SHW_PN_BACKWARD(P_, X_)                                                                                          \
  hipLaunchKernelGGL((shw::pointnet_backward_kernel<P_, X_>), grid, block, 0, st, x, params, feat, argmax, gfeat, clouds, \
                     points, emb, plan.groups, plan.chunk_len, rowdx, part, w5part, b5part)
  if (gparams && gx) SHW_PN_BACKWARD(true, true);
  else if (gparams) SHW_PN_BACKWARD(true, false);
  else SHW_PN_BACKWARD(false, true);
#undef SHW_PN_BACKWARD
  int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  if (gparams) {
    hipLaunchKernelGGL(shw::pointnet_trunk_reduce_kernel, dim3((shw::kPnTrunk + 15) / 16), dim3(256), 0, st,
                       (const float*)part, (int)plan.blocks, gparams);
    if ((rc = (int)hipGetLastError()) != 0) return rc;
    hipLaunchKernelGGL(shw::pointnet_head_reduce_kernel, dim3((unsigned)(((long)emb * 129 + 255) / 256)), dim3(256), 0, st,
                       (const float*)w5part, (const float*)b5part, plan.chunks, emb, gparams + shw::kOffW5);
    if ((rc = (int)hipGetLastError()) != 0) return rc;
  }
  if (gx) {
    rc = (int)hipMemsetAsync(gx, 0, (size_t)(clouds * points) * 3 * sizeof(float), st);
    if (rc != 0) return rc;
    const int parts = (emb + shw::kPnScatterBlock - 1) / shw::kPnScatterBlock;
    hipLaunchKernelGGL(shw::pointnet_scatter_kernel, dim3((unsigned)(clouds * parts)), dim3(shw::kPnScatterBlock), 0, st,
                       (const float*)rowdx, feat, argmax, gfeat, points, emb, parts, gx);
    rc = (int)hipGetLastError();
  }
  return rc;
}

}  // extern "C"
