// shw_flow.hip -- the sphere map phi of the trainers: `flows` residual blocks z <- z + MLP(z) on 3-D points, the MLP a
// chain of `layers` pairs [Swish(gamma_k), Linear_k] of width `hidden` (include/shw.h shw_flow_residual_*).
//
// The kernels read PACKED EFFECTIVE parameters: per flow, per layer, gamma_k = softplus(beta_k), then W_eff,k row-major
// (out, in), then b_k.  The spectral normalisation that turns the raw weight into W_eff is a few small operations per
// layer and stays with the caller (flows.py), where autograd carries the gradient of the packed buffer back through it.
//
// One point per lane; `hidden` is a template parameter so that every activation sits in a register with a compile-time
// index, `layers` and `flows` are run-time loops.  Parameter addresses depend on loop counters only: the reads are
// wave-uniform.  The forward keeps two activation vectors.  The backward saves nothing per point between the calls: it
// walks the flows forward once, keeping each flow's entry point in LDS (3 floats per flow and lane), then takes the
// flows last to first, recomputes the flow's layer inputs into LDS (one column per lane, so no barrier and no bank
// conflict) and back-propagates.  Parameter gradients: a layer's 1 + out*in + out per-lane contributions are summed over
// the wave 64 at a time by a transpose-reduce (63 adds and 63 cross-lane moves per 64 values, lane L ends with value L;
// wave_reduce.hpp, shared with shw_sphere_map.hip),
// a wave is a block, each block owns one partial vector of the workspace and adds its tiles to it in order, and a second
// kernel sums the partial vectors in ascending order: no float atomics, the same bits on every run.
#include <hip/hip_runtime.h>

#include "../../include/shw.h"
#include "wave_reduce.hpp"

namespace shw {

constexpr int kFlowMaxHidden = 32, kFlowMinLayers = 2, kFlowMaxLayers = 8, kFlowMaxFlows = 16;
constexpr int kFlowForwardBlock = 256;
constexpr int kFlowMaxBlocks = 2048;          // backward: partial vectors at most (two waves per SIMD)
constexpr int kFlowMinBlocks = 256;           // ... and at least, when there are that many tiles
constexpr long kFlowPartialFloats = 1L << 22; // ... and between the two, a workspace of about 16 MB
constexpr float kSwishScale = 1.0f / 1.1f;

inline bool flow_shape_ok(int dim, int hidden, int layers, int flows) {
  return dim == 3 && hidden >= 1 && hidden <= kFlowMaxHidden && layers >= kFlowMinLayers && layers <= kFlowMaxLayers &&
         flows >= 1 && flows <= kFlowMaxFlows;
}
__host__ __device__ constexpr int flow_first_count(int h) { return 1 + 3 * h + h; }
__host__ __device__ constexpr int flow_mid_count(int h) { return 1 + h * h + h; }
__host__ __device__ constexpr int flow_last_count(int h) { return 1 + 3 * h + 3; }
inline long flow_param_count(int hidden, int layers) {
  return flow_first_count(hidden) + (long)(layers - 2) * flow_mid_count(hidden) + flow_last_count(hidden);
}
// blocks of the backward kernel = partial vectors in the workspace
inline long flow_backward_blocks(long points, long total_params) {
  const long tiles = (points + 63) / 64;
  long cap = kFlowPartialFloats / total_params;
  cap = cap < kFlowMinBlocks ? kFlowMinBlocks : cap > kFlowMaxBlocks ? kFlowMaxBlocks : cap;
  return tiles < cap ? tiles : cap;
}

// x * sigmoid(gamma x) / 1.1 and the two factors its derivatives need.  e = exp(-|t|) never overflows; the sigmoid and
// its complement are both formed from e, so sigmoid(-large) is exactly 0, sigmoid(large) exactly 1, neither loses its
// small side to cancellation, and s * c underflows to 0 instead of producing inf * 0.
struct Swish { float a, s, c; };
__device__ __forceinline__ Swish swish(float x, float gamma) {
  const float t = gamma * x;
  const float e = expf(-fabsf(t));                     // the accurate one: a gradient of beta is a sum that cancels
  const float q = 1.0f + e;                            // in [1, 2]
  float r = __builtin_amdgcn_rcpf(q);
  r = fmaf(fmaf(-q, r, 1.0f), r, r);                   // one Newton step: correctly rounded but for rare last-bit cases
  const float small = e * r;
  Swish o;
  o.s = t >= 0.f ? r : small;
  o.c = t >= 0.f ? small : r;
  o.a = x * o.s * kSwishScale;
  return o;
}

// o = b + W swish(u); p -> gamma, W (OUT, IN) row-major, b
template <int IN, int OUT>
__device__ __forceinline__ void layer_forward(const float* __restrict__ p, const float (&u)[IN], float (&o)[OUT]) {
  const float gamma = p[0];
  const float* __restrict__ W = p + 1;
  const float* __restrict__ b = W + OUT * IN;
  float a[IN];
#pragma unroll
  for (int i = 0; i < IN; ++i) a[i] = swish(u[i], gamma).a;
#pragma unroll
  for (int j = 0; j < OUT; ++j) {
    float acc = b[j];
#pragma unroll
    for (int i = 0; i < IN; ++i) acc = fmaf(W[j * IN + i], a[i], acc);
    o[j] = acc;
  }
}

// one residual block on z; h is left holding the input of the last layer
template <int H>
__device__ __forceinline__ void flow_forward(const float* __restrict__ q, int layers, float (&z)[3]) {
  float h[H];
  layer_forward<3, H>(q, z, h);
  q += flow_first_count(H);
  for (int k = 1; k < layers - 1; ++k) {
    float o[H];
    layer_forward<H, H>(q, h, o);
#pragma unroll
    for (int j = 0; j < H; ++j) h[j] = o[j];
    q += flow_mid_count(H);
  }
  float r[3];
  layer_forward<H, 3>(q, h, r);
#pragma unroll
  for (int c = 0; c < 3; ++c) z[c] += r[c];
}

template <int H>
__global__ __launch_bounds__(kFlowForwardBlock) void flow_forward_kernel(const float* __restrict__ x,
                                                                        const float* __restrict__ params, long points,
                                                                        int layers, int flows, float* __restrict__ y) {
  const long p = (long)blockIdx.x * kFlowForwardBlock + threadIdx.x;
  if (p >= points) return;
  float z[3] = {x[3 * p], x[3 * p + 1], x[3 * p + 2]};
  const long per_flow = flow_first_count(H) + (long)(layers - 2) * flow_mid_count(H) + flow_last_count(H);
  for (int f = 0; f < flows; ++f) flow_forward<H>(params + f * per_flow, layers, z);
  y[3 * p] = z[0];
  y[3 * p + 1] = z[1];
  y[3 * p + 2] = z[2];
}

// the layer's parameter gradients in packed order -- d gamma, d W[j][i] = d[j] a[i], d b[j] = d[j] -- summed over the
// wave 64 at a time and stored (first tile of the block) or added (later tiles) to the block's partial vector
template <int IN, int OUT, int C0>
__device__ __forceinline__ void emit_param_grads(float dgamma, const float (&d)[OUT], const float (&a)[IN],
                                                 float* __restrict__ dst, int lane, bool first) {
  constexpr int TOTAL = 1 + OUT * IN + OUT;
  if constexpr (C0 < TOTAL) {
    constexpr int REM = TOTAL - C0 < 64 ? TOTAL - C0 : 64;
    constexpr int N = flow_pow2_ceil(REM);
    float v[N];
#pragma unroll
    for (int t = 0; t < N; ++t) {
      const int c = C0 + t;
      if (c == 0) v[t] = dgamma;
      else if (c <= OUT * IN) v[t] = d[(c - 1) / IN] * a[(c - 1) % IN];
      else if (c < TOTAL) v[t] = d[c - 1 - OUT * IN];
      else v[t] = 0.f;
    }
    const float r = transpose_reduce<N>(v, lane);
    if (lane < REM) {
      float* q = dst + C0 + lane;
      *q = first ? r : *q + r;
    }
    emit_param_grads<IN, OUT, C0 + 64>(dgamma, d, a, dst, lane, first);
  }
}

// u: the layer's input (before its Swish), d: gradient w.r.t. its output -> du: gradient w.r.t. u
template <int IN, int OUT, bool WANT_P>
__device__ __forceinline__ void layer_backward(const float* __restrict__ p, const float (&u)[IN], const float (&d)[OUT],
                                               float (&du)[IN], float* __restrict__ dst, int lane, bool first) {
  const float gamma = p[0];
  const float* __restrict__ W = p + 1;
  float a[IN];
  float dgamma = 0.f;
#pragma unroll
  for (int i = 0; i < IN; ++i) {
    const Swish w = swish(u[i], gamma);
    a[i] = w.a;
    float da = 0.f;
#pragma unroll
    for (int j = 0; j < OUT; ++j) da = fmaf(W[j * IN + i], d[j], da);
    const float sc = w.s * w.c;
    dgamma = fmaf(da * kSwishScale, u[i] * (u[i] * sc), dgamma);       // d a / d gamma = x^2 s (1 - s) / 1.1
    du[i] = da * kSwishScale * fmaf(gamma * u[i], sc, w.s);            // d a / d x = (s + gamma x s (1 - s)) / 1.1
  }
  if constexpr (WANT_P) emit_param_grads<IN, OUT, 0>(dgamma, d, a, dst, lane, first);
}

// LDS, one column per lane (index * 64 + lane): the flows' entry points [flows][3], then the outputs of layers
// 0 .. layers - 3 of the flow at hand [layers - 2][H]; the input of the last layer stays in registers
inline size_t flow_backward_lds_bytes(int hidden, int layers, int flows) {
  return (size_t)(3 * flows + (layers - 2) * hidden) * 64 * sizeof(float);
}

template <int H, bool WANT_P>
__global__ __launch_bounds__(64) void flow_backward_kernel(const float* __restrict__ x, const float* __restrict__ params,
                                                          const float* __restrict__ gy, long points, int layers,
                                                          int flows, float* __restrict__ gx, float* __restrict__ partial) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x;
  float* const ent = lds + lane;
  float* const act = lds + 3 * flows * 64 + lane;
  const long per_flow = flow_first_count(H) + (long)(layers - 2) * flow_mid_count(H) + flow_last_count(H);
  const long off_last = per_flow - flow_last_count(H);
  float* mine = nullptr;                        // this block's partial vector
  if constexpr (WANT_P) mine = partial + (long)blockIdx.x * per_flow * flows;
  const long tiles = (points + 63) / 64;
  bool first = true;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x, first = false) {
    const long p = tile * 64 + lane;
    const bool live = p < points;                 // a lane past the end carries x = 0, gy = 0: every contribution is 0
    float z[3], g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      z[c] = live ? x[3 * p + c] : 0.f;
      g[c] = live ? gy[3 * p + c] : 0.f;
    }
    for (int f = 0; f < flows; ++f) {
#pragma unroll
      for (int c = 0; c < 3; ++c) ent[(3 * f + c) * 64] = z[c];
      if (f + 1 < flows) flow_forward<H>(params + f * per_flow, layers, z);
    }
    for (int f = flows - 1; f >= 0; --f) {
      const float* __restrict__ qf = params + f * per_flow;
      float* df = nullptr, *df_last = nullptr;
      if constexpr (WANT_P) { df = mine + f * per_flow; df_last = df + off_last; }
#pragma unroll
      for (int c = 0; c < 3; ++c) z[c] = ent[(3 * f + c) * 64];
      float h[H];
      layer_forward<3, H>(qf, z, h);
      for (int k = 1; k < layers - 1; ++k) {
        float o[H];
#pragma unroll
        for (int j = 0; j < H; ++j) act[((k - 1) * H + j) * 64] = h[j];
        layer_forward<H, H>(qf + flow_first_count(H) + (long)(k - 1) * flow_mid_count(H), h, o);
#pragma unroll
        for (int j = 0; j < H; ++j) h[j] = o[j];
      }
      float d[H];
      layer_backward<H, 3, WANT_P>(qf + off_last, h, g, d, df_last, lane, first);
      for (int k = layers - 2; k >= 1; --k) {
        const long off = flow_first_count(H) + (long)(k - 1) * flow_mid_count(H);
        float du[H];
#pragma unroll
        for (int j = 0; j < H; ++j) h[j] = act[((k - 1) * H + j) * 64];
        layer_backward<H, H, WANT_P>(qf + off, h, d, du, WANT_P ? df + off : nullptr, lane, first);
#pragma unroll
        for (int j = 0; j < H; ++j) d[j] = du[j];
      }
      float dz[3];
      layer_backward<3, H, WANT_P>(qf, z, d, dz, df, lane, first);
#pragma unroll
      for (int c = 0; c < 3; ++c) g[c] += dz[c];
    }
    if (live && gx) {
#pragma unroll
      for (int c = 0; c < 3; ++c) gx[3 * p + c] = g[c];
    }
  }
}

// out[p] = sum over the partial vectors, in ascending order within each of 16 interleaved slices and then over the slices
__global__ __launch_bounds__(256) void flow_param_reduce_kernel(const float* __restrict__ partial, int vectors, long count,
                                                               float* __restrict__ out) {
  __shared__ float sh[16][17];
  const int c = threadIdx.x & 15, s = threadIdx.x >> 4;
  const long p = (long)blockIdx.x * 16 + c;
  float acc = 0.f;
  if (p < count)
    for (int b = s; b < vectors; b += 16) acc += partial[b * count + p];
  sh[s][c] = acc;
  __syncthreads();
  if (s == 0 && p < count) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += sh[k][c];
    out[p] = t;
  }
}

template <int H>
static int launch_flow_forward(const float* x, const float* params, long points, int layers, int flows, float* y,
                               hipStream_t st) {
  const long blocks = (points + kFlowForwardBlock - 1) / kFlowForwardBlock;
  hipLaunchKernelGGL(flow_forward_kernel<H>, dim3((unsigned)blocks), dim3(kFlowForwardBlock), 0, st, x, params, points,
                     layers, flows, y);
  return (int)hipGetLastError();
}

template <int H>
static int launch_flow_backward(const float* x, const float* params, const float* gy, long points, int layers, int flows,
                                float* gx, float* partial, long blocks, hipStream_t st) {
  const size_t lds = flow_backward_lds_bytes(H, layers, flows);      // at most 61 440 bytes: under the 64 KB default
  if (partial)
    hipLaunchKernelGGL((flow_backward_kernel<H, true>), dim3((unsigned)blocks), dim3(64), lds, st, x, params, gy, points,
                       layers, flows, gx, partial);
  else
    hipLaunchKernelGGL((flow_backward_kernel<H, false>), dim3((unsigned)blocks), dim3(64), lds, st, x, params, gy, points,
                       layers, flows, gx, partial);
  return (int)hipGetLastError();
}

#define SHW_FLOW_HIDDEN_CASES(X)                                                                                         \
  X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20) X(21)  \
  X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)

}  // namespace shw

extern "C" {

int shw_flow_residual_supported(int dim, int hidden, int layers, int flows) {
  return shw::flow_shape_ok(dim, hidden, layers, flows) ? 1 : 0;
}

size_t shw_flow_residual_param_count(int hidden, int layers) {
  return shw::flow_shape_ok(3, hidden, layers, 1) ? (size_t)shw::flow_param_count(hidden, layers) : 0;
}

size_t shw_flow_residual_workspace_bytes(long points, int hidden, int layers, int flows) {
  if (!shw::flow_shape_ok(3, hidden, layers, flows) || points <= 0) return 0;
  const long total = shw::flow_param_count(hidden, layers) * flows;
  return (size_t)shw::flow_backward_blocks(points, total) * total * sizeof(float);
}

int shw_flow_residual_forward(const float* x, const float* params, long points, int hidden, int layers, int flows,
                              float* y, void* stream) {
  if (!shw::flow_shape_ok(3, hidden, layers, flows) || points < 0) return (int)hipErrorInvalidValue;
  if (!x || !params || !y) return (int)hipErrorInvalidValue;
  if (points == 0) return 0;
  if ((points + shw::kFlowForwardBlock - 1) / shw::kFlowForwardBlock > 0x7fffffffL) return (int)hipErrorInvalidValue;
  const hipStream_t st = (hipStream_t)stream;
  switch (hidden) {
#define X(H) case H: return shw::launch_flow_forward<H>(x, params, points, layers, flows, y, st);
    SHW_FLOW_HIDDEN_CASES(X)
#undef X
    default: return (int)hipErrorInvalidValue;
  }
}

int shw_flow_residual_backward(const float* x, const float* params, const float* gy, long points, int hidden, int layers,
                               int flows, float* gx, float* gparams, void* workspace, void* stream) {
  if (!shw::flow_shape_ok(3, hidden, layers, flows) || points < 0) return (int)hipErrorInvalidValue;
  if (!x || !params || !gy) return (int)hipErrorInvalidValue;
  if (gparams && points > 0 && !workspace) return (int)hipErrorInvalidValue;
  const hipStream_t st = (hipStream_t)stream;
  const long total = shw::flow_param_count(hidden, layers) * flows;
  if (points == 0)                                            // no point, no contribution
    return gparams ? (int)hipMemsetAsync(gparams, 0, (size_t)total * sizeof(float), st) : 0;
  if (!gx && !gparams) return 0;
  const long blocks = shw::flow_backward_blocks(points, total);
  float* partial = gparams ? static_cast<float*>(workspace) : nullptr;
  int rc;
  switch (hidden) {
#define X(H) case H: rc = shw::launch_flow_backward<H>(x, params, gy, points, layers, flows, gx, partial, blocks, st); break;
    SHW_FLOW_HIDDEN_CASES(X)
#undef X
    default: return (int)hipErrorInvalidValue;
  }
  if (rc != 0 || !gparams) return rc;
  hipLaunchKernelGGL(shw::flow_param_reduce_kernel, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, st,
                     (const float*)partial, (int)blocks, total, gparams);
  return (int)hipGetLastError();
}

}  // extern "C"
