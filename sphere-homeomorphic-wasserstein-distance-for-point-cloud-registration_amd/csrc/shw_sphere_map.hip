// shw_sphere_map.hip -- the sphere encoder of the phi-max wrappers: per point x in R^3,
//     z1 = tanh(W1 x + b1) (16),  z2 = tanh(W2 z1 + b2) (4),  o = W3 z2 + b3 (2),
//     theta1 = pi (tanh(o0) / 2 + 1/2),  theta2 = pi tanh(o1),
//     y = (sin theta1 cos theta2, sin theta1 sin theta2, cos theta1)
// (include/shw.h shw_sphere_map_*).  The 142 parameters are one flat buffer in state-dict order: W1
// row-major (16, 3), b1, W2 (4, 16), b2, W3 (2, 4), b3.
//
// One point per lane, the widths compile-time so that every activation sits in a register with a compile-time index; no
// LDS.  Parameter addresses depend on nothing per lane: the reads are wave-uniform.  The backward saves nothing from the
// forward but x: it recomputes the 22 activations with their derivatives and back-propagates.  Parameter gradients, as in
// shw_flow.hip: the 142 per-lane contributions are summed over the wave in three groups -- W1 with b1 (64 values), W2
// (64), b2 with W3 and b3 (14) -- by the transpose-reduce of wave_reduce.hpp, one 256-byte store each; a wave is a block,
// each block owns one 142-float partial vector and adds its tiles to it in tile order, and a second kernel sums the
// partial vectors in a fixed order: no float atomics, the same bits on every run.
#include <hip/hip_runtime.h>

#include "../../include/shw.h"
#include "wave_reduce.hpp"

namespace shw {

constexpr int kSphereH1 = 16, kSphereH2 = 4, kSphereOut = 2;
constexpr int kSphereW1 = 0, kSphereB1 = kSphereW1 + 3 * kSphereH1, kSphereW2 = kSphereB1 + kSphereH1,
              kSphereB2 = kSphereW2 + kSphereH1 * kSphereH2, kSphereW3 = kSphereB2 + kSphereH2,
              kSphereB3 = kSphereW3 + kSphereH2 * kSphereOut, kSphereParams = kSphereB3 + kSphereOut;
static_assert(kSphereW2 == 64 && kSphereB2 == 128 && kSphereParams == 142, "the three reduction groups start at 0, 64, 128");
constexpr int kSphereForwardBlock = 256;
constexpr int kSphereMaxBlocks = 1024;        // backward: one wave on each of the 256 x 4 SIMDs, a workspace of 568 KB
constexpr float kPi = 3.14159265358979323846f;

inline bool sphere_map_shape_ok(int dim, int hidden1, int hidden2) {
  return dim == 3 && hidden1 == kSphereH1 && hidden2 == kSphereH2;
}
// blocks of the backward kernel = partial vectors in the workspace
inline long sphere_map_backward_blocks(long points) {
  const long tiles = (points + 63) / 64;
  return tiles < kSphereMaxBlocks ? tiles : kSphereMaxBlocks;
}

// tanh(u) and 1 - tanh(u)^2, both from e = exp(-2 |u|) in [0, 1]: saturation gives exactly +-1 and exactly 0, and no
// inf / inf or inf * 0 can form.
struct Tanh { float t, d; };
__device__ __forceinline__ Tanh tanh_with_slope(float u) {
  const float e = expf(-2.0f * fabsf(u));
  const float q = 1.0f + e;                            // in [1, 2]
  float r = __builtin_amdgcn_rcpf(q);
  r = fmaf(fmaf(-q, r, 1.0f), r, r);                   // one Newton step
  Tanh o;
  o.t = copysignf((1.0f - e) * r, u);
  o.d = 4.0f * e * r * r;
  return o;
}

// sin(pi u) and cos(pi u) for |u| <= 1 (the angles are pi times a tanh, so the argument is known in half turns and the
// reduction is exact): u = k / 2 + r with |r| <= 1/4, polynomials on |pi r| <= pi / 4, then the quadrant.
__device__ __forceinline__ void sincos_pi(float u, float& s, float& c) {
  const float k = rintf(2.0f * u);
  const float a = kPi * fmaf(-0.5f, k, u);
  const float z = a * a;
  const float sp = fmaf(fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f), z * a, a);
  const float cp = fmaf(fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f), z * z,
                        fmaf(-0.5f, z, 1.0f));
  const int q = (int)k;
  const float sq = (q & 1) ? cp : sp, cq = (q & 1) ? sp : cp;
  s = (q & 2) ? -sq : sq;
  c = ((q + 1) & 2) ? -cq : cq;
}

// b + sum_i w[i] z[i] rounded once (Ogita, Rump and Oishi's Dot2: every product and every partial sum hands its rounding
// error on, and the errors are added at the end).  Why the forward affords ten operations per term: a pre-activation feeds
// a chain of tanh whose slopes multiply, so with pre-activations of order 5 the rounding of a plain 16-term fmaf chain
// (a few 1e-7 of the sum) comes out of the gradients as a few 1e-6 of their largest entry -- measured, 2.2e-6 against
// 3e-7 with this sum -- and the kernels are bound by their launches, not by their arithmetic.
template <int IN>
__device__ __forceinline__ float dot_rounded_once(const float* __restrict__ w, const float (&z)[IN], float b) {
#pragma clang fp contract(off)                         // s + p must not become fmaf(w, z, s): e is the error of THAT sum
  float s = b, e = 0.f;
#pragma unroll
  for (int i = 0; i < IN; ++i) {
    const float p = w[i] * z[i];
    const float ep = __builtin_fmaf(w[i], z[i], -p);
    const float t = s + p;
    const float bb = t - s;
    e += ep + ((s - (t - bb)) + (p - bb));
    s = t;
  }
  return s + e;
}

struct Point { float c[3]; };                          // one 12-byte load or store per lane

// what the backward needs of a point: the activations, their slopes, and the sines and cosines of the two angles
struct SphereAct {
  float z1[kSphereH1], d1[kSphereH1], z2[kSphereH2], d2[kSphereH2], dt[kSphereOut], s1, c1, s2, c2;
};

__device__ __forceinline__ void sphere_map_point(const float* __restrict__ P, const float (&x)[3], SphereAct& a) {
#pragma unroll
  for (int j = 0; j < kSphereH1; ++j) {
    const Tanh t = tanh_with_slope(dot_rounded_once<3>(P + kSphereW1 + 3 * j, x, P[kSphereB1 + j]));
    a.z1[j] = t.t;
    a.d1[j] = t.d;
  }
#pragma unroll
  for (int j = 0; j < kSphereH2; ++j) {
    const Tanh t = tanh_with_slope(dot_rounded_once<kSphereH1>(P + kSphereW2 + kSphereH1 * j, a.z1, P[kSphereB2 + j]));
    a.z2[j] = t.t;
    a.d2[j] = t.d;
  }
  float t[kSphereOut];
#pragma unroll
  for (int j = 0; j < kSphereOut; ++j) {
    const Tanh th = tanh_with_slope(dot_rounded_once<kSphereH2>(P + kSphereW3 + kSphereH2 * j, a.z2, P[kSphereB3 + j]));
    t[j] = th.t;
    a.dt[j] = th.d;
  }
  // theta1 = pi / 2 + pi t0 / 2: sin theta1 = cos(pi t0 / 2), cos theta1 = -sin(pi t0 / 2); theta2 = pi t1
  float sh, ch;
  sincos_pi(0.5f * t[0], sh, ch);
  a.s1 = ch;
  a.c1 = -sh;
  sincos_pi(t[1], a.s2, a.c2);
}

__global__ __launch_bounds__(kSphereForwardBlock) void sphere_map_forward_kernel(const float* __restrict__ x,
                                                                                const float* __restrict__ params,
                                                                                long points, float* __restrict__ y) {
  const long p = (long)blockIdx.x * kSphereForwardBlock + threadIdx.x;
  if (p >= points) return;
  const Point in = reinterpret_cast<const Point*>(x)[p];
  SphereAct a;
  sphere_map_point(params, in.c, a);
  Point out;
  out.c[0] = a.s1 * a.c2;
  out.c[1] = a.s1 * a.s2;
  out.c[2] = a.c1;
  reinterpret_cast<Point*>(y)[p] = out;
}

// one group of per-lane contributions summed over the wave and stored (first tile of the block) or added (later tiles)
template <int N>
__device__ __forceinline__ void emit_group(float (&v)[N], int count, float* __restrict__ dst, int lane, bool first) {
  const float r = transpose_reduce<N>(v, lane);
  if (lane < count) {
    float* q = dst + lane;
    *q = first ? r : *q + r;
  }
}

template <bool WANT_P>
__global__ __launch_bounds__(64) void sphere_map_backward_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ params,
                                                                const float* __restrict__ gy, long points,
                                                                float* __restrict__ gx, float* __restrict__ partial) {
  const int lane = threadIdx.x;
  const float* __restrict__ P = params;
  float* mine = nullptr;                        // this block's partial vector
  if constexpr (WANT_P) mine = partial + (long)blockIdx.x * kSphereParams;
  const long tiles = (points + 63) / 64;
  bool first = true;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x, first = false) {
    const long p = tile * 64 + lane;
    const bool live = p < points;                 // a lane past the end carries x = 0, gy = 0: every contribution is 0
    Point in = {{0.f, 0.f, 0.f}}, g = {{0.f, 0.f, 0.f}};
    if (live) {
      in = reinterpret_cast<const Point*>(x)[p];
      g = reinterpret_cast<const Point*>(gy)[p];
    }
    SphereAct a;
    sphere_map_point(P, in.c, a);
    const float dth1 = a.c1 * (g.c[0] * a.c2 + g.c[1] * a.s2) - g.c[2] * a.s1;
    const float dth2 = a.s1 * (g.c[1] * a.c2 - g.c[0] * a.s2);
    const float go[kSphereOut] = {dth1 * (0.5f * kPi) * a.dt[0], dth2 * kPi * a.dt[1]};
    float g2[kSphereH2];                          // gradients at the pre-activations of the second layer
#pragma unroll
    for (int i = 0; i < kSphereH2; ++i) {
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < kSphereOut; ++j) acc = fmaf(P[kSphereW3 + kSphereH2 * j + i], go[j], acc);
      g2[i] = acc * a.d2[i];
    }
    if constexpr (WANT_P) {
      float v[16];                                // b2, W3, b3, two zeros
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int c = kSphereB2 + t;
        if (c < kSphereW3) v[t] = g2[c - kSphereB2];
        else if (c < kSphereB3) v[t] = go[(c - kSphereW3) / kSphereH2] * a.z2[(c - kSphereW3) % kSphereH2];
        else if (c < kSphereParams) v[t] = go[c - kSphereB3];
        else v[t] = 0.f;
      }
      emit_group<16>(v, kSphereParams - kSphereB2, mine + kSphereB2, lane, first);
      float w[64];                                // W2
#pragma unroll
      for (int t = 0; t < 64; ++t) w[t] = g2[t / kSphereH1] * a.z1[t % kSphereH1];
      emit_group<64>(w, 64, mine + kSphereW2, lane, first);
    }
    float g1[kSphereH1];                          // ... of the first layer
#pragma unroll
    for (int i = 0; i < kSphereH1; ++i) {
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < kSphereH2; ++j) acc = fmaf(P[kSphereW2 + kSphereH1 * j + i], g2[j], acc);
      g1[i] = acc * a.d1[i];
    }
    if constexpr (WANT_P) {
      float v[64];                                // W1, b1
#pragma unroll
      for (int t = 0; t < 64; ++t) v[t] = t < kSphereB1 ? g1[t / 3] * in.c[t % 3] : g1[t - kSphereB1];
      emit_group<64>(v, 64, mine + kSphereW1, lane, first);
    }
    if (live && gx) {
      Point out;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < kSphereH1; ++j) acc = fmaf(P[kSphereW1 + 3 * j + c], g1[j], acc);
        out.c[c] = acc;
      }
      reinterpret_cast<Point*>(gx)[p] = out;
    }
  }
}

// out[p] = sum over the partial vectors, in ascending order within each of 16 interleaved slices and then over the slices
__global__ __launch_bounds__(256) void sphere_map_param_reduce_kernel(const float* __restrict__ partial, int vectors,
                                                                     float* __restrict__ out) {
  __shared__ float sh[16][17];
  const int c = threadIdx.x & 15, s = threadIdx.x >> 4;
  const int p = blockIdx.x * 16 + c;
  float acc = 0.f;
  if (p < kSphereParams)
    for (int b = s; b < vectors; b += 16) acc += partial[b * kSphereParams + p];
  sh[s][c] = acc;
  __syncthreads();
  if (s == 0 && p < kSphereParams) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += sh[k][c];
    out[p] = t;
  }
}

}  // namespace shw

extern "C" {

int shw_sphere_map_supported(int dim, int hidden1, int hidden2) {
  return shw::sphere_map_shape_ok(dim, hidden1, hidden2) ? 1 : 0;
}

size_t shw_sphere_map_param_count(int hidden1, int hidden2) {
  return shw::sphere_map_shape_ok(3, hidden1, hidden2) ? (size_t)shw::kSphereParams : 0;
}

int shw_sphere_map_backward_blocks(long points) {
  return points <= 0 ? 0 : (int)shw::sphere_map_backward_blocks(points);
}

size_t shw_sphere_map_workspace_bytes(long points) {
  return points <= 0 ? 0 : (size_t)shw::sphere_map_backward_blocks(points) * shw::kSphereParams * sizeof(float);
}

int shw_sphere_map_forward(const float* x, const float* params, long points, float* y, void* stream) {
  if (points < 0 || !x || !params || !y) return (int)hipErrorInvalidValue;
  if (points == 0) return 0;
  const long blocks = (points + shw::kSphereForwardBlock - 1) / shw::kSphereForwardBlock;
  if (blocks > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(shw::sphere_map_forward_kernel, dim3((unsigned)blocks), dim3(shw::kSphereForwardBlock), 0,
                     (hipStream_t)stream, x, params, points, y);
  return (int)hipGetLastError();
}

int shw_sphere_map_backward(const float* x, const float* params, const float* gy, long points, float* gx, float* gparams,
                            float* workspace, void* stream) {
  if (points < 0 || !x || !params || !gy) return (int)hipErrorInvalidValue;
  if (gparams && points > 0 && !workspace) return (int)hipErrorInvalidValue;
  const hipStream_t st = (hipStream_t)stream;
  if (points == 0)                                            // no point, no contribution
    return gparams ? (int)hipMemsetAsync(gparams, 0, shw::kSphereParams * sizeof(float), st) : 0;
  if (!gx && !gparams) return 0;
  const long blocks = shw::sphere_map_backward_blocks(points);
  if (gparams)
    hipLaunchKernelGGL(shw::sphere_map_backward_kernel<true>, dim3((unsigned)blocks), dim3(64), 0, st, x, params, gy,
                       points, gx, workspace);
  else
    hipLaunchKernelGGL(shw::sphere_map_backward_kernel<false>, dim3((unsigned)blocks), dim3(64), 0, st, x, params, gy,
                       points, gx, (float*)nullptr);
  const int rc = (int)hipGetLastError();
  if (rc != 0 || !gparams) return rc;
  hipLaunchKernelGGL(shw::sphere_map_param_reduce_kernel, dim3((shw::kSphereParams + 15) / 16), dim3(256), 0, st,
                     (const float*)workspace, (int)blocks, gparams);
  return (int)hipGetLastError();
}

}  // extern "C"
