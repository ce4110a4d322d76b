// shw_mssw.hip -- the sphere encoder of mini_batch_Residual_MSSW.py with its residual blocks applied forward
// (mssw.py transform_to_sphere(reverse=False); include/shw.h shw_mssw_*): per point (b, n) of a (B, N, 3)
// cloud,
//     h1 = relu(W1 x + b1) (8),  h2 = relu(W2 h1 + b2) (8),  z = W3 h2 + b3 (2),
//     per flow f:  z <- z + W_eff,1 a(W_eff,0 a(z) + c0) + c1,   z <- z * exp(s[f, n]) + t[f, n],
//     theta1 = pi (tanh(z0) / 2 + 1/2),  theta2 = pi tanh(z1),
//     y = (sin theta1 cos theta2, sin theta1 sin theta2, cos theta1),
// a(x) = x sigmoid(gamma x) / 1.1 the Swish of shw_flow.hip.  The scale and shift belong to the POINT INDEX n, not to the
// network: the reference's ActNorm takes its statistics over the batch axis only.
//
// params: the encoder in state-dict order -- W1 row-major (8, 3), b1, W2 (8, 8), b2, W3 (2, 8), b3, 122 floats -- then per
// flow gamma0, W_eff,0 (4, 2), c0 (4), gamma1, W_eff,1 (2, 4), c1 (2), 24 floats.  affine (F, N, 4): (s0, s1, t0, t1).
//
// One point per lane; every width is compile-time, so every activation sits in a register.  Parameter addresses depend on
// nothing per lane: the reads are wave-uniform.  A lane reads one 16-byte group of `affine` per flow.  The forward uses no
// LDS.  The backward saves nothing from the forward but x: it walks forward once, keeping each flow's entry point in LDS
// (2 doubles per flow and lane, one column per lane: no barrier), then takes the flows last to first.  The network up to
// the last scale and shift is float64 arithmetic on the float32 data ("WHY DOUBLE" below).
// Gradients of the parameters, as in shw_sphere_map.hip: per-lane contributions are summed over the wave by the
// transpose-reduce of wave_reduce.hpp in groups of 32 or 64, a wave is a block, each block owns one partial vector and
// adds its tiles to it in tile order, and a second kernel sums the partial vectors in a fixed order.  Gradients of
// `affine` are sums over the batch axis only: every point writes its (gs0, gs1, gt0, gt1) per flow into the workspace and
// a third kernel adds them in ascending b.  No float atomics anywhere: the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/shw.h"
#include "wave_reduce.hpp"

namespace shw {

constexpr int kMsswH = 8, kMsswOut = 2, kMsswFlowH = 4, kMsswMaxFlows = 8;
constexpr int kMsswW1 = 0, kMsswB1 = kMsswW1 + 3 * kMsswH, kMsswW2 = kMsswB1 + kMsswH, kMsswB2 = kMsswW2 + kMsswH * kMsswH,
              kMsswW3 = kMsswB2 + kMsswH, kMsswB3 = kMsswW3 + kMsswH * kMsswOut, kMsswEnc = kMsswB3 + kMsswOut;
// one flow: gamma0, W0 (4, 2), c0 (4), gamma1, W1 (2, 4), c1 (2)
constexpr int kMsswG0 = 0, kMsswF0 = 1, kMsswC0 = kMsswF0 + 2 * kMsswFlowH, kMsswG1 = kMsswC0 + kMsswFlowH,
              kMsswF1 = kMsswG1 + 1, kMsswC1 = kMsswF1 + 2 * kMsswFlowH, kMsswFlow = kMsswC1 + 2;
static_assert(kMsswW2 == 32 && kMsswB2 == 96 && kMsswEnc == 122 && kMsswFlow == 24,
              "the encoder's three reduction groups start at 0, 32, 96; a flow fills one group of 32");
constexpr int kMsswForwardBlock = 256;
constexpr int kMsswMaxBlocks = 1024;          // backward: one wave on each of the 256 x 4 SIMDs
constexpr float kMsswPi = 3.14159265358979323846f;

inline bool mssw_shape_ok(int hidden, int layers, int flows) {
  return hidden == kMsswFlowH && layers == 2 && flows >= 1 && flows <= kMsswMaxFlows;
}
inline long mssw_backward_blocks(long points) {
  const long tiles = (points + 63) / 64;
  return tiles < kMsswMaxBlocks ? tiles : kMsswMaxBlocks;
}
inline size_t mssw_affine_bytes(long B, long N, int flows) { return (size_t)B * (size_t)N * flows * 4 * sizeof(float); }

// tanh(u) and 1 - tanh(u)^2, both from e = exp(-2 |u|) in [0, 1]: saturation gives exactly +-1 and exactly 0, and no
// inf / inf or inf * 0 can form (shw_sphere_map.hip).
struct MsswTanh { float t, d; };
__device__ __forceinline__ MsswTanh mssw_tanh_with_slope(float u) {
  const float e = expf(-2.0f * fabsf(u));
  const float q = 1.0f + e;                            // in [1, 2]
  float r = __builtin_amdgcn_rcpf(q);
  r = fmaf(fmaf(-q, r, 1.0f), r, r);                   // one Newton step
  MsswTanh o;
  o.t = copysignf((1.0f - e) * r, u);
  o.d = 4.0f * e * r * r;
  return o;
}

// sin(pi u) and cos(pi u) for |u| <= 1: u = k / 2 + r with |r| <= 1/4, polynomials on |pi r| <= pi / 4, then the quadrant
// (shw_sphere_map.hip)
__device__ __forceinline__ void mssw_sincos_pi(float u, float& s, float& c) {
  const float k = rintf(2.0f * u);
  const float a = kMsswPi * fmaf(-0.5f, k, u);
  const float z = a * a;
  const float sp = fmaf(fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f), z * a, a);
  const float cp = fmaf(fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f), z * z,
                        fmaf(-0.5f, z, 1.0f));
  const int q = (int)k;
  const float sq = (q & 1) ? cp : sp, cq = (q & 1) ? sp : cp;
  s = (q & 2) ? -sq : sq;
  c = ((q + 1) & 2) ? -cq : cq;
}

// WHY DOUBLE: a data-initialised scale is exp(s) = 1 / std of a handful of clouds and the shift is -mean exp(s), so
// z exp(s) + t cancels and every ABSOLUTE rounding error made before it -- in the encoder, in the block -- reaches the
// angles multiplied by 1 / std, here 10 to 100.  The float32 composed path carries the same factor, but the accuracy rule
// compares against one sample of ITS error per case (4 x, floor 1e-6), which single-point cases with float32 arithmetic
// missed at 2.1e-6 against 1.3e-6.  The network up to the last scale and shift is therefore evaluated in
// float64 from the float32 data, which is also what settles the side of every ReLU kink; the angle map, which amplifies
// nothing, and all of the backward's sums stay float32.  The kernels are bound by their launches, not by this arithmetic.

// x * sigmoid(gamma x) / 1.1 and the two factors its derivatives need, sigmoid and complement both from e = exp(-|t|)
// (shw_flow.hip): sigmoid(-large) is exactly 0, sigmoid(large) exactly 1, s * c underflows to 0
struct MsswSwish { double a, s, c; };
__device__ __forceinline__ MsswSwish mssw_swish(double x, double gamma) {
  const double t = gamma * x;
  const double e = exp(-fabs(t));
  const double r = 1.0 / (1.0 + e);
  const double small = e * r;
  MsswSwish o;
  o.s = t >= 0.0 ? r : small;
  o.c = t >= 0.0 ? small : r;
  o.a = x * o.s * (1.0 / 1.1);
  return o;
}

struct MsswPoint { float c[3]; };                      // one 12-byte load or store per lane

// the encoder: activations after their ReLU (0 where the pre-activation is not > 0: torch's slope at exactly 0 is 0)
struct MsswEnc { double h1[kMsswH], h2[kMsswH]; };
__device__ __forceinline__ void mssw_encoder(const float* __restrict__ P, const float (&x)[3], MsswEnc& a, double (&z)[2]) {
#pragma unroll
  for (int j = 0; j < kMsswH; ++j) {
    double pre = P[kMsswB1 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i) pre = fma((double)P[kMsswW1 + 3 * j + i], (double)x[i], pre);
    a.h1[j] = pre > 0.0 ? pre : 0.0;
  }
#pragma unroll
  for (int j = 0; j < kMsswH; ++j) {
    double pre = P[kMsswB2 + j];
#pragma unroll
    for (int i = 0; i < kMsswH; ++i) pre = fma((double)P[kMsswW2 + kMsswH * j + i], a.h1[i], pre);
    a.h2[j] = pre > 0.0 ? pre : 0.0;
  }
#pragma unroll
  for (int j = 0; j < kMsswOut; ++j) {
    double acc = P[kMsswB3 + j];
#pragma unroll
    for (int i = 0; i < kMsswH; ++i) acc = fma((double)P[kMsswW3 + kMsswH * j + i], a.h2[i], acc);
    z[j] = acc;
  }
}

// one flow's network on z: the Swish pairs of both layers and the hidden pre-activations are left for the backward
struct MsswFlowAct { MsswSwish w0[2], w1[kMsswFlowH]; double h[kMsswFlowH], o[2]; };
__device__ __forceinline__ void mssw_flow_net(const float* __restrict__ q, const double (&z)[2], MsswFlowAct& a) {
#pragma unroll
  for (int i = 0; i < 2; ++i) a.w0[i] = mssw_swish(z[i], (double)q[kMsswG0]);
#pragma unroll
  for (int j = 0; j < kMsswFlowH; ++j) {
    a.h[j] = fma((double)q[kMsswF0 + 2 * j + 1], a.w0[1].a, fma((double)q[kMsswF0 + 2 * j], a.w0[0].a, (double)q[kMsswC0 + j]));
    a.w1[j] = mssw_swish(a.h[j], (double)q[kMsswG1]);
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    double acc = q[kMsswC1 + j];
#pragma unroll
    for (int i = 0; i < kMsswFlowH; ++i) acc = fma((double)q[kMsswF1 + kMsswFlowH * j + i], a.w1[i].a, acc);
    a.o[j] = acc;
  }
}

// the residual block and the scale and shift of its point index
__device__ __forceinline__ void mssw_flow_forward(const float* __restrict__ q, const float4 sa, double (&z)[2]) {
  MsswFlowAct a;
  mssw_flow_net(q, z, a);
  z[0] = fma(z[0] + a.o[0], exp((double)sa.x), (double)sa.z);
  z[1] = fma(z[1] + a.o[1], exp((double)sa.y), (double)sa.w);
}

// the angle map; theta1 = pi / 2 + pi t0 / 2: sin theta1 = cos(pi t0 / 2), cos theta1 = -sin(pi t0 / 2); theta2 = pi t1
struct MsswAngles { float dt[2], s1, c1, s2, c2; };
__device__ __forceinline__ void mssw_angles(const double (&z)[2], MsswAngles& a) {
  const MsswTanh t0 = mssw_tanh_with_slope((float)z[0]), t1 = mssw_tanh_with_slope((float)z[1]);
  a.dt[0] = t0.d;
  a.dt[1] = t1.d;
  float sh, ch;
  mssw_sincos_pi(0.5f * t0.t, sh, ch);
  a.s1 = ch;
  a.c1 = -sh;
  mssw_sincos_pi(t1.t, a.s2, a.c2);
}

__global__ __launch_bounds__(kMsswForwardBlock) void mssw_forward_kernel(const float* __restrict__ x,
                                                                        const float* __restrict__ params,
                                                                        const float4* __restrict__ affine, long points,
                                                                        long N, int flows, float* __restrict__ y) {
  const long p = (long)blockIdx.x * kMsswForwardBlock + threadIdx.x;
  if (p >= points) return;
  const long n = p % N;
  const MsswPoint in = reinterpret_cast<const MsswPoint*>(x)[p];
  MsswEnc enc;
  double z[2];
  mssw_encoder(params, in.c, enc, z);
  for (int f = 0; f < flows; ++f) mssw_flow_forward(params + kMsswEnc + f * kMsswFlow, affine[f * N + n], z);
  MsswAngles a;
  mssw_angles(z, a);
  MsswPoint out;
  out.c[0] = a.s1 * a.c2;
  out.c[1] = a.s1 * a.s2;
  out.c[2] = a.c1;
  reinterpret_cast<MsswPoint*>(y)[p] = out;
}

// one group of per-lane contributions summed over the wave and stored (first tile of the block) or added (later tiles)
template <int G>
__device__ __forceinline__ void mssw_emit_group(float (&v)[G], int count, float* __restrict__ dst, int lane, bool first) {
  const float r = transpose_reduce<G>(v, lane);
  if (lane < count) {
    float* q = dst + lane;
    *q = first ? r : *q + r;
  }
}

// partial: one (122 + 24 flows)-float vector per block, or unused without WANT_P.  point_affine (B, flows, N) float4:
// every point's own (gs0, gs1, gt0, gt1) per flow, or null.
template <bool WANT_P>
__global__ __launch_bounds__(64) void mssw_backward_kernel(const float* __restrict__ x, const float* __restrict__ params,
                                                          const float4* __restrict__ affine,
                                                          const float* __restrict__ gy, long points, long N, int flows,
                                                          float* __restrict__ gx, float* __restrict__ partial,
                                                          float4* __restrict__ point_affine) {
  __shared__ double lds[2 * kMsswMaxFlows * 64];
  const int lane = threadIdx.x;
  double* const ent = lds + lane;                  // the flows' entry points [flows][2], one column per lane
  const float* __restrict__ P = params;
  float* mine = nullptr;                          // this block's partial vector
  if constexpr (WANT_P) mine = partial + (long)blockIdx.x * (kMsswEnc + kMsswFlow * flows);
  const long tiles = (points + 63) / 64;
  bool first = true;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x, first = false) {
    const long p = tile * 64 + lane;
    const bool live = p < points;                 // a lane past the end carries x = 0, gy = 0, s = t = 0: it adds zeros
    const long b = live ? p / N : 0, n = live ? p - b * N : 0;
    MsswPoint in = {{0.f, 0.f, 0.f}}, g = {{0.f, 0.f, 0.f}};
    if (live) {
      in = reinterpret_cast<const MsswPoint*>(x)[p];
      g = reinterpret_cast<const MsswPoint*>(gy)[p];
    }
    MsswEnc enc;
    double z[2];
    mssw_encoder(P, in.c, enc, z);
    for (int f = 0; f < flows; ++f) {
      ent[(2 * f) * 64] = z[0];
      ent[(2 * f + 1) * 64] = z[1];
      const float4 sa = live ? affine[f * N + n] : make_float4(0.f, 0.f, 0.f, 0.f);
      mssw_flow_forward(P + kMsswEnc + f * kMsswFlow, sa, z);
    }
    MsswAngles an;
    mssw_angles(z, an);
    const float dth1 = an.c1 * (g.c[0] * an.c2 + g.c[1] * an.s2) - g.c[2] * an.s1;
    const float dth2 = an.s1 * (g.c[1] * an.c2 - g.c[0] * an.s2);
    double gz[2] = {dth1 * (0.5f * kMsswPi) * an.dt[0], dth2 * kMsswPi * an.dt[1]};
    for (int f = flows - 1; f >= 0; --f) {
      const float* __restrict__ q = P + kMsswEnc + f * kMsswFlow;
      const double zin[2] = {ent[(2 * f) * 64], ent[(2 * f + 1) * 64]};
      const float4 sa = live ? affine[f * N + n] : make_float4(0.f, 0.f, 0.f, 0.f);
      MsswFlowAct a;
      mssw_flow_net(q, zin, a);
      const double e[2] = {exp((double)sa.x), exp((double)sa.y)};
      if (live && point_affine)                   // gs = g (z + o) exp(s), gt = g
        point_affine[(b * flows + f) * N + n] =
            make_float4((float)(gz[0] * ((zin[0] + a.o[0]) * e[0])), (float)(gz[1] * ((zin[1] + a.o[1]) * e[1])),
                        (float)gz[0], (float)gz[1]);
      const double go[2] = {gz[0] * e[0], gz[1] * e[1]};
      const double gamma0 = q[kMsswG0], gamma1 = q[kMsswG1];
      double dh[kMsswFlowH], dgamma1 = 0.0;       // gradients at the hidden pre-activations
#pragma unroll
      for (int i = 0; i < kMsswFlowH; ++i) {
        const double da = fma((double)q[kMsswF1 + kMsswFlowH + i], go[1], (double)q[kMsswF1 + i] * go[0]) * (1.0 / 1.1);
        const double sc = a.w1[i].s * a.w1[i].c;
        dgamma1 = fma(da, a.h[i] * (a.h[i] * sc), dgamma1);           // d a / d gamma = x^2 s (1 - s) / 1.1
        dh[i] = da * fma(gamma1 * a.h[i], sc, a.w1[i].s);             // d a / d x = (s + gamma x s (1 - s)) / 1.1
      }
      double dz[2], dgamma0 = 0.0;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        double da = 0.0;
#pragma unroll
        for (int j = 0; j < kMsswFlowH; ++j) da = fma((double)q[kMsswF0 + 2 * j + i], dh[j], da);
        da *= 1.0 / 1.1;
        const double sc = a.w0[i].s * a.w0[i].c;
        dgamma0 = fma(da, zin[i] * (zin[i] * sc), dgamma0);
        dz[i] = da * fma(gamma0 * zin[i], sc, a.w0[i].s);
      }
      if constexpr (WANT_P) {
        float v[32];
#pragma unroll
        for (int t = 0; t < 32; ++t) {
          if (t == kMsswG0) v[t] = (float)dgamma0;
          else if (t < kMsswC0) v[t] = (float)(dh[(t - kMsswF0) / 2] * a.w0[(t - kMsswF0) % 2].a);
          else if (t < kMsswG1) v[t] = (float)dh[t - kMsswC0];
          else if (t == kMsswG1) v[t] = (float)dgamma1;
          else if (t < kMsswC1) v[t] = (float)(go[(t - kMsswF1) / kMsswFlowH] * a.w1[(t - kMsswF1) % kMsswFlowH].a);
          else if (t < kMsswFlow) v[t] = (float)go[t - kMsswC1];
          else v[t] = 0.f;
        }
        mssw_emit_group<32>(v, kMsswFlow, mine + kMsswEnc + f * kMsswFlow, lane, first);
      }
      gz[0] = go[0] + dz[0];
      gz[1] = go[1] + dz[1];
    }
    const float ge[2] = {(float)gz[0], (float)gz[1]};   // the encoder's backward and its sums are float32
    float h1[kMsswH], h2[kMsswH];
#pragma unroll
    for (int i = 0; i < kMsswH; ++i) {
      h1[i] = (float)enc.h1[i];
      h2[i] = (float)enc.h2[i];
    }
    float g2[kMsswH];                             // gradients at the pre-activations of the second layer
#pragma unroll
    for (int i = 0; i < kMsswH; ++i) {
      const float acc = fmaf(P[kMsswW3 + kMsswH + i], ge[1], P[kMsswW3 + i] * ge[0]);
      g2[i] = enc.h2[i] > 0.0 ? acc : 0.f;
    }
    if constexpr (WANT_P) {
      float v[32];                                // b2, W3, b3, six zeros
#pragma unroll
      for (int t = 0; t < 32; ++t) {
        const int c = kMsswB2 + t;
        if (c < kMsswW3) v[t] = g2[c - kMsswB2];
        else if (c < kMsswB3) v[t] = ge[(c - kMsswW3) / kMsswH] * h2[(c - kMsswW3) % kMsswH];
        else if (c < kMsswEnc) v[t] = ge[c - kMsswB3];
        else v[t] = 0.f;
      }
      mssw_emit_group<32>(v, kMsswEnc - kMsswB2, mine + kMsswB2, lane, first);
      float w[64];                                // W2
#pragma unroll
      for (int t = 0; t < 64; ++t) w[t] = g2[t / kMsswH] * h1[t % kMsswH];
      mssw_emit_group<64>(w, 64, mine + kMsswW2, lane, first);
    }
    float g1[kMsswH];                             // ... of the first layer
#pragma unroll
    for (int i = 0; i < kMsswH; ++i) {
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < kMsswH; ++j) acc = fmaf(P[kMsswW2 + kMsswH * j + i], g2[j], acc);
      g1[i] = enc.h1[i] > 0.0 ? acc : 0.f;
    }
    if constexpr (WANT_P) {
      float v[32];                                // W1, b1
#pragma unroll
      for (int t = 0; t < 32; ++t) v[t] = t < kMsswB1 ? g1[t / 3] * in.c[t % 3] : g1[t - kMsswB1];
      mssw_emit_group<32>(v, 32, mine + kMsswW1, lane, first);
    }
    if (live && gx) {
      MsswPoint out;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < kMsswH; ++j) acc = fmaf(P[kMsswW1 + 3 * j + c], g1[j], acc);
        out.c[c] = acc;
      }
      reinterpret_cast<MsswPoint*>(gx)[p] = out;
    }
  }
}

// out[p] = sum over the partial vectors, in ascending order within each of 16 interleaved slices and then over the slices
__global__ __launch_bounds__(256) void mssw_param_reduce_kernel(const float* __restrict__ partial, int vectors, int count,
                                                               float* __restrict__ out) {
  __shared__ float sh[16][17];
  const int c = threadIdx.x & 15, s = threadIdx.x >> 4;
  const int p = blockIdx.x * 16 + c;
  float acc = 0.f;
  if (p < count)
    for (int b = s; b < vectors; b += 16) acc += partial[(long)b * count + p];
  sh[s][c] = acc;
  __syncthreads();
  if (s == 0 && p < count) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += sh[k][c];
    out[p] = t;
  }
}

// out[f, n] = sum over b, ascending, of point_affine[b, f, n]; `groups` = flows * N float4 per cloud
__global__ __launch_bounds__(256) void mssw_affine_reduce_kernel(const float4* __restrict__ point_affine, long B,
                                                                long groups, float4* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= groups) return;
  float4 acc = point_affine[i];
  for (long b = 1; b < B; ++b) {
    const float4 v = point_affine[b * groups + i];
    acc.x += v.x;
    acc.y += v.y;
    acc.z += v.z;
    acc.w += v.w;
  }
  out[i] = acc;
}

inline bool mssw_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace shw

extern "C" {

int shw_mssw_supported(int hidden, int layers, int flows) { return shw::mssw_shape_ok(hidden, layers, flows) ? 1 : 0; }

size_t shw_mssw_param_count(int flows) {
  return shw::mssw_shape_ok(shw::kMsswFlowH, 2, flows) ? (size_t)(shw::kMsswEnc + shw::kMsswFlow * flows) : 0;
}

int shw_mssw_backward_blocks(long points) { return points <= 0 ? 0 : (int)shw::mssw_backward_blocks(points); }

size_t shw_mssw_workspace_bytes(long B, long N, int flows) {
  if (B <= 0 || N <= 0 || !shw::mssw_shape_ok(shw::kMsswFlowH, 2, flows)) return 0;
  return shw::mssw_affine_bytes(B, N, flows) +
         (size_t)shw::mssw_backward_blocks(B * N) * (shw::kMsswEnc + shw::kMsswFlow * flows) * sizeof(float);
}

int shw_mssw_forward(const float* x, const float* params, const float* affine, long B, long N, int flows, float* y,
                     void* stream) {
  if (B < 0 || N < 0 || !shw::mssw_shape_ok(shw::kMsswFlowH, 2, flows)) return (int)hipErrorInvalidValue;
  if (B == 0 || N == 0) return 0;                             // no point: nothing is read or written
  if (!x || !params || !affine || !y || !shw::mssw_aligned16(affine) || N > 0x7fffffffffffL / B)
    return (int)hipErrorInvalidValue;
  const long points = B * N;
  const long blocks = (points + shw::kMsswForwardBlock - 1) / shw::kMsswForwardBlock;
  if (blocks > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(shw::mssw_forward_kernel, dim3((unsigned)blocks), dim3(shw::kMsswForwardBlock), 0,
                     (hipStream_t)stream, x, params, (const float4*)affine, points, N, flows, y);
  return (int)hipGetLastError();
}

int shw_mssw_backward(const float* x, const float* params, const float* affine, const float* gy, long B, long N, int flows,
                      float* gx, float* gparams, float* gaffine, void* workspace, void* stream) {
  if (B < 0 || N < 0 || N > 0x7fffffffL || !shw::mssw_shape_ok(shw::kMsswFlowH, 2, flows) ||
      !shw::mssw_aligned16(gaffine))
    return (int)hipErrorInvalidValue;
  const hipStream_t st = (hipStream_t)stream;
  const int count = shw::kMsswEnc + shw::kMsswFlow * flows;
  if (B == 0 || N == 0) {                                     // no point, no contribution: nothing else is read
    int rc = gparams ? (int)hipMemsetAsync(gparams, 0, count * sizeof(float), st) : 0;
    if (rc == 0 && gaffine && N > 0) rc = (int)hipMemsetAsync(gaffine, 0, (size_t)flows * N * 4 * sizeof(float), st);
    return rc;
  }
  if (!x || !params || !affine || !gy || !shw::mssw_aligned16(affine) || !shw::mssw_aligned16(workspace) ||
      N > 0x7fffffffffffL / B)
    return (int)hipErrorInvalidValue;
  const long points = B * N;
  if ((gparams || gaffine) && !workspace) return (int)hipErrorInvalidValue;
  if (!gx && !gparams && !gaffine) return 0;
  const long blocks = shw::mssw_backward_blocks(points);
  float4* const point_affine = gaffine ? (float4*)workspace : nullptr;
  float* const partial = (float*)((char*)workspace + shw::mssw_affine_bytes(B, N, flows));
  if (gparams)
    hipLaunchKernelGGL(shw::mssw_backward_kernel<true>, dim3((unsigned)blocks), dim3(64), 0, st, x, params,
                       (const float4*)affine, gy, points, N, flows, gx, partial, point_affine);
  else
    hipLaunchKernelGGL(shw::mssw_backward_kernel<false>, dim3((unsigned)blocks), dim3(64), 0, st, x, params,
                       (const float4*)affine, gy, points, N, flows, gx, (float*)nullptr, point_affine);
  int rc = (int)hipGetLastError();
  if (rc == 0 && gparams) {
    hipLaunchKernelGGL(shw::mssw_param_reduce_kernel, dim3((count + 15) / 16), dim3(256), 0, st, (const float*)partial,
                       (int)blocks, count, gparams);
    rc = (int)hipGetLastError();
  }
  if (rc == 0 && gaffine) {
    const long groups = (long)flows * N;
    hipLaunchKernelGGL(shw::mssw_affine_reduce_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st,
                       (const float4*)point_affine, B, groups, (float4*)gaffine);
    rc = (int)hipGetLastError();
  }
  return rc;
}

}  // extern "C"
