// launch_recorder.cpp -- which kernel, grid, block and dynamic LDS does every C entry point launch?  Answered on the
// CPU: the host halves of the csrc units (hipcc --cuda-host-only) are linked against the stub HIP runtime below, which
// records launches instead of performing them.  The host code never dereferences its pointer arguments
// (shw_ssw_backward_points looks at their alignment only), so the driver passes made-up addresses.  Uses only
// include/shw.h: the same source builds against any tree that keeps the C ABI.  Built and compared with
// tests/golden/dispatch_launches.txt.gz by tests/test_dispatch_cpu.py (which documents the case sets).
//
//   launch_recorder <set>      set: all | fwd | grad | fwdgrad | kpl | p1 | bwd | euclid     (knobs come from the environment)
// stdout: one line per call -- the case, then `K<i> g=<grid x>,<grid y> b=<block x> lds=<bytes>` per launch and the
//         return code (a grid z other than 1 follows grid y); `K<i> = <mangled name>` is printed when a kernel is first
//         launched.
// stderr: `unlaunched <mangled name>` for every registered kernel that no case of this run launched.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "shw.h"

// ------------------------------------------------------------------------------------------------ stub HIP runtime
struct Dim3 { unsigned x, y, z; };
static std::map<const void*, std::string>& kernel_names() { static std::map<const void*, std::string> m; return m; }
static std::map<const void*, int> g_ids;
static std::string g_line;
static struct { Dim3 grid, block; size_t lds; void* stream; } g_cfg;

extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host, char*, const char* name, unsigned, void*, void*, void*, void*, int*) {
  kernel_names()[host] = name;
}
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}
unsigned __hipPushCallConfiguration(Dim3 grid, Dim3 block, size_t lds, void* stream) {
  g_cfg = {grid, block, lds, stream};
  return 0;
}
unsigned __hipPopCallConfiguration(Dim3* grid, Dim3* block, size_t* lds, void** stream) {
  *grid = g_cfg.grid; *block = g_cfg.block; *lds = g_cfg.lds; *stream = g_cfg.stream;
  return 0;
}
int hipLaunchKernel(const void* f, Dim3 grid, Dim3 block, void**, size_t lds, void*) {
  auto it = g_ids.find(f);
  if (it == g_ids.end()) {
    it = g_ids.emplace(f, (int)g_ids.size()).first;
    printf("K%d = %s\n", it->second, kernel_names().count(f) ? kernel_names()[f].c_str() : "?");
  }
  char buf[96], z[16] = "";
  if (grid.z != 1) snprintf(z, sizeof z, ",%u", grid.z);
  snprintf(buf, sizeof buf, " K%d g=%u,%u%s b=%u lds=%zu |", it->second, grid.x, grid.y, z, block.x, lds);
  g_line += buf;
  return 0;
}
int hipGetLastError(void) { return 0; }
int hipGetDevice(int* dev) { *dev = 0; return 0; }
int hipFuncSetAttribute(const void*, int, int) { return 0; }
}

// ------------------------------------------------------------------------------------------------ driver
template <class T> static T* fake(int slot, int byte_offset = 0) {       // distinct, 16-byte aligned, never dereferenced
  return reinterpret_cast<T*>((uintptr_t)0x10000000u * (unsigned)(slot + 1) + (unsigned)byte_offset);
}
static void report(int rc, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
static void report(int rc, const char* fmt, ...) {
  char head[160];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(head, sizeof head, fmt, ap);
  va_end(ap);
  printf("%s ->%s rc=%d\n", head, g_line.c_str(), rc);
  g_line.clear();
}

static const int kSizes[] = {1, 64, 65, 128, 200, 256, 257, 511, 512, 513, 700, 768, 769, 1024, 1025, 1200, 1280, 1281, 1536, 1537,
                             1700, 1792, 1793, 2000, 2047, 2048, 2049, 2560, 2561, 3000, 3072, 3073, 4096, 4097, 5000,
                             5120, 5121, 6144, 6145, 8192, 8193};
static const int kUnequal[][2] = {{1200, 900}, {2048, 1536}, {8, 5}, {4096, 4095}, {600, 500}, {500, 600}, {3000, 100},
                                  {100, 8192}, {2049, 2048}, {1400, 1400 + 9}};      // p == 1 takes any n and m
static const int kProblems[][2] = {{1, 100}, {2, 512}, {5, 205}, {8, 512}};

static void sliced(bool grad, int n, int m, int pairs, int slices, float p) {
  const int rc = grad ? shw_ssw_forward_grad(fake<float>(0), fake<float>(1), fake<float>(2), pairs, n, m, slices, 0, p,
                                             fake<float>(3), fake<int32_t>(4), fake<float>(5), fake<float>(6), nullptr)
                      : shw_ssw_forward(fake<float>(0), fake<float>(1), fake<float>(2), pairs, n, m, slices, 0, p,
                                        fake<float>(3), fake<int32_t>(4), nullptr);
  report(rc, "%s n=%d m=%d B=%dx%d p=%g", grad ? "forward_grad" : "forward", n, m, pairs, slices, p);
}

// the sliced entry points over every size; `problems`: 4 = every problem count, 2 = the smallest and the largest, 1 = the smallest
static void sliced_sweep(bool fwd, bool grad, const std::vector<float>& powers, int problems) {
  for (int g = 0; g < 2; ++g) {
    if (!(g ? grad : fwd)) continue;
    for (float p : powers) {
      for (const auto& pr : kProblems) {
        if ((problems < 4 && pr[0] != 1 && pr[0] != 8) || (problems < 2 && pr[0] != 1)) continue;
        for (int n : kSizes) sliced(g, n, n, pr[0], pr[1], p);
        if (p == 1.f)
          for (const auto& nm : kUnequal) sliced(g, nm[0], nm[1], pr[0], pr[1], p);
      }
    }
  }
}

static void general() {
  const int shapes[][2] = {{1200, 900}, {2048, 1536}, {8, 5}, {4096, 4095}, {4097, 10}, {64, 64}, {128, 100}, {200, 130}, {500, 400}, {900, 1024}};
  for (const auto& s : shapes)
    for (int w = 0; w < 3; ++w)                       // no weights, wu only, both
      for (int grad = 0; grad < 2; ++grad)
        for (float p : {1.f, 2.f, 3.f}) {
          const int rc = shw_ssw_forward_general(fake<float>(0), fake<float>(1), fake<float>(2), w ? fake<float>(7) : nullptr,
                                                 w == 2 ? fake<float>(8) : nullptr, 0, 0, 3, s[0], s[1], 100, 0, p, fake<float>(3),
                                                 fake<float>(4), grad ? fake<float>(5) : nullptr, grad ? fake<float>(6) : nullptr, nullptr);
          report(rc, "forward_general n=%d m=%d weights=%d grad=%d p=%g", s[0], s[1], w, grad, p);
        }
}

static void circle(bool every_row_count) {
  const int shapes[][3] = {{1200, 1200, 0}, {1200, 900, 0}, {1200, 1200, 1}, {2048, 2048, 0}, {3000, 3000, 0}, {5000, 5000, 0},
                           {5000, 4000, 0}, {5000, 5000, 1}, {8192, 8192, 0}, {300, 300, 0}};      // n, m, weights
  for (const auto& s : shapes)
    for (int method : {SHW_CIRCLE_AS_SLICED, SHW_CIRCLE_BISECTION, SHW_CIRCLE_LEVEL_MEDIAN})
      for (float p : {1.f, 2.f})
        for (int grad = 0; grad < 2; ++grad)
          for (int rows : {7, 2000}) {
            if (rows != 7 && !every_row_count) continue;      // (emd1D_circle at p = 2: refused, rc = 1)
            const int rc = shw_circle_ot(fake<float>(0), fake<float>(1), s[2] ? fake<float>(7) : nullptr,
                                         s[2] ? fake<float>(8) : nullptr, 0, 0, rows, s[0], s[1], p, method, fake<float>(3),
                                         fake<float>(4), grad ? fake<float>(5) : nullptr, grad ? fake<float>(6) : nullptr, nullptr);
            report(rc, "circle_ot n=%d m=%d weights=%d method=%d p=%g grad=%d rows=%d", s[0], s[1], s[2], method, p, grad, rows);
          }
}

static void backward() {
  const int shapes[][2] = {{1200, 1200}, {1201, 1201}, {1200, 900}, {1200, 1201}, {64, 64}, {2, 2}, {2048, 2048}};
  for (const auto& s : shapes)
    for (int pairs : {1, 64, 70000})
      for (int slices : {16, 32})
        for (int off : {0, 4}) {
          const int rc = shw_ssw_backward_points(fake<float>(0), fake<float>(1), fake<float>(2), fake<float>(5), fake<float>(6, off),
                                                 pairs, s[0], s[1], slices, 0, 1.f, nullptr, nullptr, fake<float>(9),
                                                 fake<float>(10), nullptr);
          report(rc, "backward_points n=%d m=%d pairs=%d slices=%d offset=%d", s[0], s[1], pairs, slices, off);
        }
}

static void rest() {
  for (int pairs : {1, 256, 257})
    for (int total = 0; total < 2; ++total)
      report(shw_ssw_reduce(fake<float>(3), pairs, 100, 0.01f, fake<float>(11), total ? fake<float>(12) : nullptr, nullptr),
             "reduce pairs=%d total=%d", pairs, total);
  for (long count : {1L, 256L, 257L, 32768L})
    report(shw_stiefel_frames(fake<float>(0), count, fake<float>(1), nullptr), "stiefel_frames count=%ld", count);
  // float64
  for (int n : {64, 2048, 4096, 4097})
    for (double p : {1.0, 2.0, 1.5})
      for (int grad = 0; grad < 2; ++grad) {
        report(shw_ssw_forward_f64(fake<double>(0), fake<double>(1), fake<double>(2), 3, n, n, 100, 0, p, fake<double>(3),
                                   fake<int32_t>(4), grad ? fake<double>(5) : nullptr, grad ? fake<double>(6) : nullptr, nullptr),
               "forward_f64 n=%d p=%g grad=%d", n, p, grad);
        for (int method : {SHW_CIRCLE_AS_SLICED, SHW_CIRCLE_BISECTION, SHW_CIRCLE_LEVEL_MEDIAN})
          report(shw_circle_ot_f64(fake<double>(0), fake<double>(1), 7, n, n, p, method, fake<double>(3), fake<int32_t>(4),
                                   grad ? fake<double>(5) : nullptr, grad ? fake<double>(6) : nullptr, nullptr),
                 "circle_ot_f64 n=%d p=%g method=%d grad=%d", n, p, method, grad);
      }
  for (int pairs : {1, 70000})
    report(shw_ssw_backward_points_f64(fake<double>(0), fake<double>(1), fake<double>(2), fake<double>(5), fake<double>(6), pairs,
                                       1200, 1200, 32, 0, 1.0, nullptr, nullptr, fake<double>(9), fake<double>(10), nullptr),
           "backward_points_f64 pairs=%d", pairs);
  for (int total = 0; total < 2; ++total)
    report(shw_ssw_reduce_f64(fake<double>(3), 300, 100, 0.01, fake<double>(11), total ? fake<double>(12) : nullptr, nullptr),
           "reduce_f64 total=%d", total);
  report(shw_stiefel_frames_f64(fake<double>(0), 257, fake<double>(1), nullptr), "stiefel_frames_f64 count=257");
}

// The Euclidean sliced family (shw_esw, shw_esw_dim, shw_gsw, shw_line_ot): every entry point over the values at which a
// step of its launch ladders changes.
static void euclid() {
  float *const xs = fake<float>(0), *const xt = fake<float>(1), *const th = fake<float>(2), *const sum = fake<float>(3);
  float *const cs = fake<float>(5), *const ct = fake<float>(6), *const wu = fake<float>(7), *const wv = fake<float>(8);
  float *const gs = fake<float>(9), *const gt = fake<float>(10), *const sw = fake<float>(11);
  float *const pu = fake<float>(12), *const pv = fake<float>(13);
  const int sizes[] = {1, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097};
  const int unequal[][2] = {{1200, 900}, {900, 1200}, {4096, 1}, {1, 4096}, {65, 64}, {2049, 300}, {300, 4097}};
  const int dims[] = {1, 3, 4, 5, 8, 9, 16, 17, 64, 65};
  const float powers[] = {2.f, 1.f, 1.5f};

  // size classes x power x gradient: the forward kernels (3 pairs x 100 slices, dim 6 where there is one)
  for (int n : sizes)
    for (float p : powers)
      for (int grad = 0; grad < 2; ++grad) {
        float *const a = grad ? cs : nullptr, *const b = grad ? ct : nullptr;
        report(shw_esw_forward(xs, xt, th, 3, n, 100, 0, p, sum, a, b, nullptr), "esw_forward n=%d p=%g grad=%d", n, p, grad);
        report(shw_esw_forward_dim(xs, xt, th, 3, n, 6, 100, 0, p, sum, a, b, nullptr), "esw_forward_dim n=%d p=%g grad=%d", n, p, grad);
        report(shw_gsw_rows_forward(xs, xt, 300, n, p, sum, a, b, nullptr), "gsw_rows_forward n=%d p=%g grad=%d", n, p, grad);
        report(shw_gsw_circular_forward(xs, xt, th, 3, n, 6, 100, 0, 1.5f, p, sum, a, b, nullptr),
               "gsw_circular_forward n=%d p=%g grad=%d", n, p, grad);
      }
  // line transport: equal and unequal sizes x power x gradient x weights (none, u only, both) x potentials
  for (int k = 0; k < (int)(sizeof sizes / sizeof sizes[0] + sizeof unequal / sizeof unequal[0]); ++k) {
    const int ns = sizeof sizes / sizeof sizes[0];
    const int n = k < ns ? sizes[k] : unequal[k - ns][0], m = k < ns ? sizes[k] : unequal[k - ns][1];
    for (float p : powers)
      for (int grad = 0; grad < 2; ++grad)
        for (int w = 0; w < 3; ++w)
          for (int pot = 0; pot < 2; ++pot) {
            float *const a = grad ? cs : nullptr, *const b = grad ? ct : nullptr;
            const float *const u_w = w ? wu : nullptr, *const v_w = w == 2 ? wv : nullptr;
            const long us = w ? n : 0, vs = w == 2 ? m : 0;
            if (!pot) {
              report(shw_line_rows_forward(xs, xt, 300, n, m, p, u_w, v_w, us, vs, sum, a, b, nullptr),
                     "line_rows_forward n=%d m=%d p=%g grad=%d weights=%d", n, m, p, grad, w);
              report(shw_line_esw_forward(xs, xt, th, 3, n, m, 6, 100, 0, p, u_w, v_w, us, vs, sum, a, b, nullptr),
                     "line_esw_forward n=%d m=%d p=%g grad=%d weights=%d", n, m, p, grad, w);
            } else {                                            // (a potential row without its weights: refused)
              report(shw_line_rows_forward_pot(xs, xt, 300, n, m, p, u_w, v_w, us, vs, sum, a, b, pu, w == 1 ? nullptr : pv, nullptr),
                     "line_rows_forward_pot n=%d m=%d p=%g grad=%d weights=%d", n, m, p, grad, w);
              report(shw_line_esw_forward_pot(xs, xt, th, 3, n, m, 6, 100, 0, p, u_w, v_w, us, vs, sum, a, b, pu,
                                              w == 1 ? nullptr : pv, nullptr),
                     "line_esw_forward_pot n=%d m=%d p=%g grad=%d weights=%d", n, m, p, grad, w);
            }
          }
  }
  // the gradient kernels over the point counts (workgroups of 256 points)
  for (int n : sizes) {
    report(shw_esw_backward_points(th, cs, ct, sw, 2, n, 100, 0, gs, gt, nullptr), "esw_backward_points n=%d", n);
    report(shw_esw_backward_dirs(xs, xt, cs, ct, sw, 2, n, 100, gs, nullptr), "esw_backward_dirs n=%d", n);
    report(shw_esw_backward_points_dim(th, cs, ct, sw, 2, n, 6, 100, 0, gs, gt, nullptr), "esw_backward_points_dim n=%d", n);
    report(shw_esw_backward_dirs_dim(xs, xt, cs, ct, sw, 2, n, 6, 100, gs, nullptr), "esw_backward_dirs_dim n=%d", n);
    report(shw_gsw_circular_backward_points(xs, xt, th, cs, ct, sw, 2, n, 6, 100, 0, 1.5f, gs, gt, nullptr),
           "gsw_circular_backward_points n=%d", n);
    report(shw_gsw_circular_backward_dirs(xs, xt, th, cs, ct, sw, 2, n, 6, 100, 0, 1.5f, gs, nullptr),
           "gsw_circular_backward_dirs n=%d", n);
  }
  for (const auto& nm : unequal) {
    report(shw_line_esw_backward_points(th, cs, ct, sw, 2, nm[0], nm[1], 6, 100, 0, gs, gt, nullptr),
           "line_esw_backward_points n=%d m=%d", nm[0], nm[1]);
    report(shw_line_esw_backward_dirs(xs, xt, cs, ct, sw, 2, nm[0], nm[1], 6, 100, gs, nullptr),
           "line_esw_backward_dirs n=%d m=%d", nm[0], nm[1]);
  }
  // point dimension (coordinate chunks of the gradient kernels) x stride of the directions: shared, per pair, too short
  for (int dim : dims)
    for (int st = 0; st < 3; ++st) {
      const long stride = st == 0 ? 0 : 100L * dim - (st == 2);
      for (int grad = 0; grad < 2; ++grad) {
        float *const a = grad ? cs : nullptr, *const b = grad ? ct : nullptr;
        report(shw_esw_forward_dim(xs, xt, th, 2, 1200, dim, 100, stride, 2.f, sum, a, b, nullptr),
               "esw_forward_dim dim=%d stride=%ld grad=%d", dim, stride, grad);
        report(shw_gsw_circular_forward(xs, xt, th, 2, 1200, dim, 100, stride, 1.5f, 2.f, sum, a, b, nullptr),
               "gsw_circular_forward dim=%d stride=%ld grad=%d", dim, stride, grad);
        report(shw_line_esw_forward(xs, xt, th, 2, 1200, 900, dim, 100, stride, 2.f, nullptr, nullptr, 0, 0, sum, a, b, nullptr),
               "line_esw_forward dim=%d stride=%ld grad=%d", dim, stride, grad);
      }
      report(shw_esw_backward_points_dim(th, cs, ct, sw, 2, 1200, dim, 100, stride, gs, gt, nullptr),
             "esw_backward_points_dim dim=%d stride=%ld", dim, stride);
      report(shw_gsw_circular_backward_points(xs, xt, th, cs, ct, sw, 2, 1200, dim, 100, stride, 1.5f, gs, gt, nullptr),
             "gsw_circular_backward_points dim=%d stride=%ld", dim, stride);
      report(shw_gsw_circular_backward_dirs(xs, xt, th, cs, ct, sw, 2, 1200, dim, 100, stride, 1.5f, gs, nullptr),
             "gsw_circular_backward_dirs dim=%d stride=%ld", dim, stride);
      report(shw_line_esw_backward_points(th, cs, ct, sw, 2, 1200, 900, dim, 100, stride, gs, gt, nullptr),
             "line_esw_backward_points dim=%d stride=%ld", dim, stride);
      if (st == 0) {
        report(shw_esw_backward_dirs_dim(xs, xt, cs, ct, sw, 2, 1200, dim, 100, gs, nullptr), "esw_backward_dirs_dim dim=%d", dim);
        report(shw_line_esw_backward_dirs(xs, xt, cs, ct, sw, 2, 1200, 900, dim, 100, gs, nullptr), "line_esw_backward_dirs dim=%d", dim);
      }
    }
  // problem counts: a grid's y holds 65535 pairs; a forward grid 2^31 - 1 workgroups
  const int counts[][2] = {{0, 100}, {1, 0}, {1, 1}, {65535, 1}, {65536, 1}, {65536, 32768}, {-1, 1}};      // pairs, slices
  for (const auto& c : counts) {
    const int B = c[0], L = c[1];
    report(shw_esw_forward(xs, xt, th, B, 200, L, 0, 2.f, sum, cs, ct, nullptr), "esw_forward pairs=%d slices=%d", B, L);
    report(shw_esw_forward_dim(xs, xt, th, B, 200, 6, L, 0, 2.f, sum, cs, ct, nullptr), "esw_forward_dim pairs=%d slices=%d", B, L);
    report(shw_gsw_rows_forward(xs, xt, (long)B * L, 200, 2.f, sum, cs, ct, nullptr), "gsw_rows_forward rows=%ld", (long)B * L);
    report(shw_gsw_circular_forward(xs, xt, th, B, 200, 6, L, 0, 1.5f, 2.f, sum, cs, ct, nullptr),
           "gsw_circular_forward pairs=%d slices=%d", B, L);
    report(shw_line_rows_forward(xs, xt, (long)B * L, 200, 150, 2.f, nullptr, nullptr, 0, 0, sum, cs, ct, nullptr),
           "line_rows_forward rows=%ld", (long)B * L);
    report(shw_line_esw_forward(xs, xt, th, B, 200, 150, 6, L, 0, 2.f, nullptr, nullptr, 0, 0, sum, cs, ct, nullptr),
           "line_esw_forward pairs=%d slices=%d", B, L);
    report(shw_line_esw_forward_pot(xs, xt, th, B, 200, 150, 6, L, 0, 2.f, wu, wv, 200, 150, sum, cs, ct, pu, pv, nullptr),
           "line_esw_forward_pot pairs=%d slices=%d", B, L);
    report(shw_esw_backward_points(th, cs, ct, sw, B, 200, L, 0, gs, gt, nullptr), "esw_backward_points pairs=%d slices=%d", B, L);
    report(shw_esw_backward_dirs(xs, xt, cs, ct, sw, B, 200, L, gs, nullptr), "esw_backward_dirs pairs=%d slices=%d", B, L);
    report(shw_esw_backward_points_dim(th, cs, ct, sw, B, 200, 6, L, 0, gs, gt, nullptr),
           "esw_backward_points_dim pairs=%d slices=%d", B, L);
    report(shw_esw_backward_dirs_dim(xs, xt, cs, ct, sw, B, 200, 6, L, gs, nullptr), "esw_backward_dirs_dim pairs=%d slices=%d", B, L);
    report(shw_gsw_circular_backward_points(xs, xt, th, cs, ct, sw, B, 200, 6, L, 0, 1.5f, gs, gt, nullptr),
           "gsw_circular_backward_points pairs=%d slices=%d", B, L);
    report(shw_gsw_circular_backward_dirs(xs, xt, th, cs, ct, sw, B, 200, 6, L, 0, 1.5f, gs, nullptr),
           "gsw_circular_backward_dirs pairs=%d slices=%d", B, L);
    report(shw_line_esw_backward_points(th, cs, ct, sw, B, 200, 150, 6, L, 0, gs, gt, nullptr),
           "line_esw_backward_points pairs=%d slices=%d", B, L);
    report(shw_line_esw_backward_dirs(xs, xt, cs, ct, sw, B, 200, 150, 6, L, gs, nullptr),
           "line_esw_backward_dirs pairs=%d slices=%d", B, L);
  }
  // refused: a power below 1, one coefficient row without the other, weights with a stride shorter than the row
  report(shw_esw_forward(xs, xt, th, 3, 200, 100, 0, 0.5f, sum, nullptr, nullptr, nullptr), "esw_forward p=0.5");
  report(shw_esw_forward_dim(xs, xt, th, 3, 200, 6, 100, 0, 2.f, sum, cs, nullptr, nullptr), "esw_forward_dim coef_s only");
  report(shw_gsw_rows_forward(xs, xt, 300, 200, 0.5f, sum, nullptr, nullptr, nullptr), "gsw_rows_forward p=0.5");
  report(shw_gsw_circular_forward(xs, xt, th, 3, 200, 6, 100, 0, 1.5f, 2.f, sum, nullptr, ct, nullptr), "gsw_circular_forward coef_t only");
  report(shw_line_rows_forward(xs, xt, 300, 200, 150, 2.f, wu, nullptr, 199, 0, sum, nullptr, nullptr, nullptr), "line_rows_forward weight stride 199");
  report(shw_line_esw_forward(xs, xt, th, 3, 200, 150, 6, 100, 0, 0.5f, nullptr, nullptr, 0, 0, sum, nullptr, nullptr, nullptr), "line_esw_forward p=0.5");
  // the reduction of the potentials over the slices: per pair, or shared (groups of 64 rows, then the groups)
  const int reduce[][2] = {{0, 100}, {1, 1}, {1, 64}, {1, 65}, {2, 100}, {65535, 1}, {65536, 1}, {65535, 64}, {65535, 65}};
  for (const auto& c : reduce)
    for (int count : {1, 256, 257, 4096, 4097})
      for (int shared = 0; shared < 2; ++shared)
        for (int ws = 0; ws < 2; ++ws) {
          if (ws && !shared) continue;
          const size_t bytes = shw_line_weight_grads_workspace_bytes(c[0], c[1], count, shared);
          report(shw_line_weight_grads(pu, sw, c[0], c[1], count, shared, ws ? fake<void>(14) : nullptr, gs, nullptr),
                 "line_weight_grads pairs=%d slices=%d count=%d shared=%d workspace=%d of %zu", c[0], c[1], count, shared, ws, bytes);
        }
}

int main(int argc, char** argv) {
  const std::string set = argc > 1 ? argv[1] : "all";
  if (set == "all") {
    sliced_sweep(true, true, {1.f, 2.f, 3.f, 1.5f}, 4);
    general(); circle(true); backward(); rest();
  } else if (set == "fwd") {            // knobs of the loss-only family rule
    sliced_sweep(true, false, {2.f}, 2); sliced_sweep(true, false, {1.5f}, 1); circle(false);
  } else if (set == "grad") {           // ... of the training family rule
    sliced_sweep(false, true, {2.f}, 2); sliced_sweep(false, true, {1.5f}, 1); circle(false);
  } else if (set == "fwdgrad") {        // the small-grid threshold: every problem count
    sliced_sweep(true, true, {2.f}, 4); circle(false);
  } else if (set == "kpl") {            // the keys-per-lane classes: p != 1 and p == 1
    sliced_sweep(true, true, {1.f, 2.f}, 2); circle(false);
  } else if (set == "p1") {             // knobs of the p == 1 rule (it does not look at the problem count)
    sliced_sweep(true, true, {1.f}, 1); circle(false);
  } else if (set == "bwd") {
    backward();
  } else if (set == "euclid") {         // the Euclidean sliced family: no knob reaches it
    euclid();
  } else {
    fprintf(stderr, "unknown case set %s\n", set.c_str());
    return 2;
  }
  for (const auto& kv : kernel_names()) {
    const std::string& name = kv.second;
    const bool other_unit = name.find("sinkhorn") != std::string::npos || name.find("chamfer") != std::string::npos;
    if (!other_unit && !g_ids.count(kv.first)) fprintf(stderr, "unlaunched %s\n", name.c_str());
  }
  return 0;
}
