/* shw.h -- C ABI of the MI355X (gfx950) spherical sliced-Wasserstein / Chamfer hot path.
 *
 * The reference has no FFI layer: its "operator API" for this path is a set of dependency-injected
 * Python callables.  The entry points below are what those callables bind to;
 * each one names the reference code it replaces (paths relative to
 * /root/reference/Point_Cloud_Resistration/losses/).  INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless stated otherwise;
 *   - the caller owns and allocates every buffer, including workspaces (sizes from the *_bytes
 *     helpers); nothing is allocated, freed or synchronised inside;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the default stream);
 *   - return value is a hipError_t cast to int: 0 = success, 1 (hipErrorInvalidValue) = bad
 *     arguments / unsupported size, anything else = the launch error.
 *   - clouds are fp32 row-major (pairs, points, 3); directions are fp32 (slices, 3, 2) orthonormal
 *     2-frames, either one set per pair (u_pair_stride = slices*6) or shared (u_pair_stride = 0).
 *   - the entries whose names end in _f64 take the same arrays as `double` (equal cloud sizes, uniform weights, at
 *     most SHW_MAX_POINTS_F64 points per cloud; the *_general_f64 entries: any two sizes and weights, at most
 *     SHW_MAX_POINTS_F64_GENERAL points per cloud); every other entry is fp32.
 */
#ifndef SHW_H
#define SHW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the library is built with -fvisibility=hidden: these entry points are its only dynamic symbols */
#define SHW_API __attribute__((visibility("default")))

#define SHW_ABI_VERSION 3 /* 2: shw_ssw_backward_points takes per-pair upstream weights; 3: shw_circle_ot takes `method`,
                             shw_sinkhorn_forward_train takes plan / cost_matrix */
#define SHW_MAX_POINTS 8192 /* per cloud, per pair */
#define SHW_MAX_POINTS_F64 4096 /* per cloud, per pair, on the float64 entry points (shw_*_f64) */
#define SHW_MAX_POINTS_F64_GENERAL 2048 /* per cloud, per pair, on the general float64 entry points (shw_*_general_f64) */

/* ABI version of the loaded library (== SHW_ABI_VERSION of the header it was built from). */
SHW_API int shw_abi_version(void);

/* Largest point count per cloud the sort kernels accept (SHW_MAX_POINTS). */
SHW_API int shw_max_points(void);

/* ---------------------------------------------------------------------------------------------
 * Direction frames.
 * Replaces: `U, _ = torch.linalg.qr(Z)` (max_spherical_sliced_w.py:308, _fast.py:318) for Z of shape (count, 3, 2):
 * reduced QR by Householder reflectors with LAPACK's sign convention, one thread per matrix.  The Gaussian
 * draw itself (`torch.randn`, :307) stays with the caller so the generator is consumed as in the reference.
 *   z (count, 3, 2) fp32 in, u (count, 3, 2) fp32 out (orthonormal columns).
 */
SHW_API int shw_stiefel_frames(const float* z, long count, float* u, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Spherical sliced-Wasserstein, forward.
 * Replaces: sliced_cost (max_spherical_sliced_w.py:251-286; batched _fast.py:258-295) =
 *   projection (:270-271) + normalise (:274-275) + circle coordinate (:278-279) + per-slice sort
 *   (:163-164 / :224-225) + circular OT solve (binary_search_circle :117-207 for p != 1,
 *   emd1D_circle :210-247 for p == 1) -- everything up to, not including, the mean over slices.
 *
 *   xs (pairs, n, 3), xt (pairs, m, 3), dirs (see header comment), p >= 1.
 *   slice_cost  (pairs*slices) fp32 out : circular OT cost W_p^p of every (pair, slice).
 *   slice_shift (pairs*slices) int32 out, may be NULL : optimal cyclic shift k* of the sorted
 *                target against the sorted source (p != 1), or the median level (p == 1).
 * This entry point: uniform weights; n == m for p != 1; any n, m for p == 1; 1 <= n, m <= SHW_MAX_POINTS.
 * (n != m or weights with p != 1: shw_ssw_forward_general.)
 */
SHW_API int shw_ssw_forward(const float* xs, const float* xt, const float* dirs,
                    int pairs, int n, int m, int slices, long u_pair_stride, float p,
                    float* slice_cost, int32_t* slice_shift, void* stream);

/* Reduction of per-slice costs to the reference's scalars.
 * Replaces: torch.mean(w1) (:286) per pair and the `w1 += mean(...)` loop over the batch
 * (_fast.py:291-293).
 *   pair_loss (pairs) out : scale * sum_l slice_cost[b, l]   (scale = 1/slices on one GPU, or
 *                           1/global_slices when slices are sharded across ranks)
 *   total     (2)     out : total[0] = sum_b pair_loss[b], total[1] = total[0] / pairs
 * Deterministic (fixed-order shuffle + serial tree, no atomics).
 */
SHW_API int shw_ssw_reduce(const float* slice_cost, int pairs, int slices, float scale,
                   float* pair_loss, float* total, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Spherical sliced-Wasserstein, forward + gradient in one pass.
 * Replaces: autograd through Cost -> gather -> sort -> atan2 -> normalize -> matmul
 * (max_spherical_sliced_w.py:207, :100-112, :163-164, :270-279); used by the notebooks' gradient
 * flow (Flow_cube.ipynb:1381-1383) and by any trainer that back-propagates through the loss.
 *
 * Computes slice_cost / slice_shift as shw_ssw_forward and, additionally,
 *   coef_s (pairs*slices*n) fp32 scratch : d cost(b,l) / d coord_s[b,l,i]  in ORIGINAL point order
 *   coef_t (pairs*slices*m) fp32 scratch : d cost(b,l) / d coord_t[b,l,j]
 * which shw_ssw_backward_points turns into d(sum_b pair_loss[b]) / d xs, / d xt:
 *   grad_xs[b,i,:] = scale * sum_l coef_s[b,l,i] * (-b_ U[:,0] + a_ U[:,1]) / (2 pi (a_^2 + b_^2)),
 *   (a_, b_) = U_l^T xs[b,i]   (SURVEY.md 8a row A9), likewise for xt.
 * Deterministic: every gradient element is summed over slices in a fixed order by one thread.
 */
SHW_API size_t shw_ssw_coef_bytes(int pairs, int n, int m, int slices);

SHW_API int shw_ssw_forward_grad(const float* xs, const float* xt, const float* dirs,
                         int pairs, int n, int m, int slices, long u_pair_stride, float p,
                         float* slice_cost, int32_t* slice_shift,
                         float* coef_s, float* coef_t, void* stream);

/* pair_w (pairs) and total_w (1) fp32, each may be NULL: upstream gradients d loss / d pair_loss[b] and
 * d loss / d total[0] of shw_ssw_reduce's outputs; row b of both gradients is multiplied by
 * pair_w[b] + total_w[0] inside the kernel (a NULL term counts as 0; both NULL = 1).  Any number of pairs
 * (batches beyond 65535 pairs go out as several launches). */
SHW_API int shw_ssw_backward_points(const float* xs, const float* xt, const float* dirs,
                            const float* coef_s, const float* coef_t,
                            int pairs, int n, int m, int slices, long u_pair_stride, float scale,
                            const float* pair_w, const float* total_w, float* grad_xs, float* grad_xt, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Spherical sliced-Wasserstein, general circular OT: n != m and / or non-uniform weights.
 * Replaces: binary_search_circle with u_weights / v_weights and unequal sample counts
 * (max_spherical_sliced_w.py:117-207, dCost :25-65, Cost :68-113), reached from sliced_cost (:284) when the
 * trainers use different source / target densities (train_W_COS.py:292-293,334-336) or the caller passes
 * weights (:289).  Follows the reference's bisection over the cut theta and its tangent exit.  p == 1 takes the
 * weighted form of the level-median formula (emd1D_circle, :210-247); slice_theta then holds the median level.
 *   wu (n) or (pairs, n), wv (m) or (pairs, m): non-negative weights summing to 1, NULL = uniform;
 *   w*_pair_stride = 0 when one weight vector is shared by all pairs (the reference's usage), else n / m.
 *   slice_theta (pairs*slices) fp32 out, may be NULL : the cut the solve ended on.
 *   coef_s / coef_t as in shw_ssw_forward_grad, both NULL for a loss-only evaluation.
 * 1 <= n, m <= 4096 on this path.
 */
SHW_API int shw_ssw_forward_general(const float* xs, const float* xt, const float* dirs,
                            const float* wu, const float* wv, long wu_pair_stride, long wv_pair_stride,
                            int pairs, int n, int m, int slices, long u_pair_stride, float p,
                            float* slice_cost, float* slice_theta, float* coef_s, float* coef_t, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Circle level: optimal transport between rows of circle COORDINATES (numbers in [0, 1]), no projection.
 * Replaces: binary_search_circle(u_values, v_values, u_weights, v_weights, p) (max_spherical_sliced_w.py:117-207)
 * and emd1D_circle(u_values, v_values, u_weights, v_weights) (:210-247), called on (rows, n) / (rows, m) coordinate
 * tensors -- the same kernels as the sliced entry points, their loaders reading one float per atom instead of
 * projecting a point on a frame.
 *   method : SHW_CIRCLE_BISECTION    = binary_search_circle for every p >= 1.  p == 1 is that function's DEFAULT (:117): the
 *                                      bisection over the cut ending in Cost's p == 1 branch (:107-108), i.e. the true circular
 *                                      W_1 -- NOT the value of emd1D_circle, whose formula leaves out the wrap segment;
 *            SHW_CIRCLE_LEVEL_MEDIAN = emd1D_circle (p must be 1);
 *            SHW_CIRCLE_AS_SLICED    = sliced_cost's own dispatch (:281-284): level-median for p == 1, bisection otherwise.
 *   u (rows, n), v (rows, m); wu / wv weights (n) / (m) shared (stride 0) or per row (stride n / m), NULL = uniform;
 *   cost (rows) out : W_p^p of every row;
 *   aux  (rows) out, may be NULL : int32 optimal shift k* (equal sizes, p != 1) or median level (p == 1), or the
 *                fp32 cut the bisection ended on (n != m or weights);
 *   grad_u (rows*n), grad_v (rows*m) out, both NULL for a value-only call : d cost[row] / d u[row, i], / d v[row, j].
 * Same size limits as the sliced entry points (8192; 4096 with weights or n != m and p != 1).
 */
#define SHW_CIRCLE_AS_SLICED 0
#define SHW_CIRCLE_BISECTION 1
#define SHW_CIRCLE_LEVEL_MEDIAN 2
SHW_API int shw_circle_ot(const float* u, const float* v, const float* wu, const float* wv, long wu_row_stride,
                          long wv_row_stride, int rows, int n, int m, float p, int method, float* cost, float* aux,
                          float* grad_u, float* grad_v, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gradients with respect to the WEIGHTS of weighted clouds on the circle (additive to ABI 3; csrc/shw_ssw_weights.hip).
 * The reference cannot serve as the statement here: binary_search_circle ends in Cost(tc.detach(), ...) (:207), so its
 * autograd differentiates Cost at a fixed cut, while with weights the minimising cut sits on a kink of cut -> Cost -- a
 * source level A_r = a_(1) + .. + a_(r) meeting a rotated target level B_j - cut -- that moves with the weights.  These
 * entries return the gradient of W(a, b) = min over the cut of Cost(cut; a, b), weights in sorted order, A / B the CDFs:
 *   fixed cut : ga_i = sum_(r >= i, r < n-1) [c(u_r, y) - c(u_(r+1), y)],  y the rotated target atom active at level A_r,
 *               gb_k = sum_(j >= k) [c(x, v_j) - c(x, v_next(j))], x the source atom active at level B_j - cut and next(j)
 *               the next target atom around the circle (one turn later after the last); the sum runs over the target's
 *               own sorted order, whatever the cut wraps.  d Cost / d cut = -(sum of all target jumps).
 *   W         : G = lambda G+ + (1 - lambda) G-, the fixed-cut gradients on the two sides of the kink (ties resolved
 *               target level first / source level first), lambda = -s- / (s+ - s-) with s+- the two slopes in the cut,
 *               clipped to [0, 1], 0.5 when both are 0.  Equivalently d W / d a_i = ga_i - s [i <= r],
 *               d W / d b_k = gb_k + s [k <= j] on either side, for the kink cut* = B_j - A_r.  With exactly tied levels
 *               (W has no gradient) the mix is a subgradient of the convex W.
 *   p == 1 level median (emd1D_circle's formula, its quirk included): in merged order, gaps g_k, signed weights +a / -b,
 *               level_k their running sum, median level_(k*), sigma_k = sign(level_k - median), H_k = sum_(t >= k) g_t
 *               sigma_t, S = H_0: the derivative w.r.t. the signed weight at k is H_k - S [k <= k*] (negated for a target atom).
 * The two sides are evaluated at t - 3e-7 and t + 3e-7 (levels compared in double), t the cut: the fp32 cut of the solve
 * is within rounding of the kink at best.  Where both slopes there have one sign (the solve also ends once nothing is left
 * to gain in the COST, possibly many kinks from the minimiser) t is moved until the window holds the minimum, and a window
 * that holds several kinks is narrowed, down to 1e-9: at most 48 evaluations per row, one when the solve ended on the kink.
 * Jumps are differences of fp32 costs summed in double in a fixed order (the same bits on every run).  Weights are taken
 * as normalised (sum 1, >= 0), so each row is returned centred, (G_i - sum_s a_s G_s / T) / T with T = sum a: the gradient
 * of the cost composed with w -> w / sum w; sum_i a_i G_i = 0.  A side of one atom gets exactly 0; an atom of weight 0 gets
 * the potential at its position.  The solve is not repeated: the cut is an INPUT, the one shw_ssw_forward_general
 * (slice_theta) / shw_circle_ot (aux) wrote for the same clouds and weights.
 *   slice_cut / cut (pairs*slices) / (rows) in; may be NULL where p == 1 takes the level median;
 *   pot_u (pairs*slices, n) / (rows, n), pot_v (pairs*slices, m) / (rows, m) out, by original index; one may be NULL.
 *   A potential row needs its side's weights (the other side's may be NULL = uniform).  1 <= n, m <= 4096.
 * The reduction over slices, grad[b,i] = sum_l w[b,l] pot[b,l,i], is shw_line_weight_grads below.
 * shw_circle_weight_potentials takes shw_circle_ot's `method`.  Return hipErrorInvalidValue on anything else. */
SHW_API int shw_ssw_weight_potentials(const float* xs, const float* xt, const float* dirs, const float* wu, const float* wv,
                                      long wu_pair_stride, long wv_pair_stride, int pairs, int n, int m, int slices,
                                      long u_pair_stride, float p, const float* slice_cut, float* pot_u, float* pot_v,
                                      void* stream);

SHW_API int shw_circle_weight_potentials(const float* u, const float* v, const float* wu, const float* wv,
                                         long wu_row_stride, long wv_row_stride, int rows, int n, int m, float p, int method,
                                         const float* cut, float* pot_u, float* pot_v, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Float64 path: equal cloud sizes, uniform weights, any p >= 1 (additive to ABI 3).
 * The reference takes its arithmetic type from its input (`dtype = u_values.dtype`, max_spherical_sliced_w.py:153-160;
 * _fast.py:157, :221): double clouds and double directions give a double loss and double gradients.  These entries are
 * that call: the conventions of the header comment with `double` in place of fp32, kernels of their own
 * (csrc/shw_ssw_f64.hip: one workgroup per (pair, slice), double atan2, every sum in a fixed order -- results are
 * bit-identical from run to run).  n == m is required and 1 <= n <= SHW_MAX_POINTS_F64; anything else returns 1.
 * Weighted and unequal-size clouds: the *_general_f64 entries further down, or the fp32 entry points.
 */

/* Largest point count per cloud the float64 entry points accept (SHW_MAX_POINTS_F64). */
SHW_API int shw_max_points_f64(void);

/* Replaces: `U, _ = torch.linalg.qr(Z)` (max_spherical_sliced_w.py:308, _fast.py:318) on double Z, as
 * shw_stiefel_frames: Householder steps with LAPACK's sign convention, one thread per (3, 2) matrix. */
SHW_API int shw_stiefel_frames_f64(const double* z, long count, double* u, void* stream);

/* Replaces: sliced_cost on double tensors up to, not including, the mean over slices (max_spherical_sliced_w.py:251-286,
 * _fast.py:258-295; binary_search_circle :117-207 for p != 1 as min over shifts k of c(k), emd1D_circle :210-247 for
 * p == 1) -- shw_ssw_forward and shw_ssw_forward_grad in one entry.
 *   slice_cost (pairs*slices) out; slice_shift (pairs*slices) int32 out, may be NULL: k* (p != 1) or median level (p == 1);
 *   coef_s, coef_t (pairs*slices*n) double scratch, both NULL for a loss-only call: d cost(b,l) / d coord in ORIGINAL
 *   point order, the input of shw_ssw_backward_points_f64. */
SHW_API int shw_ssw_forward_f64(const double* xs, const double* xt, const double* dirs, int pairs, int n, int m,
                                int slices, long u_pair_stride, double p, double* slice_cost, int32_t* slice_shift,
                                double* coef_s, double* coef_t, void* stream);

/* Replaces: autograd through gather -> sort -> atan2 -> normalize -> matmul (:163-164, :270-279) on double tensors, as
 * shw_ssw_backward_points: row b of both gradients is multiplied by pair_w[b] + total_w[0] (NULL terms count as 0, both
 * NULL = 1); every gradient element is summed over the slices in a fixed order. */
SHW_API int shw_ssw_backward_points_f64(const double* xs, const double* xt, const double* dirs, const double* coef_s,
                                        const double* coef_t, int pairs, int n, int m, int slices, long u_pair_stride,
                                        double scale, const double* pair_w, const double* total_w, double* grad_xs,
                                        double* grad_xt, void* stream);

/* Replaces: torch.mean(w1) (:286) and the `w1 += mean(...)` loop over the batch (_fast.py:291-293) in double, as
 * shw_ssw_reduce: pair_loss (pairs), total (2, may be NULL) = {sum_b pair_loss[b], that / pairs}. */
SHW_API int shw_ssw_reduce_f64(const double* slice_cost, int pairs, int slices, double scale, double* pair_loss,
                               double* total, void* stream);

/* Replaces: binary_search_circle (:117-207) and emd1D_circle (:210-247) on double rows of circle coordinates, equal
 * sizes, no weights; `method` as in shw_circle_ot.  SHW_CIRCLE_BISECTION at p == 1 is the true circular W_1, for equal
 * sizes and uniform weights again min_k c(k).
 *   u, v (rows, n); cost (rows) out; aux (rows) int32 out, may be NULL: k* or the median level;
 *   grad_u, grad_v (rows*n) out, both NULL for a value-only call. */
SHW_API int shw_circle_ot_f64(const double* u, const double* v, int rows, int n, int m, double p, int method,
                              double* cost, int32_t* aux, double* grad_u, double* grad_v, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Float64 general circular OT: weighted and / or unequal-size clouds, any p >= 1 (additive to ABI 3).
 * The double form of shw_ssw_forward_general / shw_circle_ot for the shapes the entries above refuse: kernels of
 * csrc/shw_ssw_f64_general.hip, one workgroup per (pair, slice), every sum in a fixed order -- results are bit-identical
 * from run to run.  1 <= n, m <= SHW_MAX_POINTS_F64_GENERAL; anything else returns 1 without touching the device.
 * p != 1 (and SHW_CIRCLE_BISECTION at every p) is the DEFINITION min over the cut theta in [-1, 1] of Cost(theta)
 * (Cost: max_spherical_sliced_w.py:68-113), found exactly -- Cost is convex and piecewise linear in theta -- and not
 * the reference's stopping rule (:191-200), which ends up to 1.6e-11 above it (fixture G14).
 */

/* Largest point count per cloud the general float64 entry points accept (SHW_MAX_POINTS_F64_GENERAL). */
SHW_API int shw_max_points_f64_general(void);

/* Replaces: sliced_cost on double tensors with n != m and / or weights, up to the mean over slices
 * (max_spherical_sliced_w.py:251-286, _fast.py:258-295: sort :262-269, cumsum of the gathered weights :161-167,
 * binary_search_circle :117-207 with dCost :25-65 and Cost :68-113 for p != 1, emd1D_circle :210-247 for p == 1).
 * Arguments as shw_ssw_forward_general, in double:
 *   wu (n) or (pairs, n), wv (m) or (pairs, m): weights summing to 1, NULL = uniform; w*_pair_stride = 0 for a shared
 *   row, else the doubles between consecutive pairs' rows;
 *   slice_cost (pairs*slices) out; slice_theta (pairs*slices) out, may be NULL: the cut theta* (p != 1) or the median
 *   level (p == 1);
 *   coef_s (pairs*slices*n), coef_t (pairs*slices*m) double scratch, both NULL for a loss-only call: d cost(b,l) / d coord
 *   at the detached cut (:207) in ORIGINAL point order, the input of shw_ssw_backward_points_general_f64. */
SHW_API int shw_ssw_forward_general_f64(const double* xs, const double* xt, const double* dirs, const double* wu,
                                        const double* wv, long wu_pair_stride, long wv_pair_stride, int pairs, int n,
                                        int m, int slices, long u_pair_stride, double p, double* slice_cost,
                                        double* slice_theta, double* coef_s, double* coef_t, void* stream);

/* Replaces: autograd through gather -> sort -> atan2 -> normalize -> matmul (:163-164, :270-279) on double tensors of
 * two sizes: shw_ssw_backward_points_f64 with n != m allowed -- coef_s (pairs*slices*n), coef_t (pairs*slices*m),
 * grad_xs (pairs, n, 3), grad_xt (pairs, m, 3); pair_w / total_w / scale as there; fixed-order sums. */
SHW_API int shw_ssw_backward_points_general_f64(const double* xs, const double* xt, const double* dirs,
                                                const double* coef_s, const double* coef_t, int pairs, int n, int m,
                                                int slices, long u_pair_stride, double scale, const double* pair_w,
                                                const double* total_w, double* grad_xs, double* grad_xt, void* stream);

/* Replaces: binary_search_circle (:117-207) and emd1D_circle (:210-247) on double rows of circle coordinates with
 * weights and / or n != m; `method` as in shw_circle_ot, weights as in shw_ssw_forward_general_f64 (per row).
 *   u (rows, n), v (rows, m); cost (rows) out; aux (rows) out, may be NULL: the cut theta* or the median level;
 *   grad_u (rows*n), grad_v (rows*m) out, both NULL for a value-only call. */
SHW_API int shw_circle_ot_general_f64(const double* u, const double* v, const double* wu, const double* wv,
                                      long wu_row_stride, long wv_row_stride, int rows, int n, int m, double p, int method,
                                      double* cost, double* aux, double* grad_u, double* grad_v, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Spherical sliced-Wasserstein on S^(dim-1): points of dimension 2 <= dim <= 64, fp32 (additive to ABI 3).
 * The reference reads the point dimension from its input (`d = Xs.shape[1]`, max_spherical_sliced_w.py:304; frames
 * (L, d, 2), :307-308); only the projection (:270-271) and its backward depend on it.  These entries (kernels of
 * csrc/shw_ssw_dim.hip) write the circle coordinates of both clouds to a workspace, run shw_circle_ot on them -- every
 * size class, every p >= 1, n != m and weights -- and turn its gradient rows into point gradients:
 *   clouds (pairs, points, dim); dirs (slices, dim, 2) shared (u_pair_stride = 0) or (pairs, slices, dim, 2)
 *   (u_pair_stride >= slices*dim*2 floats).
 * Limits: those of shw_circle_ot (8192 points per cloud; 4096 with weights, or with n != m at p != 1).  dim outside
 * 2..64 or a size outside the limits returns 1 without touching the device.  dim = 3 is accepted and gives the
 * coordinates of the R^3 kernels bit for bit (the same sum fma(x_d, U[d][k], acc), d ascending from +0).
 */

/* Largest point dimension of the entries of this section (64). */
SHW_API int shw_max_point_dim(void);

/* Replaces: `U, _ = torch.linalg.qr(Z)` (:308) for Z (count, dim, 2), as shw_stiefel_frames: two Householder steps with
 * LAPACK's sign convention, one thread per matrix.  z (count, dim, 2) in, u (count, dim, 2) out. */
SHW_API int shw_stiefel_frames_dim(const float* z, long count, int dim, float* u, void* stream);

/* Replaces: projection, normalise and circle coordinate (:270-279) of ONE cloud.
 *   x (pairs, n, dim); coords (pairs*slices*n) out: coords[(b*slices + l)*n + i] in [0, 1], the coordinate of point i
 *   of pair b on the great circle of frame l.  An all-zero point gets coordinate 0. */
SHW_API int shw_ssw_coords_dim(const float* x, const float* dirs, int pairs, int n, int dim, int slices,
                               long u_pair_stride, float* coords, void* stream);

/* Bytes of the workspace of shw_ssw_forward_dim: the two coordinate arrays, 4 * pairs * slices * (n + m). */
SHW_API size_t shw_ssw_dim_workspace_bytes(int pairs, int n, int m, int slices);

/* Replaces: sliced_cost (:251-286, _fast.py:258-295) up to, not including, the mean over slices, for any dim:
 * shw_ssw_coords_dim on both clouds, then shw_circle_ot with SHW_CIRCLE_AS_SLICED on the pairs*slices rows.
 *   wu (n) or (pairs, n), wv (m) or (pairs, m): weights as in shw_ssw_forward_general, NULL = uniform;
 *   w*_pair_stride = 0 for a row shared by all pairs (one circle-level launch), else the floats between consecutive
 *   pairs' rows (one circle-level launch per pair);
 *   workspace : shw_ssw_dim_workspace_bytes(pairs, n, m, slices) bytes; holds the coordinates after the call;
 *   slice_cost (pairs*slices) out; slice_aux (pairs*slices) out, may be NULL: `aux` of shw_circle_ot (int32 shift or
 *   median level, or the fp32 cut);
 *   coef_s (pairs*slices*n), coef_t (pairs*slices*m) out, both NULL for a loss-only call: d cost(b,l) / d coord in
 *   ORIGINAL point order, the input of shw_ssw_backward_points_dim. */
SHW_API int shw_ssw_forward_dim(const float* xs, const float* xt, const float* dirs, const float* wu, const float* wv,
                                long wu_pair_stride, long wv_pair_stride, int pairs, int n, int m, int dim, int slices,
                                long u_pair_stride, float p, void* workspace, float* slice_cost, float* slice_aux,
                                float* coef_s, float* coef_t, void* stream);

/* shw_ssw_backward_points for any dim (n != m allowed): grad_xs (pairs, n, dim), grad_xt (pairs, m, dim),
 *   grad_x[b,i,:] = scale (pair_w[b] + total_w[0]) sum_l coef[b,l,i] (-b_ U_l[:,0] + a_ U_l[:,1]) / (2 pi (a_^2 + b_^2)),
 *   (a_, b_) = U_l^T x[b,i] recomputed from the point, zero where a_^2 + b_^2 == 0; pair_w / total_w as there.
 * One thread owns a gradient row and adds the slices in ascending order: bit-identical from run to run. */
SHW_API int shw_ssw_backward_points_dim(const float* xs, const float* xt, const float* dirs, const float* coef_s,
                                        const float* coef_t, int pairs, int n, int m, int dim, int slices,
                                        long u_pair_stride, float scale, const float* pair_w, const float* total_w,
                                        float* grad_xs, float* grad_xt, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Spherical sliced-Wasserstein: gradients with respect to the slicing frames (additive to ABI 3; kernels of
 * csrc/shw_ssw_dirs.hip).  The coefficient rows every training-form forward writes (coef[b,l,i] = d cost(b,l) /
 * d coord[b,l,i], original point order) folded with d coord / d U instead of d coord / d x.  With (a_, b_) = U_l^T x_i,
 * r2 = a_^2 + b_^2 and coord = (atan2(-b_, -a_) + pi) / (2 pi):
 *   grad_dirs[b,l,:,0] = sc_b sum_i coef[b,l,i] (-b_i) / (2 pi r2_i) x_i
 *   grad_dirs[b,l,:,1] = sc_b sum_i coef[b,l,i] ( a_i) / (2 pi r2_i) x_i,    sc_b = scale (pair_w[b] + total_w[0]),
 * summed over the points of both clouds (coef_s with xs, coef_t with xt); a point with r2 == 0 adds 0, the guard of the
 * point-gradient entries.  pair_w / total_w as in shw_ssw_backward_points (NULL terms count as 0, both NULL = 1).
 *   grad_dirs (pairs, slices, dim, 2) out, ALWAYS one row per (pair, slice) -- the convention of shw_esw_backward_dirs:
 *   frames shared by several pairs (u_pair_stride = 0) sum their rows over the pairs on the host side.
 * The cost does not change when the frame is rotated in its plane or scaled, so every row satisfies
 *   <g[:,0], u2> - <g[:,1], u1> = 0   and   <g[:,0], u1> + <g[:,1], u2> = 0   up to rounding.
 * Limits: 1 <= n, m <= shw_max_points() (float32), the larger of shw_max_points_f64() and
 * shw_max_points_f64_general() (float64, one entry for both float64 paths: n != m allowed); 2 <= dim <= 64.  A null
 * pointer or a size outside the limits returns 1 without touching the device; pairs == 0 or slices == 0 is a no-op.
 * More than 65535 pairs go out as several launches.  Sums run in a fixed order without atomics: the same bits on
 * every run.
 */
SHW_API int shw_ssw_backward_dirs(const float* xs, const float* xt, const float* dirs, const float* coef_s,
                                  const float* coef_t, int pairs, int n, int m, int slices, long u_pair_stride,
                                  float scale, const float* pair_w, const float* total_w, float* grad_dirs, void* stream);

SHW_API int shw_ssw_backward_dirs_dim(const float* xs, const float* xt, const float* dirs, const float* coef_s,
                                      const float* coef_t, int pairs, int n, int m, int dim, int slices,
                                      long u_pair_stride, float scale, const float* pair_w, const float* total_w,
                                      float* grad_dirs, void* stream);

SHW_API int shw_ssw_backward_dirs_f64(const double* xs, const double* xt, const double* dirs, const double* coef_s,
                                      const double* coef_t, int pairs, int n, int m, int slices, long u_pair_stride,
                                      double scale, const double* pair_w, const double* total_w, double* grad_dirs,
                                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * Euclidean sliced-Wasserstein (the notebooks' SWD baseline).
 * Replaces: sliced_wasserstein_distance (Wasserstein_flow_problem/Flow_cube.ipynb:280-292): projection on unit
 * directions, per-slice sort of both projected sequences, sum of |sorted difference|^p.
 *   xs, xt (pairs, n, 3) -- equal counts, as the notebook code requires; thetas (slices, 3) shared
 *   (theta_pair_stride = 0) or (pairs, slices, 3) (stride = slices*3); p >= 1; n <= 4096; pairs <= 65535
 *   (pairs ride on gridDim.y in the two backward kernels).
 *   slice_sum (pairs*slices) out : S_l = sum_i |u_(i) - v_(i)|^p     (the notebook's outer (mean_l S_l)^(1/p)
 *                                  is host arithmetic on `slices` numbers)
 *   coef_s / coef_t (pairs*slices*n) scratch, both NULL for a value-only call : d S_l / d projection in
 *   original point order; shw_esw_backward_points turns them into
 *   grad_x[b,i,:] = sum_l slice_w[b,l] * coef[b,l,i] * theta[b,l,:]  (slice_w = upstream gradient of S).
 */
SHW_API int shw_esw_forward(const float* xs, const float* xt, const float* thetas, int pairs, int n, int slices,
                    long theta_pair_stride, float p, float* slice_sum, float* coef_s, float* coef_t, void* stream);

SHW_API int shw_esw_backward_points(const float* thetas, const float* coef_s, const float* coef_t, const float* slice_w,
                            int pairs, int n, int slices, long theta_pair_stride,
                            float* grad_xs, float* grad_xt, void* stream);

/* Gradient w.r.t. the directions (max_sliced_wasserstein_distance, Flow_cube.ipynb:294-323, ascends on them):
 *   grad_thetas[b,l,:] = slice_w[b,l] * sum_i (coef_s[b,l,i] * xs[b,i,:] + coef_t[b,l,i] * xt[b,i,:]),
 * always (pairs, slices, 3); directions shared by several pairs sum their rows on the host side. */
SHW_API int shw_esw_backward_dirs(const float* xs, const float* xt, const float* coef_s, const float* coef_t,
                          const float* slice_w, int pairs, int n, int slices, float* grad_thetas, void* stream);

/* The same three entries for points of dimension `dim`, 1 <= dim <= 64 (the notebooks' ASWD projects points
 * augmented to 6 coordinates): xs, xt (pairs, n, dim); thetas (slices, dim) shared (theta_pair_stride = 0) or
 * (pairs, slices, dim) (stride >= slices*dim); grad_xs / grad_xt (pairs, n, dim); grad_thetas (pairs, slices, dim).
 * Keys are sum_d x[i,d] * theta[l,d] accumulated in the order d = 0..dim-1; coef_s / coef_t as above.  n <= 4096,
 * pairs <= 65535 in the backward entries.  Gradients are reduced in a fixed order (no atomics). */
SHW_API int shw_esw_forward_dim(const float* xs, const float* xt, const float* thetas, int pairs, int n, int dim,
                                int slices, long theta_pair_stride, float p, float* slice_sum, float* coef_s,
                                float* coef_t, void* stream);

SHW_API int shw_esw_backward_points_dim(const float* thetas, const float* coef_s, const float* coef_t,
                                        const float* slice_w, int pairs, int n, int dim, int slices,
                                        long theta_pair_stride, float* grad_xs, float* grad_xt, void* stream);

SHW_API int shw_esw_backward_dirs_dim(const float* xs, const float* xt, const float* coef_s, const float* coef_t,
                                      const float* slice_w, int pairs, int n, int dim, int slices, float* grad_thetas,
                                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * Generalised sliced-Wasserstein (csrc/shw_gsw.hip): the sort-and-difference of the notebooks' GSWD / max-GSWD /
 * DSWD family (Wasserstein_flow_problem/Flow_cube.ipynb, the cell that starts with `def rand_projections`) for
 * defining functions other than a dot product with a direction.  float32.
 *
 * Rows of keys the caller computed.  Replaces the sort / |difference|^p / sum lines of gsw_nn_1, gsw_nn_3,
 * max_gsw_nn_1 and max_gsw_nn_3 (keys = the transposed output of the caller's network), and serves any other
 * defining function evaluated in torch.
 *   u, v (rows, n) contiguous; 1 <= n <= 4096; p >= 1; rows >= 0, any count.
 *   row_sum (rows) out : sum_i |u_(i) - v_(i)|^p, u_(.) and v_(.) the rows sorted ascending.
 *   coef_u / coef_v (rows, n) out, both NULL for a value-only call : d row_sum[r] / d u[r,i] and d row_sum[r] / d v[r,i]
 *   in original element order (d|D|^p/dD of the sorted difference scattered through the sort's indices, negated for
 *   v; 0 at a zero difference for p = 1, as the Euclidean entries).
 * Returns hipErrorInvalidValue on a null pointer (other than both coefficient rows), one coefficient row without the
 * other, n outside 1..4096, rows < 0 or p < 1. */
SHW_API int shw_gsw_rows_forward(const float* u, const float* v, long rows, int n, float p, float* row_sum,
                                 float* coef_u, float* coef_v, void* stream);

/* Circular defining function g(x, theta) = || x - r theta ||_2, fused: keys, sorts and sums in one kernel, no
 * (pairs, slices, n) key matrix in memory.  Replaces GSWD_circular, max_GSWD_circular and circular_function.
 *   xs, xt (pairs, n, dim), 1 <= dim <= 64, 1 <= n <= 4096; thetas (slices, dim) shared (theta_pair_stride = 0) or
 *   (pairs, slices, dim) (stride >= slices*dim); r any float; p >= 1; pairs * slices < 2^31.
 *   The key of point i on slice l is sqrt(sum_d (x[i,d] - r*theta[l,d])^2), from the differences, accumulated in the
 *   order d = 0..dim-1 (r*theta[l,d] rounded first, as the notebook's `theta * r`).
 *   slice_sum (pairs*slices) out : S_l = sum_i |key_s(i) - key_t(i)|^p over the sorted keys.
 *   coef_s / coef_t (pairs*slices*n) scratch, both NULL for a value-only call : (d S_l / d key) / key in original
 *   point order, 0 where key == 0 -- a point exactly at r theta contributes gradient 0 where the notebook's autograd
 *   yields NaN (the one deliberate deviation).  The two backward entries read them:
 *   grad_x[b,i,:]      = sum_l slice_w[b,l] * coef[b,l,i] * (x[b,i,:] - r theta[b,l,:])
 *   grad_thetas[b,l,:] = -r slice_w[b,l] * sum_i ( coef_s[b,l,i] * (xs[b,i,:] - r theta[b,l,:])
 *                                                + coef_t[b,l,i] * (xt[b,i,:] - r theta[b,l,:]) ),
 *   grad_xs / grad_xt (pairs, n, dim); grad_thetas always (pairs, slices, dim) -- directions shared by several pairs
 *   sum their rows on the host side.  pairs <= 65535 in the backward entries (pairs ride on gridDim.y).  Gradients
 *   are reduced in a fixed order (no atomics).
 * Returns hipErrorInvalidValue on a null pointer, dim outside 1..64, n outside 1..4096, a pair stride shorter than
 * slices*dim, p < 1 or pairs over the limit. */
SHW_API int shw_gsw_circular_forward(const float* xs, const float* xt, const float* thetas, int pairs, int n, int dim,
                                     int slices, long theta_pair_stride, float r, float p, float* slice_sum,
                                     float* coef_s, float* coef_t, void* stream);

SHW_API int shw_gsw_circular_backward_points(const float* xs, const float* xt, const float* thetas, const float* coef_s,
                                             const float* coef_t, const float* slice_w, int pairs, int n, int dim,
                                             int slices, long theta_pair_stride, float r, float* grad_xs,
                                             float* grad_xt, void* stream);

SHW_API int shw_gsw_circular_backward_dirs(const float* xs, const float* xt, const float* thetas, const float* coef_s,
                                           const float* coef_t, const float* slice_w, int pairs, int n, int dim,
                                           int slices, long theta_pair_stride, float r, float* grad_thetas,
                                           void* stream);

/* ---------------------------------------------------------------------------------------------
 * 1-D optimal transport on the line (csrc/shw_line_ot.hip): two weighted empirical measures of n and m atoms, n != m
 * allowed.  cost = W_p^p = int_0^1 |F_u^-1(t) - F_v^-1(t)|^p dt (the quantile merge), mass-normalised: for n == m and
 * no weights it equals the Euclidean / generalised entries' sum divided by n.  float32, 1 <= n, m <= 4096, p >= 1.
 * Weights (both forms): a pointer or NULL (uniform) per side, and a stride in floats from one row's (pair's) weights to
 * the next, 0 = one weight row shared by all; a non-zero stride must be >= the side's count.  Weights are >= 0 and
 * finite with a positive sum per row; the kernel divides by the sum.  The sign and the sum are NOT checked on the
 * device: a row whose weights sum to 0 or less yields, in bounded time, a value that means nothing.  A zero weight contributes nothing
 * and gets coefficient 0.  With both sides NULL the CDFs are the exact integer grid of lcm(n, m) steps.
 * Gradients with respect to the weights come from the *_pot entries below, not from these.  Cost and coefficients are
 * the same bits on every run.
 *
 * Rows of keys the caller computed (any defining function).
 *   u (rows, n), v (rows, m) contiguous; rows >= 0, any count.
 *   row_cost (rows) out.
 *   coef_u (rows, n) / coef_v (rows, m) out, both NULL for a value-only call : d row_cost[r] / d u[r,i] and
 *   d row_cost[r] / d v[r,j] in original element order: the sum over the merged intervals in which the atom is active of
 *   delta * p |d|^(p-1) sgn(d), d = u - v (negated for v; 0 at d == 0).
 * Returns hipErrorInvalidValue on a null pointer (other than weights and both coefficient rows), one coefficient row
 * without the other, n or m outside 1..4096, rows < 0, p < 1, or a weight stride that is non-zero with a null pointer or
 * shorter than the count. */
SHW_API int shw_line_rows_forward(const float* u, const float* v, long rows, int n, int m, float p,
                                  const float* u_weights, const float* v_weights, long u_weight_stride,
                                  long v_weight_stride, float* row_cost, float* coef_u, float* coef_v, void* stream);

/* Fused Euclidean projection: xs (pairs, n, dim), xt (pairs, m, dim), 1 <= dim <= 64, pairs <= 65535; thetas
 * (slices, dim) shared (theta_pair_stride = 0) or (pairs, slices, dim) (stride >= slices*dim).  The key of point i on
 * slice l is sum_d x[i,d] * theta[l,d] accumulated in the order d = 0..dim-1 (the keys of shw_esw_forward_dim, bit for
 * bit); no (pairs, slices, n) key matrix is formed.  Weights are per pair: stride 0 or >= the count.
 *   slice_cost (pairs*slices) out : W_p^p of the two projected measures.
 *   coef_s (pairs*slices*n) / coef_t (pairs*slices*m) scratch, both NULL for a value-only call : d slice_cost / d key
 *   in original point order; the two backward entries read them.
 * Returns hipErrorInvalidValue as the rows form, and on dim outside 1..64, pairs outside 0..65535 or a pair stride
 * shorter than slices*dim. */
SHW_API int shw_line_esw_forward(const float* xs, const float* xt, const float* thetas, int pairs, int n, int m, int dim,
                                 int slices, long theta_pair_stride, float p, const float* u_weights,
                                 const float* v_weights, long u_weight_stride, long v_weight_stride, float* slice_cost,
                                 float* coef_s, float* coef_t, void* stream);

/* grad_xs[b,i,:] = sum_l slice_w[b,l] * coef_s[b,l,i] * theta[b,l,:] (pairs, n, dim), and grad_xt (pairs, m, dim) from
 * coef_t; slices summed in the order l = 0..slices-1.  Same limits as the forward entry. */
SHW_API int shw_line_esw_backward_points(const float* thetas, const float* coef_s, const float* coef_t,
                                         const float* slice_w, int pairs, int n, int m, int dim, int slices,
                                         long theta_pair_stride, float* grad_xs, float* grad_xt, void* stream);

/* grad_thetas[b,l,:] = slice_w[b,l] * ( sum_i coef_s[b,l,i] * xs[b,i,:] + sum_j coef_t[b,l,j] * xt[b,j,:] ), always
 * (pairs, slices, dim) -- directions shared by several pairs sum their rows on the host side.  Reduced in a fixed
 * order (no atomics).  Same limits as the forward entry. */
SHW_API int shw_line_esw_backward_dirs(const float* xs, const float* xt, const float* coef_s, const float* coef_t,
                                       const float* slice_w, int pairs, int n, int m, int dim, int slices,
                                       float* grad_thetas, void* stream);

/* Gradients with respect to the weights (the weighted path only; the entries above are unchanged and give none).
 *
 * Per row: sorted values u_(0..n-1), v_(0..m-1); normalised masses abar = a / T_a, bbar = b / T_b (T the sum of the raw
 * weights); CDF ends A_r, B_j, the last end of each side 1.  Walk the merged ends in ascending order; ON EQUAL LEVELS THE
 * u END COMES FIRST, and segments of zero width count.  Segment k has the active atoms (i_k, j_k) and the cost
 * c_k = |u_(i_k) - v_(j_k)|^p; it is closed by A_i (then i advances) or by B_j (then j advances); the walk stops at
 * (n-1, m-1).  The jump at the end that closes segment k is c_k - c_(k+1): phi_r when the end is A_r, psi_j when it is
 * B_j; the last ends have none.  So phi_r = c(r, j) - c(r+1, j) with j the first v atom with B_j >= A_r, and
 * psi_j = c(i, j) - c(i, j+1) with i the first u atom with A_i > B_j (the last atom when there is none): one tie rule for
 * both sides, without which the pair is not a subgradient.
 *   f_r = sum_{s=r}^{n-2} phi_s, f_(n-1) = 0;   g_j = sum_{s=j}^{m-2} psi_s, g_(m-1) = 0
 *   d cost / d a_(r) = (f_r - sum_s abar_s f_s) / T_a        d cost / d b_(j) = (g_j - sum_s bbar_s g_s) / T_b
 * written at the atom's original index.  sum_i a_i * grad_i = 0 on each side (the cost does not change when a side's
 * weights are scaled), sum abar f + sum bbar g + c_last = cost, and a side with one atom gets exactly 0.  An atom of
 * weight 0 gets the potential at its position -- the derivative to the right, the rate at which the cost changes when the
 * atom gains mass -- while its value coefficient stays 0.  The jumps are differences of float32 costs, summed in float32
 * inside a lane and in double across the 64 lanes and in the mean; the CDF is the 2^30 grid of the entries above.  Cost and
 * coefficients are the bits of the entries without potentials, and everything is the same bits on every run.
 *
 *   pot_u (rows, n) / pot_v (rows, m) out (fused form: (pairs*slices, n) / (pairs*slices, m)), each may be NULL: the
 *   gradient of that row's (slice's) cost with respect to that row's (pair's) RAW weights.  A row needs its side's weights.
 *   coef_* may be NULL with pot_* given (gradients with respect to the weights only).
 * Return hipErrorInvalidValue as the entries without potentials, and on a potential row for a side whose weights are NULL. */
SHW_API int shw_line_rows_forward_pot(const float* u, const float* v, long rows, int n, int m, float p,
                                      const float* u_weights, const float* v_weights, long u_weight_stride,
                                      long v_weight_stride, float* row_cost, float* coef_u, float* coef_v, float* pot_u,
                                      float* pot_v, void* stream);

SHW_API int shw_line_esw_forward_pot(const float* xs, const float* xt, const float* thetas, int pairs, int n, int m,
                                     int dim, int slices, long theta_pair_stride, float p, const float* u_weights,
                                     const float* v_weights, long u_weight_stride, long v_weight_stride,
                                     float* slice_cost, float* coef_s, float* coef_t, float* pot_u, float* pot_v,
                                     void* stream);

/* The reduction over slices: grad[b,i] = sum_l slice_w[b,l] * pot[b,l,i], pot (pairs, slices, count), slice_w
 * (pairs, slices), slices summed in the order l = 0..slices-1; shared == 0: grad (pairs, count).  shared != 0 (one weight
 * row shared by the pairs): summed over the pairs as well, grad (count): the pairs*slices rows in ascending order, in groups
 * of 64 rows whose sums are then added in ascending order; this needs `workspace`, device memory of
 * shw_line_weight_grads_workspace_bytes(pairs, slices, count, shared) bytes (0 bytes: NULL is fine).  The rows form with
 * shared weights is pairs = 1, slices = rows.  No atomics: the same bits on every run.  1 <= count <= 4096,
 * 0 <= pairs <= 65535, pairs*slices <= 65535*64 when shared; hipErrorInvalidValue otherwise and on null pointers. */
SHW_API size_t shw_line_weight_grads_workspace_bytes(int pairs, int slices, int count, int shared);

SHW_API int shw_line_weight_grads(const float* pot, const float* slice_w, int pairs, int slices, int count, int shared,
                                  void* workspace, float* grad, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Log-domain Sinkhorn distance (comparison metric); value-only entry point.
 * Replaces: log_Sinkhorn_Distance_Loss.forward and log_N_Sinkhorn_Distance_Loss.forward
 * (/root/reference/Comparison_Wasserstein_with_Chamfer_distance/losses/sinkhorn.py:14-63, :104-157), called at
 * main_rotation.py:207-211.
 *   x (pairs, n, 3), y (pairs, m, 3); eps > 0; max_iter >= 0; norm_p = p of the coordinate-wise cost
 *   sum_d |x_d - y_d|^p ('L2' -> 2); cost_pow = N of the log_N variant (1 for the plain class);
 *   thresh = the convergence threshold on mean_b sum_i |u - u_old| (the reference hard-codes 1e-9).
 *   pairs <= 65535 (gridDim.y).
 *   workspace : shw_sinkhorn_workspace_bytes(pairs, n, m) bytes of device memory (duals, statistics);
 *               after the call its first pairs*n floats hold u and the next pairs*m floats hold v.
 *   cost (pairs) out : sum_ij exp(M_ij) C_ij  (before the batch reduction and the 1/N power, host side);
 *   plan, cost_matrix : optional dense (pairs, n, m) outputs P and C that the reference returns; NULL to skip.
 * The cost matrix is never stored unless asked for; the iteration count is fixed at enqueue time and the
 * convergence test is a device-side flag that turns the remaining launches into no-ops (no host sync).
 */
SHW_API size_t shw_sinkhorn_workspace_bytes(int pairs, int n, int m);

SHW_API int shw_sinkhorn_forward(const float* x, const float* y, int pairs, int n, int m, float eps, int max_iter,
                         int norm_p, int cost_pow, float thresh, void* workspace, float* cost, float* plan,
                         float* cost_matrix, void* stream);

/* Log-domain Sinkhorn with gradients w.r.t. both clouds.
 * Replaces: autograd through log_Sinkhorn_Distance_Loss.forward (sinkhorn.py:35-49: the iterations are differentiable).
 * shw_sinkhorn_forward_train runs the same iterations and keeps the trajectory of the duals (u_t, v_t), t = 0..T, in
 * `workspace` (shw_sinkhorn_train_workspace_bytes(pairs, n, m, max_iter) bytes: 2 (max_iter + 2) pairs (n + m) floats);
 * shw_sinkhorn_backward walks it from t = T down to 1, two kernels per iteration, recomputing the transport weights
 * from the points (nothing dense is stored), every gradient row owned by one thread (deterministic):
 *   grad_cost (pairs) in : upstream gradient of cost[b];  grad_x (pairs, n, 3), grad_y (pairs, m, 3) out (overwritten).
 * The workspace must be passed unchanged from the forward to the backward call (same sizes, eps, max_iter, norms).
 * plan, cost_matrix (ABI 3): optional dense (pairs, n, m) outputs P and C of the SAME solve (NULL to skip), plain values: the
 * gradient this library computes is that of `cost`.
 */
SHW_API size_t shw_sinkhorn_train_workspace_bytes(int pairs, int n, int m, int max_iter);

SHW_API int shw_sinkhorn_forward_train(const float* x, const float* y, int pairs, int n, int m, float eps, int max_iter,
                                       int norm_p, int cost_pow, float thresh, void* workspace, float* cost, float* plan,
                                       float* cost_matrix, void* stream);

SHW_API int shw_sinkhorn_backward(const float* x, const float* y, int pairs, int n, int m, float eps, int max_iter,
                                  int norm_p, int cost_pow, void* workspace, const float* grad_cost, float* grad_x,
                                  float* grad_y, void* stream);

/* The same backward for a loss that also consumes the plan P and the cost matrix C of shw_sinkhorn_forward_train
 * (the reference's P and C are autograd-visible, sinkhorn.py:46-60).  Additive, ABI 3.
 *   grad_cost (pairs), grad_plan (pairs, n, m), grad_cost_matrix (pairs, n, m) in : upstream gradients of cost, P and C;
 *   each may be NULL (= zero).  With Ghat_ij = g C_ij + GP_ij the recursion starts from
 *     ubar_i = sum_j P_ij Ghat_ij / eps,  vbar_j = sum_i P_ij Ghat_ij / eps,
 *     K_ij = P_ij (g (1 - C_ij / eps) - GP_ij / eps) + GC_ij,  gx_i = sum_j K_ij dC_ij/dx_i,  gy_j = sum_i K_ij dC_ij/dy_j
 *   and then walks the iterations exactly as shw_sinkhorn_backward does.  The two dense tensors are read once per side
 *   (x side: one wave per row, lanes along j; y side: one thread per column); no atomics, deterministic.
 *   With grad_plan = grad_cost_matrix = NULL the result equals shw_sinkhorn_backward's up to rounding (not bit for bit:
 *   callers that need the bits call that entry). */
SHW_API int shw_sinkhorn_backward_plan(const float* x, const float* y, int pairs, int n, int m, float eps, int max_iter,
                                       int norm_p, int cost_pow, void* workspace, const float* grad_cost,
                                       const float* grad_plan, const float* grad_cost_matrix, float* grad_x, float* grad_y,
                                       void* stream);

/* Soft correspondences without dense tensors: the barycentric map of the plan, from the same single solve as the cost.
 *   map (pairs, n, 3) out : T_i = sum_j P_ij y_j / r_i;  row_sum (pairs, n) out : r_i = sum_j P_ij;  cost (pairs) out as
 *   shw_sinkhorn_forward_train (same bits).  A row whose whole sum underflowed (r_i = 0) gets T_i = 0 and passes no gradient.
 *   workspace : shw_sinkhorn_train_workspace_bytes(pairs, n, m, max_iter), passed unchanged to shw_sinkhorn_map_backward.
 * shw_sinkhorn_map_backward: grad_map (pairs, n, 3) in, grad_cost (pairs) in or NULL; grad_x, grad_y out (overwritten).
 *   It is shw_sinkhorn_backward_plan with the implicit rank-3 cotangent GP_ij = G_i . (y_j - T_i) / r_i, GC = 0, and the
 *   direct term gy_j += sum_i P_ij G_i / r_i; nothing (pairs, n, m) is read or written. */
SHW_API int shw_sinkhorn_map_forward(const float* x, const float* y, int pairs, int n, int m, float eps, int max_iter,
                                     int norm_p, int cost_pow, float thresh, void* workspace, float* cost, float* map,
                                     float* row_sum, void* stream);

SHW_API int shw_sinkhorn_map_backward(const float* x, const float* y, int pairs, int n, int m, float eps, int max_iter,
                                      int norm_p, int cost_pow, void* workspace, const float* map, const float* row_sum,
                                      const float* grad_map, const float* grad_cost, float* grad_x, float* grad_y,
                                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * Chamfer distance (comparison baseline).
 * Replaces: pytorch3d.loss.chamfer_distance with default arguments, as called at
 * train_CD.py:123,161,327-328, main_rotation.py:203, test_ERROR.py:216 (third-party arithmetic,
 * un-vendored and un-pinned: see DESIGN.md "parity unpinned").
 *   x (pairs, n, 3), y (pairs, m, 3)
 *   min_xy (pairs*n) fp32 out : min_j |x_i - y_j|^2 ;  nn_xy (pairs*n) int32 out : its argmin j
 *   min_yx (pairs*m) fp32 out : min_i |x_i - y_j|^2 ;  nn_yx (pairs*m) int32 out : its argmin i
 *   pair_loss (pairs) out : mean_i min_xy[b,i] + mean_j min_yx[b,j]   (deterministic reduction)
 * All five outputs are required (the index arrays feed shw_chamfer_backward).  pairs <= 65535 (gridDim.y).
 */
SHW_API int shw_chamfer_forward(const float* x, const float* y, int pairs, int n, int m,
                        float* min_xy, int32_t* nn_xy, float* min_yx, int32_t* nn_yx,
                        float* pair_loss, void* stream);

/* grad of sum_b w[b]*pair_loss[b] (w = per-pair upstream gradient, device pointer, (pairs)).
 * grad_x, grad_y are overwritten.  Owner-computed (round 3): every row is summed by one thread in a fixed order --
 * bit-identical from run to run (round 2 scattered with float atomics and needed zero-filled outputs). */
SHW_API int shw_chamfer_backward(const float* x, const float* y, const int32_t* nn_xy, const int32_t* nn_yx,
                         const float* w, int pairs, int n, int m,
                         float* grad_x, float* grad_y, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Exact Wasserstein cost between two uniform clouds of EQUAL size (csrc/shw_emd.hip); clouds of different sizes:
 * shw_emd_units_* further down.
 * Replaces: ot.emd2 (POT, a CPU network simplex in a Python loop over the batch) as the reference's live loss calls it:
 * losses/s2_wasserstein.py:13-66 Cos_disimilarity_W (train_W_COS.py:393, train_Pseudo_W_COS.py:391), :73-126
 * Geodesic_distance_W, Flow_cube.ipynb cell 5 wasserstein_distance / wasserstein_distance_geo, the W2 metric of the flow
 * notebooks and main_rotation.py:213-219.  With n = m and uniform weights the problem is a linear assignment problem;
 * it is solved by an eps-scaling forward auction on fixed-point costs, one workgroup per pair.
 *   "Exact" means: the returned permutation sigma has mean_i C(i, sigma(i)) <= optimum + K 2^-25, K the power of two
 *   the kernel finds above the largest cost of the pair -- below the float32 resolution of the costs themselves.
 *   POT is third-party and not installed: parity with ot.emd2 itself is unpinned; the tests compare with scipy's
 *   linear_sum_assignment.
 *   kind 0: C = sum_d |x_d - y_d|^p (cos_cost_matrix, :52-63);  kind 1: C = angle(x, y)^p (geodesic_cost_matrix,
 *   :112-123) with the angle from atan2(|x cross y|, x . y) and pi / 2 for a zero-length point.  p >= 1, any float.
 */

/* Largest n of the entries below (2048). */
SHW_API int shw_max_points_emd(void);

/* Bytes of the workspace the forward writes and the backward reads: the assignment, its inverse, one flag per pair. */
SHW_API size_t shw_emd_workspace_bytes(int pairs, int n);

/* x, y (pairs, n, 3) fp32;  n == m, 1 <= n <= the limit, pairs <= 65535, pairs == 0 is a no-op.
 *   cost (pairs) fp32 out  : mean_i C(x_i, y_assign[i]), summed in a fixed order
 *   assign (pairs, n) int32 out : the target of each source point
 *   rounds (pairs) int32 out : bidding rounds used.  Every loop is bounded: a pair that would need more than
 *     1024 n + 4096 rounds (8 x the worst ratio the CPU restatement records) gets cost NaN, rounds = that cap
 *     and the identity assignment.
 * Deterministic: the same inputs give the same bits. */
SHW_API int shw_emd_forward(const float* x, const float* y, int pairs, int n, int m, int kind, float p, void* workspace,
                            float* cost, int32_t* assign, int32_t* rounds, void* stream);

/* grad of sum_b w[b] cost[b] (w: device pointer, (pairs)); workspace: as the forward left it.  The plan is locally
 * constant: grad_x[i] = (w/n) dC(x_i, y_assign[i])/dx_i and grad_y[j] likewise through the inverse permutation -- what
 * ot.emd2's autograd gives through C.  Owner-computed, no atomics, bit-identical from run to run; outputs overwritten.
 * kind 1: where sin(angle) = 0 or a point has zero length, 0 is written (the reference's acos gives inf / NaN).
 * A pair whose cost is NaN (round cap) gets zero gradients. */
SHW_API int shw_emd_backward(const float* x, const float* y, const void* workspace, const float* w, int pairs, int n,
                             int kind, float p, float* grad_x, float* grad_y, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Exact Wasserstein cost between two uniform clouds of DIFFERENT sizes (csrc/shw_emd_units.hip).
 * Replaces: ot.emd2 where the trainers give the clouds different point counts (train_W_COS.py:292-293, 334-336
 * --source_p_n / --target_p_n; train_RUNNER.py:193-218: 128 source points against 256 and 512 target points).
 * With g = gcd(n, m), ks = m / g, kt = n / g, U = lcm(n, m) = n ks = m kt: every source carries ks units of mass 1 / U,
 * every target has kt slots; supplies and demands are integral in units, so the transport optimum is the optimum of the
 * U x U assignment problem between units and slots, solved by the rule of shw_emd_forward without expanding the clouds
 * (a bidding unit evaluates the cost once per target).  "Exact" as above: mean over units <= optimum + K 2^-25.
 * SIZES.  1 <= n, m <= 2048, U <= 4096 (a bid word names its bidder in 12 bits), and the kernel's LDS footprint
 * 40 U + 12 (n + m) bytes (each count rounded up to 4) at most 162 816 (the CU's 160 KB less 1 KB): every pair with
 * lcm(n, m) <= 2048, n == m included, and above that e.g. (768, 1024) and (1024, 1536), U = 3072.  Everything else is
 * REFUSED: (1000, 1024) has U = 128 000.  Uniform weights only; kind and p as above.
 */

/* U = lcm(n, m) if the pair is served, else 0.  Makes no HIP call. */
SHW_API int shw_emd_units_supported(int n, int m);

/* Bytes of the workspace: the target of each unit, the source of each slot (pairs * U int32 each), one flag per pair.
 * 0 for a pair that is not served. */
SHW_API size_t shw_emd_units_workspace_bytes(int pairs, int n, int m);

/* x (pairs, n, 3), y (pairs, m, 3) fp32; pairs <= 65535, pairs == 0 is a no-op.
 *   cost (pairs) fp32 out        : (1/U) sum_q C(x[q / ks], y[targets[q]]), summed in a fixed order
 *   targets (pairs, U) int32 out : the target POINT (not the slot) of each unit; units i ks .. i ks + ks - 1 belong to
 *                                  source i, and every target is named by exactly kt units
 *   rounds (pairs) int32 out     : bidding rounds used; a pair that would need more than 1024 U + 4096 gets cost NaN,
 *                                  rounds = that cap and unit q on target q / kt.
 * Deterministic: the same inputs give the same bits.  With n == m, targets is shw_emd_forward's assign. */
SHW_API int shw_emd_units_forward(const float* x, const float* y, int pairs, int n, int m, int kind, float p,
                                  void* workspace, float* cost, int32_t* targets, int32_t* rounds, void* stream);

/* grad of sum_b w[b] cost[b]; workspace: as the forward left it.  grad_x[i] = (w/U) sum over the ks units of x_i of
 * dC(x_i, y_t)/dx_i in unit order, grad_y[j] the same over its kt slots in slot order.  Owner-computed, no atomics,
 * bit-identical from run to run; outputs overwritten; zero conventions as shw_emd_backward. */
SHW_API int shw_emd_units_backward(const float* x, const float* y, const void* workspace, const float* w, int pairs, int n,
                                   int m, int kind, float p, float* grad_x, float* grad_y, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The sphere map phi: residual flows on 3-D points (csrc/shw_flow.hip).
 * Replaces: the values and gradients the trainers take from `Norm_Flow_structure(flow_name="Residual")`
 * (s2_wasserstein.py:134-163, train_W_COS.py:40,390): `flows` blocks z <- z + MLP(z), the MLP a chain of `layers` pairs
 * [Swish, Linear] (nets/lipschitz.py:14-67), 3 -> hidden -> ... -> hidden -> 3, the activation BEFORE every linear layer:
 * a(x) = x sigmoid(gamma x) / 1.1.  The log-determinant the reference estimates and throws away is not computed.
 * PARAMETERS are packed and EFFECTIVE: per flow, per layer k, in this order
 *     gamma_k = softplus(beta_k)  (1),   W_eff,k row-major (out_k, in_k),   b_k (out_k)
 * with W_eff = W / max(1, sigma / coeff) formed by the caller, so shw_flow_residual_param_count(hidden, layers) =
 * (1 + 4 hidden) + (layers - 2) (1 + hidden^2 + hidden) + (4 + 3 hidden) floats per flow.
 * ENVELOPE: dim == 3, 1 <= hidden <= 32, 2 <= layers <= 8, 1 <= flows <= 16; anything else is hipErrorInvalidValue.
 * Finite inputs give finite outputs and gradients (sigmoid of a large negative argument is 0, of a large positive one 1).
 */

/* 1 inside the envelope, else 0.  Makes no HIP call. */
SHW_API int shw_flow_residual_supported(int dim, int hidden, int layers, int flows);

/* floats of the packed parameters of ONE flow; 0 outside the envelope */
SHW_API size_t shw_flow_residual_param_count(int hidden, int layers);

/* bytes of the backward's workspace (partial parameter-gradient vectors, one per workgroup); 0 for points <= 0 */
SHW_API size_t shw_flow_residual_workspace_bytes(long points, int hidden, int layers, int flows);

/* x (points, 3) fp32, params (flows * param_count) fp32 -> y (points, 3) fp32.  All flows in one launch; points == 0
 * is a no-op. */
SHW_API int shw_flow_residual_forward(const float* x, const float* params, long points, int hidden, int layers, int flows,
                                      float* y, void* stream);

/* gy (points, 3): gradient w.r.t. y.  gx (points, 3) out, gparams (flows * param_count) out, laid out as params; either
 * may be NULL and is then not computed.  Nothing is saved by the forward: the layer inputs are recomputed from x.
 * workspace: shw_flow_residual_workspace_bytes bytes, needed only with gparams; it need not be cleared.  gparams is
 * summed without atomics in a fixed order: the same inputs give the same bits.  points == 0 zeroes gparams. */
SHW_API int shw_flow_residual_backward(const float* x, const float* params, const float* gy, long points, int hidden,
                                       int layers, int flows, float* gx, float* gparams, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The registration network's trunk: PointNet point MLP fused with the max-pool (csrc/shw_pointnet.hip).
 * Replaces: `Pooling()(MLP_Architecture(emb)(x))` of models/pcrnet.py:29,49 -- five 1x1 convolutions 3 -> 64 -> 64 -> 64
 * -> 128 -> emb, a ReLU after each, and the maximum over the points.  max_i relu(z_i) = relu(max_i z_i), so the last
 * layer's (clouds, emb, points) output is never stored: the forward keeps a running maximum and its arg-max, and the
 * backward recomputes the hidden layers on the arg-max points only, one row per (cloud, channel).
 * PARAMETERS are packed: W1 (64, 3) b1 (64) W2 (64, 64) b2 W3 (64, 64) b3 W4 (128, 64) b4 W5 (emb, 128) b5 (emb), each
 * weight row-major (out, in) = Conv1d's (out, in, 1); 16-byte aligned.
 * ENVELOPE: dim == 3, emb % 32 == 0, 32 <= emb <= 2048, clouds >= 1, 1 <= points < 2^31; anything else is
 * hipErrorInvalidValue.  Layers 2..5 run on the exact-f32 matrix instruction: every dot product is an f32 fmaf chain.
 * Neither entry allocates, synchronises or reads back; both can be captured into a graph.
 */

/* 1 inside the envelope, else 0.  Makes no HIP call. */
SHW_API int shw_pointnet_supported(int dim, int emb);

/* floats of the packed parameters, 16 896 + 129 emb; 0 outside the envelope */
SHW_API size_t shw_pointnet_param_count(int emb);

/* bytes of the workspace of the forward (backward == 0: per-tile maxima, clouds * ceil(points / 64) * emb pairs) or of the
 * backward (per-row point gradients and per-workgroup partial parameter gradients); 0 outside the envelope */
SHW_API size_t shw_pointnet_workspace_bytes(long clouds, long points, int emb, int backward);

/* x (clouds, points, 3) fp32 -> feat (clouds, emb) = relu(max over the points of the last pre-activation) and argmax
 * (clouds, emb) int32, the point index of that maximum.  Ties go to the lowest index; argmax is in [0, points) whatever
 * the input holds, also for channels whose feature is 0.  workspace need not be cleared. */
SHW_API int shw_pointnet_forward(const float* x, const float* params, long clouds, long points, int emb, float* feat,
                                 int* argmax, void* workspace, void* stream);

/* gfeat (clouds, emb): gradient w.r.t. feat; feat and argmax as the forward returned them.  gx (clouds, points, 3) out:
 * zero except at arg-max points, the channels of one point added in ascending channel order.  gparams out, laid out as
 * params.  Either may be NULL and is then not computed.  A channel with feat == 0 passes nothing.  Sums run in a fixed
 * order without atomics: the same inputs give the same bits.  workspace (16-byte aligned) need not be cleared. */
SHW_API int shw_pointnet_backward(const float* x, const float* params, const float* feat, const int* argmax,
                                  const float* gfeat, long clouds, long points, int emb, float* gx, float* gparams,
                                  void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The sphere encoder of the phi-max wrappers (csrc/shw_sphere_map.hip).
 * Replaces: the values and gradients of `transform_to_sphere` (max_spherical_sliced_w.py:334-350) and of
 * `transform_to_sphere_fast` (max_spherical_sliced_w_fast.py:323-338), the phi both files' `__main__` hand to
 * `max_spherical_wassersten_distance[_fast]` (:555-561, _fast.py:411-417).  Per point x in R^3:
 *     z1 = tanh(W1 x + b1),  z2 = tanh(W2 z1 + b2),  o = W3 z2 + b3,
 *     theta1 = pi (tanh(o0) / 2 + 1/2),  theta2 = pi tanh(o1),
 *     y = (sin theta1 cos theta2, sin theta1 sin theta2, cos theta1).
 * PARAMETERS are one flat fp32 buffer in state-dict order: W1 row-major (16, 3), b1 (16), W2 (4, 16), b2 (4), W3 (2, 4),
 * b3 (2) -- 142 floats.
 * ENVELOPE: dim == 3, hidden1 == 16, hidden2 == 4.  Finite inputs give finite outputs and gradients: a saturated tanh
 * is exactly +-1 with a slope of exactly 0.  No entry allocates, synchronises or reads back; all can be captured into a
 * graph.
 */

/* 1 for (3, 16, 4), else 0.  Makes no HIP call.  (Replaces the widths written into :338-341, _fast.py:327-329.) */
SHW_API int shw_sphere_map_supported(int dim, int hidden1, int hidden2);

/* floats of the parameter buffer, 142; 0 outside the envelope.  (The six tensors of `self.net`, :338-342.) */
SHW_API size_t shw_sphere_map_param_count(int hidden1, int hidden2);

/* workgroups (one wave each) the backward launches for `points` points: min(ceil(points / 64), 1024), 0 for points <= 0.
 * Workgroup b takes the 64-point tiles b, b + blocks, ... in order.  (No counterpart in the reference: autograd of
 * :345-348 sums in library order.) */
SHW_API int shw_sphere_map_backward_blocks(long points);

/* bytes of the backward's workspace, one 142-float partial vector per workgroup; 0 for points <= 0 */
SHW_API size_t shw_sphere_map_workspace_bytes(long points);

/* x (points, 3) fp32, params (142) fp32 -> y (points, 3) fp32, unit vectors.  points == 0 is a no-op.
 * (Replaces `forward`, :344-350 and _fast.py:332-338.) */
SHW_API int shw_sphere_map_forward(const float* x, const float* params, long points, float* y, void* stream);

/* gy (points, 3): gradient w.r.t. y.  gx (points, 3) out, gparams (142) out, laid out as params; either may be NULL and
 * is then not computed.  Nothing is saved by the forward: the activations are recomputed from x.  workspace:
 * shw_sphere_map_workspace_bytes bytes, needed only with gparams; it need not be cleared.  gparams is summed without
 * atomics in a fixed order: the same inputs give the same bits.  points == 0 zeroes gparams.
 * (Replaces autograd's backward through :345-348, reached from `loss.backward(retain_graph=True)`, :523 and _fast.py:369.) */
SHW_API int shw_sphere_map_backward(const float* x, const float* params, const float* gy, long points, float* gx,
                                    float* gparams, float* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The registration network after its trunk: the pose head and the rigid pose update (csrc/shw_pose.hip).
 * Replaces, per refinement iteration of `PCRNet.Pose_estimation` (models/pcrnet.py): `self.linear(torch.cat([template
 * features, source features], 1))` -- six Linear layers 2 emb -> w1 -> w2 -> w3 -> w4 -> w5 -> 7 with a ReLU after the
 * first five -- and what follows it: `create_pose_7d`, the transposed rotated identity, the two `bmm`s that update est_R
 * and est_t, and `quaternion_transform` of the source (data_utils/Data_set_transformation.py).
 * HEAD PARAMETERS are one flat fp32 buffer: W1 row-major (w1, 2 emb), b1 (w1), W2 (w2, w1), b2, ..., W6 (7, w5), b6 (7).
 * HEAD ENVELOPE: emb and w1..w5 multiples of 32 in [32, 2048], the output 7 wide, clouds >= 1 (batch tiles of 32 inside
 * the kernels); no dropout.  Exact f32 on v_mfma_f32_32x32x2_f32, every sum in a fixed order, no atomics: the same
 * inputs give the same bits.
 * POSE UPDATE LIMITS: 1 <= clouds <= 65535 (the cloud is gridDim.y), 1 <= points < 2^31.
 * Anything else is hipErrorInvalidValue, returned before any HIP call.  No entry allocates, synchronises or reads back;
 * all can be captured into a graph.
 */

/* 1 inside the head's envelope, else 0.  Makes no HIP call. */
SHW_API int shw_pose_head_supported(int emb, int w1, int w2, int w3, int w4, int w5);

/* floats of the head's parameter buffer; 0 outside the envelope */
SHW_API size_t shw_pose_head_param_count(int emb, int w1, int w2, int w3, int w4, int w5);

/* bytes of a head buffer.  which == 0: the forward's workspace (two buffers of partial sums); 1: the backward's; 2: the
 * saved activations, the five hidden layers after their ReLU stored [feature][clouds rounded up to 32].  0 outside the
 * envelope, for clouds < 1 and for another `which`. */
SHW_API size_t shw_pose_head_workspace_bytes(long clouds, int emb, int w1, int w2, int w3, int w4, int w5, int which);

/* tf, sf (clouds, emb) fp32, params -> out (clouds, 7) fp32 and `saved` (which == 2 bytes) for the backward.  One launch
 * per layer and one that adds the last layer's partial sums.  workspace (which == 0 bytes) need not be cleared. */
SHW_API int shw_pose_head_forward(const float* tf, const float* sf, const float* params, long clouds, int emb, int w1,
                                  int w2, int w3, int w4, int w5, float* out, float* saved, void* workspace, void* stream);

/* gout (clouds, 7): gradient w.r.t. out; saved as the forward wrote it.  gtf, gsf (clouds, emb) out, gparams out, laid
 * out as params; each may be NULL and is then not computed.  One launch per layer (input gradient and weight gradient
 * are workgroup ranges of one grid) and one that adds the first layer's partial sums into gtf / gsf.  workspace
 * (which == 1 bytes) need not be cleared.
 * (Replaces autograd's backward through `self.linear` and the `cat`.) */
SHW_API int shw_pose_head_backward(const float* tf, const float* sf, const float* params, const float* saved,
                                   const float* gout, long clouds, int emb, int w1, int w2, int w3, int w4, int w5,
                                   float* gtf, float* gsf, float* gparams, void* workspace, void* stream);

/* workgroups per cloud of the pose update's backward: min(ceil(points / 256), 64), 0 for points <= 0.  Workgroup x
 * takes the 256-point tiles x, x + blocks, ... in order.  (No counterpart in the reference.) */
SHW_API int shw_pose_update_backward_blocks(long points);

/* bytes of the pose update's backward workspace: twelve partial sums per workgroup; 0 for clouds < 1 or points < 1 */
SHW_API size_t shw_pose_update_workspace_bytes(long clouds, long points);

/* vector (clouds, 7), est_R (clouds, 3, 3), est_t (clouds, 1, 3), source (clouds, points, 3), all fp32 ->
 *     q = vector[0:4] / max(|vector[0:4]|, 1e-12),  t = vector[4:7],  rot(x) = x + 2 (q0 u x x + u x (u x x)),  u = q[1:4],
 *     est_R_out = R est_R,  est_t_out = est_t R^T + t,  source_out[n] = rot(source[n]) + t,   R's columns rot(e_j).
 * One launch.  The zero quaternion gives R = I. */
SHW_API int shw_pose_update_forward(const float* vector, const float* est_R, const float* est_t, const float* source,
                                    long clouds, long points, float* est_R_out, float* est_t_out, float* source_out,
                                    void* stream);

/* g_est_R_out, g_est_t_out, g_source_out: the cotangents of the three outputs, each may be NULL (absent).  g_vector
 * (clouds, 7), g_est_R, g_est_t, g_source out; each may be NULL and is then not computed.  One launch over the points
 * (g_source = R^T g and the per-workgroup sums of g and g x^T) and one lane per cloud that adds the sums in workgroup order
 * and carries them through the rotation, the quaternion and its normalisation (F.normalize's rule: above the clamp
 * (g - q (q . g)) / |v|, at or below it g / 1e-12).  workspace: shw_pose_update_workspace_bytes bytes, needed with
 * g_vector and g_source_out; it need not be cleared.  No atomics: the same inputs give the same bits. */
SHW_API int shw_pose_update_backward(const float* vector, const float* est_R, const float* est_t, const float* source,
                                     const float* g_est_R_out, const float* g_est_t_out, const float* g_source_out,
                                     long clouds, long points, float* g_vector, float* g_est_R, float* g_est_t,
                                     float* g_source, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The sphere encoder of the minibatch Residual-MSSW loss with its blocks applied forward (csrc/shw_mssw.hip).
 * Replaces: the values and gradients of `transform_to_sphere(flow_name="Residual", n_flow_layer)` of
 * mini_batch_Residual_MSSW.py:392-406 after its data-dependent initialisation -- the pointwise encoder
 * `MLP_Architecture` (:327-355), the flows of `Flow_structure` (:359-390) and the angle map (:402-404) -- with every
 * `Residual` built with reverse=False.  (The file itself leaves the class's default reverse=True, which applies each
 * block as its inverse by a fixed-point loop that stops on a test over the whole batch: no per-point kernel; mssw.py runs
 * it composed.)  Per point (b, n) of a (B, N, 3) cloud:
 *     h1 = relu(W1 x + b1) (8),  h2 = relu(W2 h1 + b2) (8),  z = W3 h2 + b3 (2),
 *     per flow f:  z <- z + W_eff,1 a(W_eff,0 a(z) + c0) + c1,   z <- z * exp(s[f, n]) + t[f, n],
 *     theta1 = pi (tanh(z0) / 2 + 1/2),  theta2 = pi tanh(z1),
 *     y = (sin theta1 cos theta2, sin theta1 sin theta2, cos theta1),
 * a(x) = x sigmoid(gamma x) / 1.1.  The scale and shift are per POINT INDEX n and coordinate: the reference's ActNorm(2)
 * takes its statistics over the batch axis only.
 * PARAMETERS are one flat fp32 buffer: W1 row-major (8, 3), b1 (8), W2 (8, 8), b2 (8), W3 (2, 8), b3 (2) -- 122 floats, the
 * encoder in state-dict order -- then per flow gamma0 = softplus(beta0), W_eff,0 (4, 2), c0 (4), gamma1, W_eff,1 (2, 4),
 * c1 (2) -- 24 floats, W_eff = W / max(1, sigma / 0.9) formed by the caller.  AFFINE is (flows, N, 4) fp32, 16-byte
 * aligned: (s0, s1, t0, t1) per flow and point index.
 * ENVELOPE: points of dimension 3, hidden == 4, layers == 2, 1 <= flows <= 8.  The ReLU slope is pre > 0.  Anything else
 * is hipErrorInvalidValue, returned before any HIP call.  No entry allocates, synchronises or reads back; all can be
 * captured into a graph.
 */

/* 1 for hidden == 4, layers == 2, 1 <= flows <= 8, else 0.  Makes no HIP call.  (Replaces the widths written into
 * :373-374.) */
SHW_API int shw_mssw_supported(int hidden, int layers, int flows);

/* floats of the parameter buffer, 122 + 24 flows; 0 outside the envelope */
SHW_API size_t shw_mssw_param_count(int flows);

/* workgroups (one wave each) the backward launches for `points` = B N points: min(ceil(points / 64), 1024), 0 for
 * points <= 0.  Workgroup b takes the 64-point tiles b, b + blocks, ... in order.  (No counterpart in the reference.) */
SHW_API int shw_mssw_backward_blocks(long points);

/* bytes of the backward's workspace: B N flows 16-byte groups (every point's own scale and shift gradients) and one
 * (122 + 24 flows)-float partial vector per workgroup; 0 for B N <= 0 and outside the envelope */
SHW_API size_t shw_mssw_workspace_bytes(long B, long N, int flows);

/* x (B, N, 3) fp32, params, affine -> y (B, N, 3) fp32, unit vectors.  One launch.  B N == 0 is a no-op.
 * (Replaces `forward`, :398-406.) */
SHW_API int shw_mssw_forward(const float* x, const float* params, const float* affine, long B, long N, int flows, float* y,
                             void* stream);

/* gy (B, N, 3): gradient w.r.t. y.  gx (B, N, 3) out, gparams (122 + 24 flows) out, gaffine (flows, N, 4) out (16-byte
 * aligned), laid out as the inputs; each may be NULL and is then not computed.  Nothing is saved by the forward: all is
 * recomputed from x.  gaffine[f, n] sums over the batch axis only, in ascending b; gparams sums over all points, in a
 * fixed order; no atomics: the same inputs give the same bits.  workspace: shw_mssw_workspace_bytes bytes, 16-byte
 * aligned, needed with gparams or gaffine; it need not be cleared.  B N == 0 zeroes gparams and gaffine.
 * (Replaces autograd's backward through :399-404, reached from `loss.backward(retain_graph=True)`, :440.) */
SHW_API int shw_mssw_backward(const float* x, const float* params, const float* affine, const float* gy, long B, long N,
                              int flows, float* gx, float* gparams, float* gaffine, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SHW_H */
