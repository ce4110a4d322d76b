"""Host-side mirror of the reference's spherical sliced-Wasserstein call shapes on top
of the HIP C-ABI library.  Same names, argument order and return shapes as
/root/reference/Point_Cloud_Resistration/losses/max_spherical_sliced_w.py (per pair) and
max_spherical_sliced_w_fast.py (batched):

    sliced_wasserstein_sphere(Xs, Xt, num_projections, device, u_weights=None, v_weights=None, p=2)  :289-310
    sliced_wasserstein_sphere_fast(...)                                                      _fast.py:298-319
    sliced_cost(Xs, Xt, Us, p=2, u_weights=None, v_weights=None)                 :251-286 / _fast.py:258-295

PyTorch is plumbing here (device memory, streams, autograd bookkeeping); every number is produced by
the hand-written gfx950 kernels.  CPU tensors are rejected: there is no fallback path.

Precision follows the input, as in the reference (`dtype = u_values.dtype`, :153-160): float32 everywhere, and
float64 for equal cloud sizes with uniform weights (any p >= 1, loss and gradients, sliced and circle level;
kernels of csrc/shw_ssw_f64.hip, up to `max_points_f64()` points per cloud).  Clouds and directions share one dtype.
float64 is OPT-IN: until `enable_float64()` is called (or the process starts with SHW_FLOAT64=1) double tensors raise
TypeError as they always did, so that a caller who passes double by accident is told instead of paying ~9x.
Points of dimension d != 3 (clouds (B,n,d) on S^(d-1), frames (..., d, 2), 2 <= d <= 64 = `shw_max_point_dim()`) are float32: the
kernels of csrc/shw_ssw_dim.hip write the circle coordinates, the circle-level solvers run on those rows, and a D-generic
kernel turns their gradient rows into point gradients (`_PairLossesDim`).  d = 3 keeps its own kernels.
Weighted and unequal-size double clouds are a SECOND opt-in on top of it, `enable_float64_general()` (or
SHW_FLOAT64_GENERAL=1): kernels of csrc/shw_ssw_f64_general.hip, up to `max_points_f64_general()` points per cloud, the
exact minimum over the cut for p != 1 and the level-median formula for p == 1.  While it is off such calls raise the
ValueError they always raised, so that a loader that drops one point does not silently move a caller from the
equal-size kernel to a much slower one.  Weights have the clouds' dtype.
Float32 weights that require grad (under an enabled grad mode) stay in the graph and receive a gradient of their own shape
on every path that takes weights: the sliced functions in R^3 and on S^(d-1), `binary_search_circle`, `emd1D_circle`
(kernels of csrc/shw_ssw_weights.hip).  It is the gradient of the minimum over the cut -- not the
reference's autograd, which stops at its detached cut -- resp. the derivative of the level-median formula; weights count
as normalised and the gradient is centred, sum_i w_i grad_i = 0.  Float64 weights are detached, as before.
"""
from __future__ import annotations

import os
import threading
from collections import OrderedDict

import torch

from . import _lib


_FLOATS = (torch.float32, torch.float64)
_float64_on = os.environ.get("SHW_FLOAT64", "0") == "1"
_float64_general_on = os.environ.get("SHW_FLOAT64_GENERAL", "0") == "1"


def enable_float64(on=True) -> bool:
    """Accept float64 clouds, directions and coordinate rows in the loss functions of this module (equal sizes, uniform
    weights; see the module docstring).  Off by default: double input then raises TypeError, the behaviour before the
    float64 kernels existed.  Process-wide; returns the previous setting so that a caller can restore it."""
    global _float64_on
    previous, _float64_on = _float64_on, bool(on)
    return previous


def float64_enabled() -> bool:
    return _float64_on


def enable_float64_general(on=True) -> bool:
    """Accept float64 clouds of unequal sizes and / or with weights (the general circular-OT kernels in double; see the
    module docstring).  Only effective together with `enable_float64()`.  Off by default: such calls then raise the
    ValueError they raised before these kernels existed.  Process-wide; returns the previous setting."""
    global _float64_general_on
    previous, _float64_general_on = _float64_general_on, bool(on)
    return previous


def float64_general_enabled() -> bool:
    return _float64_general_on


def _check_dtype(name, t):
    if t.dtype == torch.float32 or (t.dtype == torch.float64 and _float64_on):
        return
    if t.dtype == torch.float64:
        raise TypeError(f"{name} must be float32, got torch.float64: the float64 kernels are opt-in, call "
                        "enable_float64() (or set SHW_FLOAT64=1) to use them")
    raise TypeError(f"{name} must be float32 or float64, got {t.dtype}")


def max_points_f64() -> int:
    """Largest point count per cloud of the float64 path (`shw_max_points_f64`)."""
    return int(_lib.load().shw_max_points_f64())


def max_points_f64_general() -> int:
    """Largest point count per cloud of the general float64 path (`shw_max_points_f64_general`)."""
    return int(_lib.load().shw_max_points_f64_general())


def _check_f64_shape(n, m, weighted):
    """Which float64 kernels serve the shape -- True: the general ones (weights and / or n != m, their own opt-in).
    Everything they do not cover says so instead of failing in HIP."""
    if weighted or n != m:
        if not _float64_general_on:
            raise ValueError("float64 input is supported for equal cloud sizes with uniform weights only (got "
                             f"n = {n}, m = {m}{', weights' if weighted else ''}); weighted and unequal-size clouds are "
                             "float32 unless the general float64 kernels are switched on: call enable_float64_general() "
                             "(or set SHW_FLOAT64_GENERAL=1)")
        limit = max_points_f64_general()
        if n > limit or m > limit:
            raise ValueError(f"float64 input with weights or unequal cloud sizes is supported up to {limit} points per "
                             f"cloud, got n = {n}, m = {m}")
        return True
    limit = max_points_f64()
    if n > limit:
        raise ValueError(f"float64 input is supported up to {limit} points per cloud, got {n}")
    return False


def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _check_cloud(name, t):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: the MI355X HIP path needs device tensors (no CPU fallback)")
    _check_dtype(name, t)
    if t.shape[-1] != 3:
        raise ValueError(f"{name} must have 3 coordinates per point, got shape {tuple(t.shape)}")


def _check_point_dim(name, t, d):
    """d != 3 on the spherical path: the D-generic kernels -- 2..shw_max_point_dim() coordinates, float32."""
    most = int(_lib.load().shw_max_point_dim())
    if not 2 <= d <= most:
        raise ValueError(f"{name}: the point dimension must be in 2..{most}, got {d} (shape {tuple(t.shape)})")
    if t.dtype == torch.float64:
        raise ValueError(f"{name}: the D-generic path (point dimension {d} != 3) is float32; float64 input needs "
                         "3 coordinates per point")


def _check_sphere_cloud(name, t):
    """A cloud of the spherical sliced-W functions: `_check_cloud` (R^3; also the check of Chamfer and Sinkhorn, whose
    kernels know 3 coordinates only) or, for another last dimension, the D-generic path's range and dtype."""
    if isinstance(t, torch.Tensor) and t.is_cuda and t.dim() >= 1 and t.shape[-1] != 3:
        _check_point_dim(name, t, t.shape[-1])
        _check_dtype(name, t)
        return
    _check_cloud(name, t)


def draw_directions(num_projections, device, batch=None, d=3, dtype=None):
    """Uniform samples on the Stiefel manifold V_{d,2} from the GLOBAL torch generator, consumed exactly
    like the reference (randn of (L,d,2) resp. (B,L,d,2) on `device`, then reduced QR; :307-308,
    _fast.py:317-318).  `dtype` None: the default dtype, as the reference's `torch.randn`; torch.float64 consumes the
    generator as the reference does when the default dtype is float64."""
    shape = (num_projections, d, 2) if batch is None else (batch, num_projections, d, 2)
    Z = torch.randn(shape, device=device, dtype=dtype)
    return stiefel_frames(Z)


def stiefel_frames(Z):
    """Reduced QR `U, _ = torch.linalg.qr(Z)` of (..., d, 2) Gaussian matrices.  On the device this is the HIP
    kernel `shw_stiefel_frames` (LAPACK's Householder steps and sign convention, one thread per matrix):
    torch.linalg.qr itself takes ~0.94 s for the 32 768 frames of config 3 on MI355X, and differs from the CPU
    LAPACK result by up to 6e-6; the kernel takes microseconds and agrees with LAPACK to fp32 rounding.  CPU
    tensors (tests of the generator stream) go through torch.linalg.qr.  float64 input runs the double form of the
    kernel (`shw_stiefel_frames_f64`) and agrees with LAPACK to double rounding.  d != 3 (2..64, float32) runs the
    D-generic kernel `shw_stiefel_frames_dim`."""
    if not Z.is_cuda:
        return torch.linalg.qr(Z)[0]
    if Z.dtype in _FLOATS and Z.dim() >= 2 and Z.shape[-1] == 2 and Z.shape[-2] != 3:
        d = Z.shape[-2]
        _check_point_dim("Z", Z, d)
        Zc = Z.contiguous()
        U = torch.empty_like(Zc)
        with torch.cuda.device(Z.device):
            _lib.check(_lib.load().shw_stiefel_frames_dim(Zc.data_ptr(), Zc.numel() // (2 * d), d, U.data_ptr(),
                                                          _stream_ptr(Z.device)), "shw_stiefel_frames_dim")
        return U
    if Z.dtype not in _FLOATS or tuple(Z.shape[-2:]) != (3, 2):
        raise TypeError("stiefel_frames expects float32 or float64 (..., 3, 2)")
    lib = _lib.load()
    Zc = Z.contiguous()
    U = torch.empty_like(Zc)
    name = "shw_stiefel_frames" if Z.dtype == torch.float32 else "shw_stiefel_frames_f64"
    with torch.cuda.device(Z.device):
        _lib.check(getattr(lib, name)(Zc.data_ptr(), Zc.numel() // 6, U.data_ptr(), _stream_ptr(Z.device)), name)
    return U


class SSWWorkspace:
    """Persistent device buffers of one problem shape (B, n, m, L): the per-slice costs and shifts / cuts and --
    for training -- the two coefficient scratch rows that the slice kernel writes and the point-gradient kernel
    streams (2 x 268 MB at config 3).  Instances are leased from a small pool keyed by (device, stream,
    shape, dtype) and come back when the evaluation that used them is over: at once for a loss-only call, and when the
    autograd node of a training call dies (after its backward, or when its graph is dropped) -- see `_Lease`.
    A phi-max inner loop (max_iter + 1 evaluations of one shape per step, _fast.py:359-377) thus alternates
    between two sets of buffers instead of asking the allocator for five tensors per evaluation, and nothing is
    zero-filled.  The user-visible results (per-pair losses, total) are NOT pool memory: they are one fresh
    (B+2)-float tensor per call, so holding on to a loss value across later calls is safe.
    Work on the buffers is ordered by the stream they were leased on (the stream is part of the key).  While
    a HIP graph is being captured the pool is bypassed: buffers then belong to the graph's private memory.
    Idle buffers are capped per shape (2) and in total (MAX_IDLE_BYTES, least recently used shapes evicted first); the
    pool is guarded by a lock."""

    _pools: "OrderedDict" = OrderedDict()      # key -> idle workspaces, least recently used key first
    _lock = threading.Lock()                   # autograd may release leases from its own threads
    MAX_IDLE_PER_KEY = 2
    # bounded per key only, every distinct shape pinned up to 1 GB (a training workspace at config 3 is 537 MB)
    # that torch.cuda.empty_cache() cannot reclaim.  Idle buffers of ALL keys together stay below this many bytes: the
    # least recently used shapes go back to torch's caching allocator first.
    MAX_IDLE_BYTES = 4 << 30

    def __init__(self, key):
        dev, _stream, B, n, m, L, dtype, general64, with_coef = key
        self.key = key
        self.pooled = True
        word = 4 if dtype == torch.float32 else 8
        self.slice_cost = torch.empty(B * L, dtype=dtype, device=dev)
        self.slice_aux = torch.empty(B * L, dtype=torch.int32, device=dev)     # shift k* / median level / cut bits
        # general float64 path: the cut theta* / median level is a double, which the int32 words above cannot hold
        self.slice_cut = torch.empty(B * L, dtype=dtype, device=dev) if (dtype == torch.float64 and general64) else None
        self.coef_s = torch.empty(B * L * n, dtype=dtype, device=dev) if with_coef else None
        self.coef_t = torch.empty(B * L * m, dtype=dtype, device=dev) if with_coef else None
        self.nbytes = ((word + 4) * B * L + (word * B * L * (n + m) if with_coef else 0)
                       + (8 * B * L if self.slice_cut is not None else 0))

    @classmethod
    def lease(cls, dev, B, n, m, L, with_coef, dtype=torch.float32, general64=False):
        key = (torch.device(dev), _stream_ptr(dev), B, n, m, L, dtype, bool(general64), bool(with_coef))
        if torch.cuda.is_current_stream_capturing():
            ws = cls(key)
            ws.pooled = False
            return ws
        with cls._lock:
            idle = cls._pools.get(key)
            if idle:
                cls._pools.move_to_end(key)
                return idle.pop()
        return cls(key)

    def release(self):
        if not self.pooled:
            return
        cls = SSWWorkspace
        with cls._lock:
            idle = cls._pools.setdefault(self.key, [])
            cls._pools.move_to_end(self.key)
            if len(idle) < cls.MAX_IDLE_PER_KEY and all(ws is not self for ws in idle):
                idle.append(self)
            total = sum(ws.nbytes for lst in cls._pools.values() for ws in lst)
            while total > cls.MAX_IDLE_BYTES and cls._pools:
                old_key = next(iter(cls._pools))                  # least recently used shape
                lst = cls._pools[old_key]
                if lst:
                    total -= lst.pop().nbytes                     # back to torch's caching allocator
                if not lst:
                    del cls._pools[old_key]

    @classmethod
    def idle_bytes(cls):
        with cls._lock:
            return sum(ws.nbytes for lst in cls._pools.values() for ws in lst)

    @classmethod
    def clear(cls):
        """Drop every idle buffer (hands the memory back to torch's caching allocator)."""
        with cls._lock:
            cls._pools.clear()


class _Lease:
    """Ties a leased workspace to the lifetime of the autograd node that reads it in backward: the node keeps the
    lease, and when the node is freed (CPython reference counting: after backward once the loss tensor is
    re-bound or deleted, or when a graph is dropped without backward) the buffers return to the pool.  A graph kept
    alive with retain_graph=True keeps its buffers -- a second backward through it reads intact coefficients."""

    __slots__ = ("ws",)

    def __init__(self, ws):
        self.ws = ws

    def __del__(self):
        try:
            self.ws.release()
        except Exception:        # interpreter shutdown
            pass


class _PairLosses(torch.autograd.Function):
    """(B,n,3), (B,m,3), dirs -> (B,) per-pair mean over slices of the circular OT cost W_p^p, their sum (1,), and
    on request the (B,L) per-slice costs and shifts."""

    @staticmethod
    def forward(ctx, Xs, Xt, Us, p, shared_dirs, wu, wv, need_grad, want_slices):
        lib = _lib.load()
        B, n, _ = Xs.shape
        m = Xt.shape[1]
        L = Us.shape[-3]
        dev = Xs.device
        Xs_c, Xt_c, Us_c = Xs.contiguous(), Xt.contiguous(), Us.contiguous()
        stride = 0 if shared_dirs else L * 6
        dtype = Xs.dtype
        f64 = dtype == torch.float64
        weighted = wu is not None or wv is not None
        general64 = f64 and (weighted or n != m)                # switched on and within the limit: checked by the caller
        ws = SSWWorkspace.lease(dev, B, n, m, L, need_grad, dtype, general64)
        out = torch.empty(B + 2, dtype=dtype, device=dev)                # [pair_loss (B) | total (2)]
        stream = _stream_ptr(dev)
        general = general64 or weighted or (float(p) != 1.0 and n != m)   # p == 1 with uniform weights: level-median kernel
        cs = ws.coef_s.data_ptr() if need_grad else None
        ct = ws.coef_t.data_ptr() if need_grad else None

        def wargs(w, cnt):
            if w is None:
                return None, 0
            return w.data_ptr(), (0 if w.dim() == 1 else cnt)
        with torch.cuda.device(dev):
            if general64:
                # n != m and / or weights in double: the exact minimum over the cut, or the level median at p == 1
                wu_p, wu_s = wargs(wu, n)
                wv_p, wv_s = wargs(wv, m)
                _lib.check(lib.shw_ssw_forward_general_f64(
                    Xs_c.data_ptr(), Xt_c.data_ptr(), Us_c.data_ptr(), wu_p, wv_p, wu_s, wv_s, B, n, m, L, stride,
                    float(p), ws.slice_cost.data_ptr(), ws.slice_cut.data_ptr(), cs, ct, stream),
                    "shw_ssw_forward_general_f64")
            elif f64:
                # equal sizes, uniform weights (checked by the caller): one entry for loss and training form
                _lib.check(lib.shw_ssw_forward_f64(Xs_c.data_ptr(), Xt_c.data_ptr(), Us_c.data_ptr(), B, n, m, L,
                                                   stride, float(p), ws.slice_cost.data_ptr(),
                                                   ws.slice_aux.data_ptr(), cs, ct, stream), "shw_ssw_forward_f64")
            elif general:
                # n != m and / or weights: the reference's bisection over the cut, followed step for step
                wu_p, wu_s = wargs(wu, n)
                wv_p, wv_s = wargs(wv, m)
                _lib.check(lib.shw_ssw_forward_general(
                    Xs_c.data_ptr(), Xt_c.data_ptr(), Us_c.data_ptr(), wu_p, wv_p, wu_s, wv_s, B, n, m, L, stride,
                    float(p), ws.slice_cost.data_ptr(), ws.slice_aux.data_ptr(), cs, ct, stream),
                    "shw_ssw_forward_general")
            elif need_grad:
                _lib.check(lib.shw_ssw_forward_grad(Xs_c.data_ptr(), Xt_c.data_ptr(), Us_c.data_ptr(), B, n, m, L,
                                                    stride, float(p), ws.slice_cost.data_ptr(),
                                                    ws.slice_aux.data_ptr(), cs, ct, stream),
                           "shw_ssw_forward_grad")
            else:
                _lib.check(lib.shw_ssw_forward(Xs_c.data_ptr(), Xt_c.data_ptr(), Us_c.data_ptr(), B, n, m, L, stride,
                                               float(p), ws.slice_cost.data_ptr(), ws.slice_aux.data_ptr(), stream),
                           "shw_ssw_forward")
            if f64:
                _lib.check(lib.shw_ssw_reduce_f64(ws.slice_cost.data_ptr(), B, L, 1.0 / L, out.data_ptr(),
                                                  out.data_ptr() + 8 * B, stream), "shw_ssw_reduce_f64")
            else:
                _lib.check(lib.shw_ssw_reduce(ws.slice_cost.data_ptr(), B, L, 1.0 / L, out.data_ptr(),
                                              out.data_ptr() + 4 * B, stream), "shw_ssw_reduce")
        cost2d = shift2d = None
        if want_slices:
            cost2d = ws.slice_cost.view(B, L).clone()
            shift2d = torch.zeros(B, L, dtype=torch.int32, device=dev) if general else ws.slice_aux.view(B, L).clone()
            ctx.mark_non_differentiable(cost2d, shift2d)
        need_w = (not f64) and (ctx.needs_input_grad[5] or ctx.needs_input_grad[6])   # (weights in the graph: _check_weights)
        if need_grad or need_w:
            ctx.save_for_backward(Xs_c, Xt_c, Us_c)
            ctx.lease = _Lease(ws)                  # the coefficients (and the cuts) stay put until this node dies
            ctx.dims = (B, n, m, L, stride)
            ctx.weights = (wu, wv, float(p)) if need_w else None
            ctx.set_materialize_grads(False)
        else:
            ws.release()                            # stream-ordered: the next lease is on the same stream
        # (the first pair's loss as a 0-dim OUTPUT: the per-pair call shape returns it, and indexing pair[0] outside would
        #  cost a SelectBackward node -- a zero fill and a copy per step, two of the notebooks' eleven launches)
        return out[:B], out[B:B + 1], cost2d, shift2d, out[0:1].view(())

    @staticmethod
    def backward(ctx, g_pair, g_total, _g_cost, _g_shift, g_first=None):
        lib = _lib.load()
        Xs_c, Xt_c, Us_c = ctx.saved_tensors
        ws = ctx.lease.ws
        B, n, m, L, stride = ctx.dims
        dev = Xs_c.device
        if g_pair is None and g_total is None and g_first is None:
            return (None,) * 9
        gwu = gwv = None
        if ctx.weights is not None and (ctx.needs_input_grad[5] or ctx.needs_input_grad[6]):
            # potential rows of every slice at the cut the solve left in the workspace, then the reduction over slices
            wu, wv, p = ctx.weights
            want_u, want_v = ctx.needs_input_grad[5], ctx.needs_input_grad[6]
            pu = torch.empty(B * L, n, dtype=torch.float32, device=dev) if want_u else None
            pv = torch.empty(B * L, m, dtype=torch.float32, device=dev) if want_v else None
            wud, wvd = (wu.detach() if wu is not None else None), (wv.detach() if wv is not None else None)
            rows_w = _upstream_rows(g_pair, g_total, g_first, B, torch.float32, dev)
            slice_w = (rows_w / L).unsqueeze(1).expand(B, L).contiguous()
            with torch.cuda.device(dev):
                _lib.check(lib.shw_ssw_weight_potentials(
                    Xs_c.data_ptr(), Xt_c.data_ptr(), Us_c.data_ptr(), wud.data_ptr() if wud is not None else None,
                    wvd.data_ptr() if wvd is not None else None, 0 if wud is None or wud.dim() == 1 else n,
                    0 if wvd is None or wvd.dim() == 1 else m, B, n, m, L, stride, p, ws.slice_aux.data_ptr(),
                    pu.data_ptr() if want_u else None, pv.data_ptr() if want_v else None, _stream_ptr(dev)),
                    "shw_ssw_weight_potentials")
            if want_u:
                gwu = _reduce_potentials(pu, slice_w, B, L, n, wu.dim() == 1)
            if want_v:
                gwv = _reduce_potentials(pv, slice_w, B, L, m, wv.dim() == 1)
        want_points = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        want_dirs = ctx.needs_input_grad[2]
        # the upstream gradients go to the kernel as they are: row b is scaled by g_pair[b] + g_total[0] there
        dtype = Xs_c.dtype
        gp = g_pair.to(dtype).contiguous() if g_pair is not None else None
        if g_first is not None:                     # gradient of the 0-dim first-pair output: belongs to row 0
            if gp is None and B == 1:
                gp = g_first.to(dtype).reshape(1)
            else:
                gp = gp.clone() if gp is not None else torch.zeros(B, dtype=dtype, device=dev)
                gp[0] += g_first.to(dtype)
        gt = g_total.to(dtype).contiguous() if g_total is not None else None
        gp_ptr = gp.data_ptr() if gp is not None else None
        gt_ptr = gt.data_ptr() if gt is not None else None
        gxs = gxt = gU = None
        with torch.cuda.device(dev):
            if want_points:
                gxs = torch.empty_like(Xs_c)
                gxt = torch.empty_like(Xt_c)
                name = ("shw_ssw_backward_points" if dtype == torch.float32 else
                        "shw_ssw_backward_points_general_f64" if ws.slice_cut is not None else
                        "shw_ssw_backward_points_f64")
                _lib.check(getattr(lib, name)(Xs_c.data_ptr(), Xt_c.data_ptr(), Us_c.data_ptr(),
                                              ws.coef_s.data_ptr(), ws.coef_t.data_ptr(), B, n, m, L, stride,
                                              1.0 / L, gp_ptr, gt_ptr, gxs.data_ptr(), gxt.data_ptr(),
                                              _stream_ptr(dev)), name)
            if want_dirs:
                # the same coefficient rows folded with d coord / d U: one row per (pair, slice), shared frames sum theirs
                gU = torch.empty(B, L, 3, 2, dtype=dtype, device=dev)
                name = "shw_ssw_backward_dirs" if dtype == torch.float32 else "shw_ssw_backward_dirs_f64"
                _lib.check(getattr(lib, name)(Xs_c.data_ptr(), Xt_c.data_ptr(), Us_c.data_ptr(),
                                              ws.coef_s.data_ptr(), ws.coef_t.data_ptr(), B, n, m, L, stride,
                                              1.0 / L, gp_ptr, gt_ptr, gU.data_ptr(), _stream_ptr(dev)), name)
                if stride == 0:
                    gU = gU.sum(0)
        return gxs, gxt, gU, None, None, gwu, gwv, None, None


class _PairLossesDim(torch.autograd.Function):
    """_PairLosses for points of any dimension 2..64 in float32: (B,n,d), (B,m,d), dirs (L,d,2) / (B,L,d,2) -> the same
    five outputs.  The circle coordinates of both clouds are written out (4 B L (n + m) bytes from the caching allocator,
    given back when forward returns), `shw_circle_ot` solves the B L rows, and backward runs the D-generic point-gradient
    kernel on the coefficient rows kept in the leased workspace."""

    @staticmethod
    def forward(ctx, Xs, Xt, Us, p, shared_dirs, wu, wv, need_grad, want_slices):
        lib = _lib.load()
        B, n, d = Xs.shape
        m = Xt.shape[1]
        L = Us.shape[-3]
        dev = Xs.device
        Xs_c, Xt_c, Us_c = Xs.contiguous(), Xt.contiguous(), Us.contiguous()
        stride = 0 if shared_dirs else L * d * 2
        ws = SSWWorkspace.lease(dev, B, n, m, L, need_grad, torch.float32)
        out = torch.empty(B + 2, dtype=torch.float32, device=dev)        # [pair_loss (B) | total (2)]
        coords = torch.empty(B * L * (n + m), dtype=torch.float32, device=dev)
        stream = _stream_ptr(dev)
        general = wu is not None or wv is not None or (float(p) != 1.0 and n != m)

        def wargs(w, cnt):
            if w is None:
                return None, 0
            return w.data_ptr(), (0 if w.dim() == 1 else cnt)
        wu_p, wu_s = wargs(wu, n)
        wv_p, wv_s = wargs(wv, m)
        with torch.cuda.device(dev):
            _lib.check(lib.shw_ssw_forward_dim(
                Xs_c.data_ptr(), Xt_c.data_ptr(), Us_c.data_ptr(), wu_p, wv_p, wu_s, wv_s, B, n, m, d, L, stride,
                float(p), coords.data_ptr(), ws.slice_cost.data_ptr(), ws.slice_aux.data_ptr(),
                ws.coef_s.data_ptr() if need_grad else None, ws.coef_t.data_ptr() if need_grad else None, stream),
                "shw_ssw_forward_dim")
            _lib.check(lib.shw_ssw_reduce(ws.slice_cost.data_ptr(), B, L, 1.0 / L, out.data_ptr(),
                                          out.data_ptr() + 4 * B, stream), "shw_ssw_reduce")
        cost2d = shift2d = None
        if want_slices:
            cost2d = ws.slice_cost.view(B, L).clone()
            shift2d = torch.zeros(B, L, dtype=torch.int32, device=dev) if general else ws.slice_aux.view(B, L).clone()
            ctx.mark_non_differentiable(cost2d, shift2d)
        need_w = ctx.needs_input_grad[5] or ctx.needs_input_grad[6]
        if need_grad or need_w:
            ctx.save_for_backward(Xs_c, Xt_c, Us_c)
            ctx.lease = _Lease(ws)                  # the coefficients (and the cuts) stay put until this node dies
            ctx.dims = (B, n, m, d, L, stride)
            # weight gradients run the circle-level kernel on the coordinate rows written above: they stay with the node
            ctx.weights = (wu, wv, float(p), coords) if need_w else None
            ctx.set_materialize_grads(False)
        else:
            ws.release()
        return out[:B], out[B:B + 1], cost2d, shift2d, out[0:1].view(())

    @staticmethod
    def backward(ctx, g_pair, g_total, _g_cost, _g_shift, g_first=None):
        lib = _lib.load()
        Xs_c, Xt_c, Us_c = ctx.saved_tensors
        ws = ctx.lease.ws
        B, n, m, d, L, stride = ctx.dims
        dev = Xs_c.device
        if g_pair is None and g_total is None and g_first is None:
            return (None,) * 9
        gwu = gwv = None
        if ctx.weights is not None and (ctx.needs_input_grad[5] or ctx.needs_input_grad[6]):
            wu, wv, p, coords = ctx.weights
            want_u, want_v = ctx.needs_input_grad[5], ctx.needs_input_grad[6]
            pu = torch.empty(B * L, n, dtype=torch.float32, device=dev) if want_u else None
            pv = torch.empty(B * L, m, dtype=torch.float32, device=dev) if want_v else None
            wud, wvd = (wu.detach() if wu is not None else None), (wv.detach() if wv is not None else None)
            rows_w = _upstream_rows(g_pair, g_total, g_first, B, torch.float32, dev)
            slice_w = (rows_w / L).unsqueeze(1).expand(B, L).contiguous()
            per_pair = (wud is not None and wud.dim() == 2) or (wvd is not None and wvd.dim() == 2)
            # (per-pair weights: one launch per pair, as the forward -- a row stride cannot say "one weight row per L rows")
            groups = [(b * L, L, b) for b in range(B)] if per_pair else [(0, B * L, 0)]
            cu, cv = coords.data_ptr(), coords.data_ptr() + 4 * B * L * n
            with torch.cuda.device(dev):
                for r0, cnt, b in groups:
                    _lib.check(lib.shw_circle_weight_potentials(
                        cu + 4 * r0 * n, cv + 4 * r0 * m,
                        None if wud is None else wud.data_ptr() + (4 * b * n if wud.dim() == 2 else 0),
                        None if wvd is None else wvd.data_ptr() + (4 * b * m if wvd.dim() == 2 else 0), 0, 0, cnt, n, m, p,
                        _lib.CIRCLE_AS_SLICED, ws.slice_aux.data_ptr() + 4 * r0,
                        pu.data_ptr() + 4 * r0 * n if want_u else None, pv.data_ptr() + 4 * r0 * m if want_v else None,
                        _stream_ptr(dev)), "shw_circle_weight_potentials")
            if want_u:
                gwu = _reduce_potentials(pu, slice_w, B, L, n, wu.dim() == 1)
            if want_v:
                gwv = _reduce_potentials(pv, slice_w, B, L, m, wv.dim() == 1)
        want_points = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        want_dirs = ctx.needs_input_grad[2]
        gp = g_pair.to(torch.float32).contiguous() if g_pair is not None else None
        if g_first is not None:                     # gradient of the 0-dim first-pair output: belongs to row 0
            if gp is None and B == 1:
                gp = g_first.to(torch.float32).reshape(1)
            else:
                gp = gp.clone() if gp is not None else torch.zeros(B, dtype=torch.float32, device=dev)
                gp[0] += g_first.to(torch.float32)
        gt = g_total.to(torch.float32).contiguous() if g_total is not None else None
        gp_ptr = gp.data_ptr() if gp is not None else None
        gt_ptr = gt.data_ptr() if gt is not None else None
        gxs = gxt = gU = None
        with torch.cuda.device(dev):
            if want_points:
                gxs = torch.empty_like(Xs_c)
                gxt = torch.empty_like(Xt_c)
                _lib.check(lib.shw_ssw_backward_points_dim(
                    Xs_c.data_ptr(), Xt_c.data_ptr(), Us_c.data_ptr(), ws.coef_s.data_ptr(), ws.coef_t.data_ptr(), B, n, m,
                    d, L, stride, 1.0 / L, gp_ptr, gt_ptr, gxs.data_ptr(), gxt.data_ptr(), _stream_ptr(dev)),
                    "shw_ssw_backward_points_dim")
            if want_dirs:
                gU = torch.empty(B, L, d, 2, dtype=torch.float32, device=dev)
                _lib.check(lib.shw_ssw_backward_dirs_dim(
                    Xs_c.data_ptr(), Xt_c.data_ptr(), Us_c.data_ptr(), ws.coef_s.data_ptr(), ws.coef_t.data_ptr(), B, n, m,
                    d, L, stride, 1.0 / L, gp_ptr, gt_ptr, gU.data_ptr(), _stream_ptr(dev)),
                    "shw_ssw_backward_dirs_dim")
                if stride == 0:
                    gU = gU.sum(0)
        return gxs, gxt, gU, None, None, gwu, gwv, None, None


def _check_weights(name, w, count, B, dev, dtype=torch.float32):
    if w is None:
        return None
    if dtype == torch.float64:
        if not isinstance(w, torch.Tensor) or not w.is_cuda or w.dtype != torch.float64:
            raise TypeError(f"{name} must be a float64 device tensor, the dtype of the clouds")
    elif not isinstance(w, torch.Tensor) or not w.is_cuda or w.dtype != torch.float32:
        raise TypeError(f"{name} must be a float32 device tensor")
    if tuple(w.shape) not in ((count,), (B, count)):
        raise ValueError(f"{name} must have shape ({count},) or ({B}, {count}), got {tuple(w.shape)}")
    if dtype == torch.float32 and w.requires_grad and torch.is_grad_enabled():
        return w.contiguous()                   # stays in the graph: the weight-gradient kernels (float32 only)
    return w.detach().contiguous()


def _reduce_potentials(pot, slice_w, pairs, slices, count, shared):
    """grad[b,i] = sum_l slice_w[b,l] pot[b,l,i] (`shw_line_weight_grads`: fixed order, no atomics): (pairs, count), or
    (count,) summed over the pairs as well for a weight row they share."""
    lib = _lib.load()
    dev = pot.device
    if pairs > 65535 or (shared and pairs * slices > 65535 * 64):
        raise ValueError("weight gradients: more than 65535 pairs, or weights shared by more than 65535 * 64 slices: "
                         "split the call")
    grad = torch.empty((count,) if shared else (pairs, count), dtype=torch.float32, device=dev)
    nbytes = lib.shw_line_weight_grads_workspace_bytes(pairs, slices, count, int(shared))
    work = torch.empty(nbytes // 4, dtype=torch.float32, device=dev) if nbytes else None
    with torch.cuda.device(dev):
        _lib.check(lib.shw_line_weight_grads(pot.data_ptr(), slice_w.data_ptr(), pairs, slices, count, int(shared),
                                             work.data_ptr() if work is not None else None, grad.data_ptr(),
                                             _stream_ptr(dev)), "shw_line_weight_grads")
    return grad


def _upstream_rows(g_pair, g_total, g_first, B, dtype, dev):
    """The upstream gradients of the three loss outputs as one (B,) row weight, or None when there is none."""
    gp = g_pair.to(dtype).contiguous() if g_pair is not None else None
    if g_first is not None:                     # gradient of the 0-dim first-pair output: belongs to row 0
        gp = gp.clone() if gp is not None else torch.zeros(B, dtype=dtype, device=dev)
        gp[0] += g_first.to(dtype)
    if g_total is not None:
        gp = gp + g_total.to(dtype).reshape(1) if gp is not None else g_total.to(dtype).reshape(1).expand(B)
    return gp


def ssw_pair_losses(Xs, Xt, Us, p=2, return_slices=False, u_weights=None, v_weights=None, return_total=False,
                    return_first=False):
    """Core op: batched clouds (B,n,3), (B,m,3); directions (B,L,3,2) or shared (L,3,2); optional weights
    (n,) / (B,n) and (m,) / (B,m).  Float32 clouds (B,n,d), (B,m,d) with directions (..., d, 2) of the same d in
    2..64 take the D-generic path (`_PairLossesDim`), with the same outputs and options.
    Returns (B,) per-pair losses = mean over slices of W_p^p on the slice circle
    [optionally also the (B,L) per-slice costs and optimal shifts; or, with return_total, the shape-[1] sum over
    pairs that the reduction kernel produces in the same launch (the batched reference value, _fast.py:291-293)].
    Scratch (per-slice arrays, gradient coefficients) lives in a pooled SSWWorkspace; results are fresh tensors.
    Losses, per-slice costs and gradients have the input's dtype; float64 with n != m or weights needs
    `enable_float64_general()` and, like the float32 general path, returns a zero shift tensor with the slices.
    Differentiable in the two clouds AND in the frames `Us` (every path: R^3 float32, D-generic, both float64 paths):
    `Us.grad` has the shape of `Us`, shared frames receive the sum over the pairs.  The frame gradient is the derivative of
    the loss as a function of an arbitrary (d,2) matrix (no projection on the Stiefel tangent space); since the loss does
    not change when a frame is rotated in its plane or scaled, <g[:,0], u2> = <g[:,1], u1> and <g[:,0], u1> = -<g[:,1], u2>.
    Backward launches the point-gradient kernel only if a cloud requires grad and the frame-gradient kernel
    (csrc/shw_ssw_dirs.hip) only if `Us` does; with frames that do not require grad nothing differs from before, and
    with frames that do, the loss and the point gradients keep their bits.
    Float32 weights that require grad receive `.grad` of their own shape ((n,) shared: summed over the pairs): backward then
    launches the potential kernel (csrc/shw_ssw_weights.hip) for the sides that need it and `shw_line_weight_grads` for the
    reduction over slices; with or without gradients to the clouds and the frames, whose bits, like the loss's, do not
    change.  With no weight requiring grad nothing is launched or allocated that was not before.  Float64 weights are
    detached: not differentiable."""
    _check_sphere_cloud("Xs", Xs)
    _check_sphere_cloud("Xt", Xt)
    _check_cloud_dirs(Us)
    if not (Xs.dtype == Xt.dtype == Us.dtype):
        raise TypeError(f"Xs, Xt and Us must share one dtype, got {Xs.dtype}, {Xt.dtype}, {Us.dtype}")
    d = Xs.shape[-1]
    if Xt.shape[-1] != d or Us.shape[-2] != d:
        raise ValueError(f"point dimension mismatch: Xs has {d} coordinates per point, Xt {Xt.shape[-1]} and the frames "
                         f"Us {Us.shape[-2]} (clouds (B,n,d), (B,m,d) and frames (L,d,2) or (B,L,d,2) share one d)")
    if Xs.dim() != 3 or Xt.dim() != 3 or Xs.shape[0] != Xt.shape[0]:
        raise ValueError(f"Xs and Xt must be (B,n,{d}) and (B,m,{d}) with the same B")
    shared = Us.dim() == 3
    if not shared and Us.shape[0] != Xs.shape[0]:
        raise ValueError(f"per-pair directions must be (B,L,{d},2)")
    if not (float(p) >= 1.0):
        raise ValueError("p must be >= 1")
    if Us.shape[-3] < 1 or Xs.shape[1] < 1 or Xt.shape[1] < 1:
        raise ValueError("need at least one slice and one point per cloud")
    if Xs.dtype == torch.float64:
        _check_f64_shape(Xs.shape[1], Xt.shape[1], u_weights is not None or v_weights is not None)
    wu = _check_weights("u_weights", u_weights, Xs.shape[1], Xs.shape[0], Xs.device, Xs.dtype)
    wv = _check_weights("v_weights", v_weights, Xt.shape[1], Xs.shape[0], Xs.device, Xs.dtype)
    # evaluation under torch.no_grad() on inputs that still carry requires_grad must not run the
    # training kernel / allocate the coefficient scratch
    need_grad = torch.is_grad_enabled() and (Xs.requires_grad or Xt.requires_grad or Us.requires_grad)
    op = _PairLosses if d == 3 else _PairLossesDim
    pair, total, cost, shift, first = op.apply(Xs, Xt, Us, float(p), shared, wu, wv, need_grad, bool(return_slices))
    if return_first:                                # 0-dim loss of the first pair (the per-pair call shape)
        return first
    if return_total:
        return pair, total
    if return_slices:
        return pair, cost, shift
    return pair


def _check_cloud_dirs(Us):
    if not isinstance(Us, torch.Tensor) or not Us.is_cuda:
        raise TypeError("Us must be a float32 or float64 device tensor")
    if Us.dim() in (3, 4) and Us.shape[-1] == 2 and Us.shape[-2] != 3:
        _check_point_dim("Us", Us, Us.shape[-2])
        _check_dtype("Us", Us)
        return
    _check_dtype("Us", Us)
    if Us.dim() not in (3, 4) or tuple(Us.shape[-2:]) != (3, 2):
        raise ValueError(f"Us must be (L,3,2) or (B,L,3,2), got {tuple(Us.shape)}")


def circle_coordinates(X, Us):
    """Circle coordinates of the reference's lines :270-279: X (B,n,d) and frames Us (L,d,2) shared or (B,L,d,2) ->
    (B,L,n) numbers in [0, 1], `coords[b,l,i]` = (atan2(-b, -a) + pi) / (2 pi) with (a, b) = U_l^T x_i.  A cloud (n,d)
    with frames (L,d,2) gives (L,n).  Float32, 2 <= d <= 64 (d = 3 included: the same bits as the R^3 kernels compute
    internally); not differentiable.  What `binary_search_circle` / `emd1D_circle` take as rows."""
    _check_sphere_cloud("X", X)
    _check_cloud_dirs(Us)
    if X.dtype != torch.float32 or Us.dtype != torch.float32:
        raise TypeError(f"circle_coordinates is float32, got {X.dtype} and {Us.dtype}")
    single = X.dim() == 2
    Xb = X.detach().unsqueeze(0) if single else X.detach()
    d = Xb.shape[-1]
    if Xb.dim() != 3 or Us.shape[-2] != d:
        raise ValueError(f"point dimension mismatch or bad shape: X {tuple(X.shape)} must be (B,n,d) or (n,d) and Us "
                         f"{tuple(Us.shape)} (L,d,2) or (B,L,d,2) with the same d")
    B, n, _ = Xb.shape
    shared = Us.dim() == 3
    if not shared and Us.shape[0] != B:
        raise ValueError(f"per-pair directions must be (B,L,{d},2)")
    L = Us.shape[-3]
    if n < 1 or L < 1:
        raise ValueError("need at least one slice and one point")
    Xc, Uc = Xb.contiguous(), Us.detach().contiguous()
    out = torch.empty(B, L, n, dtype=torch.float32, device=X.device)
    with torch.cuda.device(X.device):
        _lib.check(_lib.load().shw_ssw_coords_dim(Xc.data_ptr(), Uc.data_ptr(), B, n, d, L, 0 if shared else L * d * 2,
                                                  out.data_ptr(), _stream_ptr(X.device)), "shw_ssw_coords_dim")
    return out[0] if single else out


def sliced_cost(Xs, Xt, Us, p=2, u_weights=None, v_weights=None):
    """Reference `sliced_cost`.  Per pair -- Xs (n,3), Xt (m,3), Us (L,3,2) -> 0-dim tensor, the mean
    over slices (:286).  Batched -- Xs (B,n,3), Xt (B,m,3), Us (B,L,3,2) -> shape-[1] tensor, the SUM
    over pairs of the per-pair means (_fast.py:291-293).  Batched p == 1, which raises in the
    reference, is evaluated pair-wise here (documented extension).
    The result has the input's dtype.  For the batched total this differs from the reference on double input: it
    accumulates in `torch.zeros((1))` (_fast.py:291), which has the DEFAULT dtype, and so returns float32 for double
    clouds unless the default dtype is float64; here double clouds give a double total."""
    if Xs.dim() == 2:
        return ssw_pair_losses(Xs.unsqueeze(0), Xt.unsqueeze(0), Us, p, u_weights=u_weights, v_weights=v_weights,
                               return_first=True)
    _, total = ssw_pair_losses(Xs, Xt, Us, p, u_weights=u_weights, v_weights=v_weights, return_total=True)
    return total


def sliced_wasserstein_sphere(Xs, Xt, num_projections, device, u_weights=None, v_weights=None, p=2):
    """Reference signature (:289).  Xs (n,3), Xt (m,3) on `device` -> 0-dim tensor."""
    U = draw_directions(num_projections, device, d=Xs.shape[1], dtype=Xs.dtype)
    return sliced_cost(Xs, Xt, U, p=p, u_weights=u_weights, v_weights=v_weights)


def sliced_wasserstein_sphere_fast(Xs, Xt, num_projections, device, u_weights=None, v_weights=None, p=2):
    """Reference batched signature (_fast.py:298).  Xs (B,n,3), Xt (B,m,3) -> shape-[1] tensor."""
    U = draw_directions(num_projections, device, batch=Xs.shape[0], d=Xs.shape[2], dtype=Xs.dtype)
    return sliced_cost(Xs, Xt, U, p=p, u_weights=u_weights, v_weights=v_weights)


def retract_frames(Z):
    """(..., d, 2) matrices -> orthonormal 2-frames by Gram-Schmidt on the columns: q1 = z1 / |z1|,
    q2 = (z2 - <z2, q1> q1) / |.|.  The retraction of `max_sliced_wasserstein_sphere`: <q1, z1> = |z1| and
    <q2, z2> = |z2 - <z2, q1> q1| are never negative, so a column cannot flip its sign as it can in a reduced QR with
    LAPACK's convention (which would leave Adam's moments pointing the wrong way).  Plain torch on a few small matrices."""
    z1, z2 = Z[..., 0], Z[..., 1]
    q1 = z1 / torch.linalg.vector_norm(z1, dim=-1, keepdim=True)
    r = z2 - (z2 * q1).sum(-1, keepdim=True) * q1
    q2 = r / torch.linalg.vector_norm(r, dim=-1, keepdim=True)
    return torch.stack((q1, q2), dim=-1)


def max_sliced_wasserstein_sphere(Xs, Xt, num_projections=1, device=None, p=2, max_iter=10, lr=0.05, u_weights=None,
                                  v_weights=None, return_frames=False):
    """Max-sliced spherical W: the frames are drawn as `sliced_wasserstein_sphere` / `_fast` draw them
    (`draw_directions`, the global torch generator), moved by `max_iter` Adam ASCENT steps (step size `lr`) on the loss
    against the detached clouds -- the frame gradient of `ssw_pair_losses` -- and brought back to the Stiefel manifold
    after every step by `retract_frames`; then the loss at the final frames, differentiable in the clouds (and in float32
    weights that require grad: they are detached during the ascent).
    Xs (n,d), Xt (m,d) -> 0-dim tensor; Xs (B,n,d), Xt (B,m,d) -> shape-[1] tensor (per-pair frames), as `sliced_cost`.
    `device` None: the clouds' device.  With `return_frames` also the final frames, (L,d,2) resp. (B,L,d,2), detached.
    The counterpart of `max_sliced_wasserstein_distance` (Euclidean) and `max_GSWD_*` (generalised) for the sphere."""
    device = Xs.device if device is None else device
    batch = Xs.shape[0] if Xs.dim() == 3 else None
    U = draw_directions(num_projections, device, batch=batch, d=Xs.shape[-1], dtype=Xs.dtype).requires_grad_(True)
    xs_d, xt_d = Xs.detach(), Xt.detach()
    # (the ascent is on the frames alone: weights that require grad take part in the final evaluation only)
    uw_d = u_weights.detach() if isinstance(u_weights, torch.Tensor) else u_weights
    vw_d = v_weights.detach() if isinstance(v_weights, torch.Tensor) else v_weights
    optimizer = torch.optim.Adam([U], lr=lr)
    with torch.enable_grad():
        for _ in range(max_iter):
            value = sliced_cost(xs_d, xt_d, U, p=p, u_weights=uw_d, v_weights=vw_d)
            optimizer.zero_grad()
            (-value.sum()).backward()
            optimizer.step()
            U.data = retract_frames(U.data)
    frames = U.detach()
    value = sliced_cost(Xs, Xt, frames, p=p, u_weights=u_weights, v_weights=v_weights)
    return (value, frames) if return_frames else value


# ------------------------------------------------------------------------------------------------------------------
# circle level: the reference's binary_search_circle / emd1D_circle on rows of circle coordinates
# ------------------------------------------------------------------------------------------------------------------
class _CircleOT(torch.autograd.Function):
    """(rows,n), (rows,m) circle coordinates -> (rows,) W_p^p.  One launch; the gradient rows come out of the same
    kernels as d cost / d coordinate (what the sliced path calls its coefficient rows)."""

    @staticmethod
    def forward(ctx, u, v, p, wu, wv, need_grad, method):
        lib = _lib.load()
        rows, n = u.shape
        m = v.shape[1]
        dev = u.device
        uc, vc = u.contiguous(), v.contiguous()
        cost = torch.empty(rows, dtype=u.dtype, device=dev)
        gu = torch.empty(rows, n, dtype=u.dtype, device=dev) if need_grad else None
        gv = torch.empty(rows, m, dtype=u.dtype, device=dev) if need_grad else None
        def wargs(w, cnt):
            if w is None:
                return None, 0
            return w.data_ptr(), (0 if w.dim() == 1 else cnt)
        wu_p, wu_s = wargs(wu, n)
        wv_p, wv_s = wargs(wv, m)
        if u.dtype == torch.float64 and (n != m or wu is not None or wv is not None):
            # switched on and within the limit (checked by the caller)
            with torch.cuda.device(dev):
                _lib.check(lib.shw_circle_ot_general_f64(
                    uc.data_ptr(), vc.data_ptr(), wu_p, wv_p, wu_s, wv_s, rows, n, m, float(p), int(method),
                    cost.data_ptr(), None, gu.data_ptr() if need_grad else None, gv.data_ptr() if need_grad else None,
                    _stream_ptr(dev)), "shw_circle_ot_general_f64")
            if need_grad:
                ctx.save_for_backward(gu, gv)
            return cost
        if u.dtype == torch.float64:                # equal sizes, no weights
            with torch.cuda.device(dev):
                _lib.check(lib.shw_circle_ot_f64(uc.data_ptr(), vc.data_ptr(), rows, n, m, float(p), int(method),
                                                 cost.data_ptr(), None, gu.data_ptr() if need_grad else None,
                                                 gv.data_ptr() if need_grad else None, _stream_ptr(dev)),
                           "shw_circle_ot_f64")
            if need_grad:
                ctx.save_for_backward(gu, gv)
            return cost
        need_w = ctx.needs_input_grad[3] or ctx.needs_input_grad[4]
        cut = torch.empty(rows, dtype=torch.float32, device=dev) if need_w else None   # the cut the bisection ends on
        with torch.cuda.device(dev):
            _lib.check(lib.shw_circle_ot(uc.data_ptr(), vc.data_ptr(), wu_p, wv_p, wu_s, wv_s, rows, n, m, float(p),
                                         int(method), cost.data_ptr(), cut.data_ptr() if need_w else None,
                                         gu.data_ptr() if need_grad else None, gv.data_ptr() if need_grad else None,
                                         _stream_ptr(dev)), "shw_circle_ot")
        if need_grad:
            ctx.save_for_backward(gu, gv)
        if need_w:
            ctx.weights = (uc, vc, wu, wv, float(p), int(method), cut)
        return cost

    @staticmethod
    def backward(ctx, g):
        gu = gv = gwu = gwv = None
        if ctx.saved_tensors:
            gu, gv = ctx.saved_tensors
            w = g.to(gu.dtype).unsqueeze(1)
            gu, gv = gu * w, gv * w
        weights = getattr(ctx, "weights", None)
        if weights is not None and (ctx.needs_input_grad[3] or ctx.needs_input_grad[4]):
            # potential rows at the cut the forward kept; a weight row shared by the rows: the reduction over the rows
            lib = _lib.load()
            uc, vc, wu, wv, p, method, cut = weights
            rows, n = uc.shape
            m = vc.shape[1]
            dev = uc.device
            want_u, want_v = ctx.needs_input_grad[3], ctx.needs_input_grad[4]
            pu = torch.empty(rows, n, dtype=torch.float32, device=dev) if want_u else None
            pv = torch.empty(rows, m, dtype=torch.float32, device=dev) if want_v else None
            wud, wvd = (wu.detach() if wu is not None else None), (wv.detach() if wv is not None else None)
            with torch.cuda.device(dev):
                _lib.check(lib.shw_circle_weight_potentials(
                    uc.data_ptr(), vc.data_ptr(), wud.data_ptr() if wud is not None else None,
                    wvd.data_ptr() if wvd is not None else None, 0 if wud is None or wud.dim() == 1 else n,
                    0 if wvd is None or wvd.dim() == 1 else m, rows, n, m, p, method, cut.data_ptr(),
                    pu.data_ptr() if want_u else None, pv.data_ptr() if want_v else None, _stream_ptr(dev)),
                    "shw_circle_weight_potentials")
            g32 = g.to(torch.float32).contiguous()
            if want_u:
                gwu = _reduce_potentials(pu, g32, 1, rows, n, True) if wu.dim() == 1 else pu * g32.unsqueeze(1)
            if want_v:
                gwv = _reduce_potentials(pv, g32, 1, rows, m, True) if wv.dim() == 1 else pv * g32.unsqueeze(1)
        return gu, gv, None, gwu, gwv, None, None


def _check_rows(name, t):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name} must be a float32 or float64 device tensor (no CPU fallback)")
    _check_dtype(name, t)
    if t.dim() not in (1, 2):
        raise ValueError(f"{name} must be (n,) or (rows, n) circle coordinates")
    return t.unsqueeze(0) if t.dim() == 1 else t


def _circle_ot(u_values, v_values, u_weights, v_weights, p, method):
    u, v = _check_rows("u_values", u_values), _check_rows("v_values", v_values)
    if u.shape[0] != v.shape[0]:
        raise ValueError("u_values and v_values need the same number of rows")
    if u.dtype != v.dtype:
        raise TypeError(f"u_values and v_values must share one dtype, got {u.dtype} and {v.dtype}")
    if not (float(p) >= 1.0):
        raise ValueError("p must be >= 1")
    if u.dtype == torch.float64:
        if u.shape[1] < 1 or v.shape[1] < 1:
            raise ValueError("need at least one coordinate per row")
        _check_f64_shape(u.shape[1], v.shape[1], u_weights is not None or v_weights is not None)
    wu = _check_weights("u_weights", u_weights, u.shape[1], u.shape[0], u.device, u.dtype)
    wv = _check_weights("v_weights", v_weights, v.shape[1], u.shape[0], u.device, u.dtype)
    need_grad = torch.is_grad_enabled() and (u.requires_grad or v.requires_grad)
    return _CircleOT.apply(u, v, float(p), wu, wv, need_grad, method)


def binary_search_circle(u_values, v_values, u_weights=None, v_weights=None, p=1):
    """Reference `binary_search_circle` (max_spherical_sliced_w.py:117-207): circular OT cost W_p^p between rows of circle
    coordinates in [0, 1], (rows, n) and (rows, m) -> (rows,), by the bisection over the cut for EVERY p >= 1.  p = 1 is
    the reference's default and ends in `Cost`'s p == 1 branch (:107-108): the true circular W_1, up to 2.5 % away from
    what `emd1D_circle` returns (that formula leaves out the wrap segment; `sliced_cost` sends p == 1 there, :281-284).
    Differentiable w.r.t. the coordinates (the cut is detached as at :207).  Double rows with weights or n != m need
    `enable_float64_general()` and return the exact minimum over the cut, which the reference's stopping rule ends up to
    1.6e-11 above (fixture G14)."""
    return _circle_ot(u_values, v_values, u_weights, v_weights, p, _lib.CIRCLE_BISECTION)


def emd1D_circle(u_values, v_values, u_weights=None, v_weights=None, p=1):
    """Reference `emd1D_circle` (:210-247): the level-median formula for p = 1, quirk included.
    The reference function has no branch for p != 1 (it falls off its end and returns None); that is an error here.
    Double rows with weights or n != m need `enable_float64_general()`."""
    if float(p) != 1.0:
        raise ValueError("emd1D_circle is the p = 1 level-median formula (the reference returns None for p != 1); "
                         "use binary_search_circle for p != 1")
    return _circle_ot(u_values, v_values, u_weights, v_weights, 1.0, _lib.CIRCLE_LEVEL_MEDIAN)
