"""What a refinement iteration of `PCRNet` does after the trunk, on the HIP path (csrc/shw_pose.hip, include/shw.h
shw_pose_*).

    pose_head(template_features, source_features, params, widths)            the fused op: (B, emb), (B, emb) -> (B, 7)
    pose_head_composed(template_features, source_features, params, widths)   the same math in torch operations
    pose_update(vector, est_R, est_t, source)             the fused op: -> (est_R', est_t', source')
    pose_update_composed(vector, est_R, est_t, source)    the lines of `PCRNet.Pose_estimation`, operation for operation

The head is six linear layers 2 emb -> w1 -> ... -> w5 -> 7 on the concatenation of the two feature tensors, a ReLU after
the first five.  PACKED PARAMETERS: W1 (w1, 2 emb) row-major, b1, ..., W6 (7, w5), b6 in one flat buffer
(`PCRNet.packed_head_params()` is one `torch.cat`, so the buffer's gradient reaches `linear.*` by autograd).

The pose update: q = vector[:, 0:4] / max(|vector[:, 0:4]|, 1e-12), t = vector[:, 4:7], rot(x) = x + 2 (w u x x + u x (u x x)),
R the matrix whose columns are rot(e_j); est_R' = R est_R, est_t' = est_t R^T + t, source'_n = rot(source_n) + t.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib
from .pcrnet import create_pose_7d, get_translation, quaternion_rotate, quaternion_transform
from .ssw import _stream_ptr

HEAD_WIDTHS = (1024, 1024, 512, 512, 256)
HEAD_OUT = 7
MIN_WIDTH, MAX_WIDTH, WIDTH_STEP = 32, 2048, 32                   # include/shw.h shw_pose_head_supported
MAX_CLOUDS = 65535                                                # the pose update's clouds ride on gridDim.y
_ENVELOPE = (f"the fused head takes an embedding width and five hidden widths that are multiples of {WIDTH_STEP} in "
             f"[{MIN_WIDTH}, {MAX_WIDTH}]")


def pose_head_supported(emb, widths=HEAD_WIDTHS):
    widths = tuple(widths)
    return len(widths) == 5 and all(isinstance(w, int) and MIN_WIDTH <= w <= MAX_WIDTH and w % WIDTH_STEP == 0
                                    for w in (emb,) + widths)


def _head_layer_shapes(emb, widths=HEAD_WIDTHS):
    sizes = (2 * emb,) + tuple(widths) + (HEAD_OUT,)
    return [(sizes[k + 1], sizes[k]) for k in range(len(sizes) - 1)]


def pose_head_param_count(emb, widths=HEAD_WIDTHS):
    """floats of the packed parameters of a head on features of width `emb`"""
    return sum(o * i + o for o, i in _head_layer_shapes(emb, widths))


def unpack_pose_head_params(params, emb, widths=HEAD_WIDTHS):
    """the packed buffer as six (weight (out, in), bias (out,)) views"""
    count = pose_head_param_count(emb, widths)
    if params.dim() != 1 or params.numel() != count:
        raise ValueError(f"params must have shape ({count},), got {tuple(params.shape)}")
    layers, off = [], 0
    for out, inp in _head_layer_shapes(emb, widths):
        layers.append((params[off:off + out * inp].view(out, inp), params[off + out * inp:off + out * inp + out]))
        off += out * inp + out
    return layers


def pose_head_composed(template_features, source_features, params, widths=HEAD_WIDTHS):
    """(B, emb), (B, emb), packed parameters -> (B, 7) in torch operations, on any device and dtype: what
    `PCRNet.linear(torch.cat([template_features, source_features], dim=1))` computes without dropout"""
    h = torch.cat([template_features, source_features], dim=1)
    layers = unpack_pose_head_params(params, template_features.shape[1], widths)
    for weight, bias in layers[:-1]:
        h = F.relu(F.linear(h, weight, bias))
    return F.linear(h, layers[-1][0], layers[-1][1])


def pose_update_composed(vector, est_R, est_t, source):
    """(B, 7), (B, 3, 3), (B, 1, 3), (B, N, 3) -> (est_R', est_t', source'): the lines `PCRNet.Pose_estimation` runs after
    its head, in the same torch operations, on any device and dtype"""
    batch_size = source.size(0)
    pose_7d = create_pose_7d(vector)
    identity = torch.eye(3).to(source).view(1, 3, 3).expand(batch_size, 3, 3).contiguous()
    est_R_temp = quaternion_rotate(identity, pose_7d).permute(0, 2, 1)
    est_t_temp = get_translation(pose_7d).view(-1, 1, 3)
    est_t = torch.bmm(est_R_temp, est_t.permute(0, 2, 1)).permute(0, 2, 1) + est_t_temp
    est_R = torch.bmm(est_R_temp, est_R)
    source = quaternion_transform(source, pose_7d)
    return est_R, est_t, source


def _check_f32(named):
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")


def _check_device(named):
    for name, t in named:
        if not t.is_cuda:
            raise RuntimeError(f"{name} is on {t.device}: the MI355X HIP path needs device tensors "
                               "(the *_composed functions run anywhere)")
    if len({t.device for _, t in named}) != 1:
        raise ValueError("all tensors must be on one device")


def _ptr(t):
    return None if t is None else t.data_ptr()


class _PoseHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tf, sf, params, emb, widths):
        lib = _lib.load()
        dev = tf.device
        clouds = tf.shape[0]
        out = torch.empty(clouds, HEAD_OUT, dtype=torch.float32, device=dev)
        saved = torch.empty(lib.shw_pose_head_workspace_bytes(clouds, emb, *widths, 2) // 4, dtype=torch.float32, device=dev)
        work = torch.empty(lib.shw_pose_head_workspace_bytes(clouds, emb, *widths, 0) // 4, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.shw_pose_head_forward(tf.data_ptr(), sf.data_ptr(), params.data_ptr(), clouds, emb, *widths,
                                                 out.data_ptr(), saved.data_ptr(), work.data_ptr(), _stream_ptr(dev)),
                       "shw_pose_head_forward")
        ctx.save_for_backward(tf, sf, params, saved)
        ctx.emb, ctx.widths = emb, widths
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        tf, sf, params, saved = ctx.saved_tensors
        emb, widths = ctx.emb, ctx.widths
        dev = tf.device
        clouds = tf.shape[0]
        want_t, want_s, want_p = ctx.needs_input_grad[:3]
        if not (want_t or want_s or want_p):
            return None, None, None, None, None
        gout = gout.to(torch.float32).contiguous()
        gtf = torch.empty_like(tf) if want_t else None
        gsf = torch.empty_like(sf) if want_s else None
        gp = torch.empty_like(params) if want_p else None
        work = torch.empty(lib.shw_pose_head_workspace_bytes(clouds, emb, *widths, 1) // 4, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.shw_pose_head_backward(tf.data_ptr(), sf.data_ptr(), params.data_ptr(), saved.data_ptr(),
                                                  gout.data_ptr(), clouds, emb, *widths, _ptr(gtf), _ptr(gsf), _ptr(gp),
                                                  work.data_ptr(), _stream_ptr(dev)),
                       "shw_pose_head_backward")
        return gtf, gsf, gp, None, None


def pose_head(template_features, source_features, params, widths=HEAD_WIDTHS):
    """(B, emb), (B, emb) float32 device features and the packed parameters (pose_head_param_count(emb, widths),) ->
    (B, 7): the six linear layers with a ReLU after the first five, on the concatenation, which is never formed.  One
    launch per layer and one small reduction forward, the same backward; exact float32, every sum in a fixed order
    without atomics: the same bits on every run.  Differentiable w.r.t. both feature tensors and the packed parameters;
    only the gradients that are needed are computed.  Saved for the backward: the inputs and the five hidden activations.
    All allocation is torch's and nothing synchronises, so the op can be captured in a graph.  Outside the envelope (emb
    and the five widths multiples of 32 in [32, 2048]): ValueError.  Refusals in this order: a wrong dtype (TypeError), a
    shape or width outside the envelope (ValueError), tensors that are not on the device (RuntimeError)."""
    named = (("template_features", template_features), ("source_features", source_features), ("params", params))
    _check_f32(named)
    widths = tuple(int(w) for w in widths)
    tf, sf = template_features, source_features
    if tf.dim() != 2 or tf.shape != sf.shape or tf.shape[0] < 1 or not pose_head_supported(int(tf.shape[1]), widths):
        raise ValueError(f"{_ENVELOPE}, on two feature tensors of one shape (B >= 1, emb); got {tuple(tf.shape)}, "
                         f"{tuple(sf.shape)}, widths={widths}")
    emb = int(tf.shape[1])
    count = pose_head_param_count(emb, widths)
    if params.dim() != 1 or params.numel() != count:
        raise ValueError(f"params must have shape ({count},), got {tuple(params.shape)}")
    _check_device(named)
    return _PoseHead.apply(tf.contiguous(), sf.contiguous(), params.contiguous(), emb, widths)


class _PoseUpdate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vector, est_R, est_t, source):
        lib = _lib.load()
        dev = source.device
        clouds, points = source.shape[0], source.shape[1]
        new_R, new_t, moved = torch.empty_like(est_R), torch.empty_like(est_t), torch.empty_like(source)
        with torch.cuda.device(dev):
            _lib.check(lib.shw_pose_update_forward(vector.data_ptr(), est_R.data_ptr(), est_t.data_ptr(), source.data_ptr(),
                                                   clouds, points, new_R.data_ptr(), new_t.data_ptr(), moved.data_ptr(),
                                                   _stream_ptr(dev)),
                       "shw_pose_update_forward")
        ctx.save_for_backward(vector, est_R, est_t, source)
        ctx.set_materialize_grads(False)                 # an absent cotangent stays None: its terms are skipped
        return new_R, new_t, moved

    @staticmethod
    def backward(ctx, g_R, g_t, g_moved):
        lib = _lib.load()
        vector, est_R, est_t, source = ctx.saved_tensors
        dev = source.device
        clouds, points = source.shape[0], source.shape[1]
        want_v, want_R, want_t, want_s = ctx.needs_input_grad
        if not (want_v or want_R or want_t or want_s):
            return None, None, None, None
        g_R, g_t, g_moved = (None if g is None else g.to(torch.float32).contiguous() for g in (g_R, g_t, g_moved))
        g_vector = torch.empty_like(vector) if want_v else None
        g_est_R = torch.empty_like(est_R) if want_R else None
        g_est_t = torch.empty_like(est_t) if want_t else None
        g_source = torch.empty_like(source) if want_s else None
        work = None
        if want_v and g_moved is not None:
            work = torch.empty(lib.shw_pose_update_workspace_bytes(clouds, points) // 4, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.shw_pose_update_backward(vector.data_ptr(), est_R.data_ptr(), est_t.data_ptr(), source.data_ptr(),
                                                    _ptr(g_R), _ptr(g_t), _ptr(g_moved), clouds, points, _ptr(g_vector),
                                                    _ptr(g_est_R), _ptr(g_est_t), _ptr(g_source), _ptr(work),
                                                    _stream_ptr(dev)),
                       "shw_pose_update_backward")
        return g_vector, g_est_R, g_est_t, g_source


def pose_update(vector, est_R, est_t, source):
    """(B, 7), (B, 3, 3), (B, 1, 3), (B, N, 3) float32 device tensors -> (est_R', est_t', source') as in the module
    docstring: what `PCRNet.Pose_estimation` computes after its head.  One launch forward; backward one launch over the
    points and one lane per cloud, the sums over the points in a fixed order without atomics: the same bits on every run.
    Differentiable w.r.t. all four inputs; only the gradients that are needed are computed, and a cotangent that is absent
    costs nothing.  All allocation is torch's and nothing synchronises, so the op can be captured in a graph.  B <= 65535."""
    named = (("vector", vector), ("est_R", est_R), ("est_t", est_t), ("source", source))
    _check_f32(named)
    if source.dim() != 3 or source.shape[-1] != 3 or source.shape[0] < 1 or source.shape[1] < 1:
        raise ValueError(f"source must have shape (B >= 1, N >= 1, 3), got {tuple(source.shape)}")
    B = source.shape[0]
    if B > MAX_CLOUDS:
        raise ValueError(f"at most {MAX_CLOUDS} clouds per call, got {B}")
    if tuple(vector.shape) != (B, 7) or tuple(est_R.shape) != (B, 3, 3) or tuple(est_t.shape) != (B, 1, 3):
        raise ValueError(f"vector, est_R, est_t must have shapes ({B}, 7), ({B}, 3, 3), ({B}, 1, 3); got "
                         f"{tuple(vector.shape)}, {tuple(est_R.shape)}, {tuple(est_t.shape)}")
    _check_device(named)
    return _PoseUpdate.apply(vector.contiguous(), est_R.contiguous(), est_t.contiguous(), source.contiguous())


__all__ = ["pose_head", "pose_head_composed", "pose_head_supported", "pose_head_param_count", "unpack_pose_head_params",
           "pose_update", "pose_update_composed", "HEAD_WIDTHS"]
