"""The registration network of the trainers: `PCRNet` (models/pcrnet.py) with its PointNet trunk `MLP_Architecture`
(models/mlp_architecture.py), `Pooling` (models/pooling.py) and the pose helpers it takes from `Dataset_Transformation`
(data_utils/Data_set_transformation.py), with the trunk and the max-pool on the HIP path (csrc/shw_pointnet.hip,
include/shw.h shw_pointnet_*).

    pointnet_max_features(x, params, emb)            the fused op: (B, N, 3) -> (B, emb), forward and backward kernels
    pointnet_max_features_composed(x, params, emb)   the same math in torch operations (any device / dtype)
    MLP_Architecture(emb_dims), Pooling(), PCRNet(feature_model, droput)     the reference's modules and state-dict layout
    qrot, create_pose_7d, get_quaternion, get_translation, quaternion_rotate, quaternion_transform, convert2transformation

The trunk is five 1x1 convolutions 3 -> 64 -> 64 -> 64 -> 128 -> emb with a ReLU after each, the pooling a maximum over
the points.  max_i relu(z_i) = relu(max_i z_i): the fused forward never stores the (B, emb, N) output of the last layer,
it returns the maximum and the arg-max point of every channel; the gradient of a max-pool reaches only those points, so
the fused backward recomputes the hidden layers on B * emb rows instead of B * N points.

PACKED PARAMETERS, the kernels' input: W1 (64, 3), b1, W2 (64, 64), b2, W3 (64, 64), b3, W4 (128, 64), b4, W5 (emb, 128),
b5, each weight row-major (out, in) -- a Conv1d weight (out, in, 1) flattened.  `MLP_Architecture.packed_params()` is one
`torch.cat` of the module's parameters, so the gradient of the packed buffer reaches them by autograd.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from .ssw import _stream_ptr

POINT_DIM = 3
HIDDEN = (64, 64, 64, 128)
MIN_EMB, MAX_EMB, EMB_STEP = 32, 2048, 32                         # include/shw.h shw_pointnet_supported
_ENVELOPE = (f"the fused trunk takes points of dimension {POINT_DIM} and an embedding width that is a multiple of "
             f"{EMB_STEP} in [{MIN_EMB}, {MAX_EMB}]")


def pointnet_supported(dim, emb):
    return dim == POINT_DIM and MIN_EMB <= emb <= MAX_EMB and emb % EMB_STEP == 0


def _layer_shapes(emb, dim=POINT_DIM):
    channels = (dim,) + HIDDEN + (emb,)
    return [(channels[k + 1], channels[k]) for k in range(5)]


def pointnet_param_count(emb, dim=POINT_DIM):
    """floats of the packed parameters of a trunk of embedding width `emb`"""
    return sum(o * i + o for o, i in _layer_shapes(emb, dim))


def unpack_pointnet_params(params, emb, dim=POINT_DIM):
    """the packed buffer as five (weight (out, in), bias (out,)) views"""
    if params.dim() != 1 or params.numel() != pointnet_param_count(emb, dim):
        raise ValueError(f"params must have shape ({pointnet_param_count(emb, dim)},), got {tuple(params.shape)}")
    layers, off = [], 0
    for out, inp in _layer_shapes(emb, dim):
        layers.append((params[off:off + out * inp].view(out, inp), params[off + out * inp:off + out * inp + out]))
        off += out * inp + out
    return layers


def pointnet_max_features_composed(x, params, emb):
    """(B, N, D) points, packed parameters -> (B, emb): max over the points of relu of the five-layer point MLP, in torch
    operations on any device and dtype (x and params of one dtype).  The fallback of the module and the reference of the
    tests.  Like the module it follows, it materialises the (B, N, emb) activation."""
    h = x
    for weight, bias in unpack_pointnet_params(params, emb, x.shape[-1]):
        h = F.relu(F.linear(h, weight, bias))
    return h.max(dim=1)[0]


class _PointNetMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, params, emb):
        lib = _lib.load()
        dev = x.device
        clouds, points = x.shape[0], x.shape[1]
        feat = torch.empty(clouds, emb, dtype=torch.float32, device=dev)
        argmax = torch.empty(clouds, emb, dtype=torch.int32, device=dev)
        nbytes = lib.shw_pointnet_workspace_bytes(clouds, points, emb, 0)
        work = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.shw_pointnet_forward(x.data_ptr(), params.data_ptr(), clouds, points, emb, feat.data_ptr(),
                                                argmax.data_ptr(), work.data_ptr(), _stream_ptr(dev)),
                       "shw_pointnet_forward")
        ctx.save_for_backward(x, params, feat, argmax)
        ctx.emb = emb
        ctx.mark_non_differentiable(argmax)
        return feat, argmax

    @staticmethod
    def backward(ctx, gfeat, _gargmax):
        lib = _lib.load()
        x, params, feat, argmax = ctx.saved_tensors
        emb = ctx.emb
        dev = x.device
        clouds, points = x.shape[0], x.shape[1]
        want_x, want_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_x or want_p):
            return None, None, None
        gfeat = gfeat.to(torch.float32).contiguous()
        gx = torch.empty_like(x) if want_x else None
        gp = torch.empty_like(params) if want_p else None
        nbytes = lib.shw_pointnet_workspace_bytes(clouds, points, emb, 1)
        work = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.shw_pointnet_backward(x.data_ptr(), params.data_ptr(), feat.data_ptr(), argmax.data_ptr(),
                                                 gfeat.data_ptr(), clouds, points, emb,
                                                 None if gx is None else gx.data_ptr(),
                                                 None if gp is None else gp.data_ptr(), work.data_ptr(),
                                                 _stream_ptr(dev)),
                       "shw_pointnet_backward")
        return gx, gp, None


def pointnet_max_features(x, params, emb, return_argmax=False):
    """(B, N, 3) float32 device points, packed parameters (pointnet_param_count(emb),) -> (B, emb) features, the maximum
    over the points of the trunk's output; with `return_argmax` also the (B, emb) int32 index of the point that attains
    each maximum (ties: the lowest index).  Two kernels forward, a handful backward; differentiable w.r.t. the points and
    w.r.t. the packed parameters, only the gradients that are needed are computed, and they are summed without atomics:
    the same bits on every run.  Saved for the backward: x, params, the features and the arg-max -- nothing of size
    B * N * emb exists at any time.  All allocation is torch's and nothing synchronises, so the op can be captured in a
    graph.  Outside the envelope (dimension 3, emb a multiple of 32 in [32, 2048]): ValueError."""
    for name, t in (("x", x), ("params", params)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if not t.is_cuda:
            raise RuntimeError(f"{name} is on {t.device}: the MI355X HIP path needs device tensors "
                               "(pointnet_max_features_composed runs anywhere)")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
    emb = int(emb)
    if x.dim() != 3 or x.shape[0] < 1 or x.shape[1] < 1 or not pointnet_supported(x.shape[-1], emb):
        raise ValueError(f"{_ENVELOPE}, on x of shape (B >= 1, N >= 1, 3); got x of shape {tuple(x.shape)}, emb={emb}")
    if params.dim() != 1 or params.numel() != pointnet_param_count(emb):
        raise ValueError(f"params must have shape ({pointnet_param_count(emb)},), got {tuple(params.shape)}")
    if params.device != x.device:
        raise ValueError("x and params must be on one device")
    params = params.contiguous()
    if params.data_ptr() % 16:
        params = params.clone()                       # a view at an odd offset: the kernels load weights 16 bytes at a time
    feat, argmax = _PointNetMax.apply(x.contiguous(), params, emb)
    return (feat, argmax) if return_argmax else feat


# ------------------------------------------------------------------------------------------------ the pose helpers
def qrot(q, v):
    """rotate the vectors v (..., 3) by the unit quaternions q (..., 4), real part first: v + 2 (w u x v + u x (u x v))"""
    assert q.shape[-1] == 4 and v.shape[-1] == 3 and q.shape[:-1] == v.shape[:-1]
    shape = v.shape
    q, v = q.reshape(-1, 4), v.reshape(-1, 3)
    u = q[:, 1:]
    uv = torch.cross(u, v, dim=1)
    uuv = torch.cross(u, uv, dim=1)
    return (v + 2 * (q[:, :1] * uv + uuv)).view(shape)


def create_pose_7d(vector):
    """(B, 7) -> (B, 7): the first four entries normalised to a unit quaternion, the translation kept"""
    return torch.cat([F.normalize(vector[:, 0:4], dim=1), vector[:, 4:]], dim=1).view(-1, 7)


def get_quaternion(pose_7d):
    return pose_7d[:, 0:4]


def get_translation(pose_7d):
    return pose_7d[:, 4:]


def quaternion_rotate(point_cloud, pose_7d):
    """(N, 3) points with one pose (1, 7), or (B, N, 3) points with (B, 7) poses -> the rotated points"""
    if point_cloud.dim() == 2:
        assert pose_7d.shape[0] == 1
        quat = get_quaternion(pose_7d).expand(point_cloud.shape[0], -1)
    elif point_cloud.dim() == 3:
        quat = get_quaternion(pose_7d).unsqueeze(1).expand(-1, point_cloud.shape[1], -1).contiguous()
    else:
        raise ValueError(f"point_cloud must be (N, 3) or (B, N, 3), got {tuple(point_cloud.shape)}")
    return qrot(quat, point_cloud)


def quaternion_transform(point_cloud, pose_7d):
    """R p + t per cloud; the translation is broadcast over axis 1 as the reference does"""
    return quaternion_rotate(point_cloud, pose_7d) + get_translation(pose_7d).view(-1, 1, 3).repeat(
        1, point_cloud.shape[1], 1)


def convert2transformation(rotation_matrix, translation_vector):
    """(B, 3, 3), (B, 1, 3) -> (B, 4, 4) homogeneous matrices"""
    last = torch.tensor([[[0.0, 0.0, 0.0, 1.0]]]).repeat(rotation_matrix.shape[0], 1, 1).to(rotation_matrix)
    top = torch.cat([rotation_matrix, translation_vector[:, 0, :].unsqueeze(-1)], dim=2)
    return torch.cat([top, last], dim=1)


# ------------------------------------------------------------------------------------------------ the modules
class MLP_Architecture(nn.Module):
    """`MLP_Architecture(emb_dims=1024)` of models/mlp_architecture.py: conv1 .. conv5, `Conv1d(in, out, 1)` with the
    default initialisation, so the reference's state dict loads (`conv1.weight` ... `conv5.bias`).  forward(x) maps
    (B, N, 3) to the (B, emb, N) activation, as the reference does.  pooled(x) is `Pooling()(forward(x))` without that
    array: with `fused` set, a float32 device input and an embedding width inside the kernel's envelope it takes
    `pointnet_max_features`, otherwise `pointnet_max_features_composed`, both from `packed_params()`."""

    def __init__(self, emb_dims=1024):
        super().__init__()
        self.emb_dims = emb_dims
        self.fused = True
        self.layers = self.create_structure()

    def create_structure(self):
        self.conv1 = nn.Conv1d(3, 64, 1)
        self.conv2 = nn.Conv1d(64, 64, 1)
        self.conv3 = nn.Conv1d(64, 64, 1)
        self.conv4 = nn.Conv1d(64, 128, 1)
        self.conv5 = nn.Conv1d(128, self.emb_dims, 1)
        self.relu = nn.ReLU()
        convs = [self.conv1, self.conv2, self.conv3, self.conv4, self.conv5]
        return [m for conv in convs for m in (conv, self.relu)]

    def forward(self, input_data):
        output = input_data.permute(0, 2, 1)
        for layer in self.layers:
            output = layer(output)
        return output

    def packed_params(self):
        """the kernels' parameter buffer: W1, b1, ..., W5, b5 in one `torch.cat`, differentiable w.r.t. each"""
        convs = (self.conv1, self.conv2, self.conv3, self.conv4, self.conv5)
        return torch.cat([t.reshape(-1) for conv in convs for t in (conv.weight, conv.bias)])

    def uses_fused(self, x, packed):
        return (self.fused and x.is_cuda and x.dtype == torch.float32 and packed.dtype == torch.float32 and x.dim() == 3
                and x.shape[0] >= 1 and x.shape[1] >= 1 and pointnet_supported(x.shape[-1], self.emb_dims))

    def pooled(self, x, packed=None):
        """(B, N, 3) -> (B, emb) = max over the points of forward(x); `packed` takes a `packed_params()` made earlier"""
        if packed is None:
            packed = self.packed_params()
        if self.uses_fused(x, packed):
            return pointnet_max_features(x, packed, self.emb_dims)
        return pointnet_max_features_composed(x, packed, self.emb_dims)


class Pooling(nn.Module):
    """maximum over the last axis of a (B, C, N) activation (models/pooling.py)"""

    def forward(self, input):
        return torch.max(input, 2)[0].contiguous()


class PCRNet(nn.Module):
    """`PCRNet(feature_model, droput=0.0)` of models/pcrnet.py (the keyword is spelled as there): the trunk's pooled
    features of template and source, concatenated, go through the head 2 emb -> 1024 -> 1024 -> 512 -> 512 -> 256 -> 7; the
    seven numbers are a quaternion and a translation that move the source, `iteration_num` times.  It takes the
    reference's state dict unchanged: `feature_model.*` and `linear.{0,2,4,6,8,10}.*` (with dropout the last layer is
    `linear.11`).  forward returns the reference's dict: est_R (B, 3, 3), est_t (B, 1, 3), est_T (B, 4, 4), r (B, emb) and
    transformed_source (B, N, 3).  Two details of the reference are kept: `r` uses the LAST iteration's source features,
    which are those of the source before its last move, and the rotation of an iteration is the transpose of the rotated
    identity.

    `feature_model=None` builds a fresh `MLP_Architecture()`.  The reference's default argument is ONE instance created
    when the class is defined and shared by every model built without the argument; here each model gets its own.

    The trunk runs through `feature_model.pooled` (fused on the device) with the parameters packed once per forward,
    not once per trunk call; a feature model without `pooled` runs as `Pooling()(feature_model(x))`.

    The head and the pose update are torch unless asked for: `fused_head` and `fused_update` (attributes, and keyword
    arguments after `droput`; both False by default) send them through `pose_head` and `pose_update` (pose.py,
    csrc/shw_pose.hip) when the tensors are float32 on the device and, for the head, `linear` is the dropout-free stack
    Linear, ReLU x 5, Linear -> 7 with widths inside the kernel's envelope; the head's parameters are then packed once
    per forward.  Anywhere else -- the CPU, float64, `droput > 0`, a `linear` edited to other shapes -- a set flag runs
    `linear` itself and `pose_update_composed`, which are today's operations.  With both flags False the lines below are
    the only ones that run."""

    def __init__(self, feature_model=None, droput=0.0, fused_head=False, fused_update=False):
        super().__init__()
        self.fused_head = fused_head
        self.fused_update = fused_update
        self._packed_head = None
        self.feature_model = MLP_Architecture() if feature_model is None else feature_model
        self.pooling = Pooling()
        emb = self.feature_model.emb_dims
        layers = []
        for inp, out in ((emb * 2, 1024), (1024, 1024), (1024, 512), (512, 512), (512, 256)):
            layers += [nn.Linear(inp, out), nn.ReLU()]
        if droput > 0.0:
            layers.append(nn.Dropout(droput))
        layers.append(nn.Linear(256, 7))
        self.linear = nn.Sequential(*layers)

    def features(self, points, packed=None):
        if hasattr(self.feature_model, "pooled"):
            return self.feature_model.pooled(points, packed)
        return self.pooling(self.feature_model(points))

    def head_shape(self):
        """(emb, the five hidden widths) when `linear` is the stack the fused head computes, else None"""
        mods = list(self.linear)
        linears, relus = mods[0::2], mods[1::2]
        if (len(mods) != 11 or not all(isinstance(m, nn.Linear) and m.bias is not None for m in linears)
                or not all(isinstance(m, nn.ReLU) for m in relus)):
            return None
        if (linears[0].in_features % 2 or linears[-1].out_features != 7
                or any(a.out_features != b.in_features for a, b in zip(linears, linears[1:]))):
            return None
        return linears[0].in_features // 2, tuple(m.out_features for m in linears[:-1])

    def packed_head_params(self):
        """the head kernels' parameter buffer: W1, b1, ..., W6, b6 of `linear` in one `torch.cat`, differentiable w.r.t. each"""
        return torch.cat([t.reshape(-1) for m in self.linear if isinstance(m, nn.Linear) for t in (m.weight, m.bias)])

    def uses_fused_head(self, template_features):
        from . import pose
        shape = self.head_shape()
        t = template_features
        return (self.fused_head and shape is not None and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2
                and t.shape[0] >= 1 and t.shape[1] == shape[0] and pose.pose_head_supported(*shape)
                and self.linear[0].weight.dtype == torch.float32 and self.linear[0].weight.device == t.device)

    def uses_fused_update(self, vector, source):
        from . import pose
        return (self.fused_update and source.is_cuda and source.dtype == torch.float32 and vector.dtype == torch.float32
                and source.dim() == 3 and 1 <= source.shape[0] <= pose.MAX_CLOUDS and source.shape[1] >= 1
                and source.shape[2] == 3)

    def _pose_estimation_switched(self, template_features, source, est_R, est_t, packed=None):
        """Pose_estimation with a flag set: each half through its fused op where that applies, else as below"""
        from . import pose
        self.source_features = self.features(source, packed)
        if self.uses_fused_head(template_features):
            packed_head = self.packed_head_params() if self._packed_head is None else self._packed_head
            vector = pose.pose_head(template_features, self.source_features, packed_head, self.head_shape()[1])
        else:
            vector = self.linear(torch.cat([template_features, self.source_features], dim=1))
        if self.uses_fused_update(vector, source):
            return pose.pose_update(vector, est_R, est_t, source)
        return pose.pose_update_composed(vector, est_R, est_t, source)

    def Pose_estimation(self, template_features, source, est_R, est_t, packed=None):
        if self.fused_head or self.fused_update:
            return self._pose_estimation_switched(template_features, source, est_R, est_t, packed)
        batch_size = source.size(0)
        self.source_features = self.features(source, packed)
        pose_7d = create_pose_7d(self.linear(torch.cat([template_features, self.source_features], dim=1)))
        identity = torch.eye(3).to(source).view(1, 3, 3).expand(batch_size, 3, 3).contiguous()
        est_R_temp = quaternion_rotate(identity, pose_7d).permute(0, 2, 1)
        est_t_temp = get_translation(pose_7d).view(-1, 1, 3)
        est_t = torch.bmm(est_R_temp, est_t.permute(0, 2, 1)).permute(0, 2, 1) + est_t_temp
        est_R = torch.bmm(est_R_temp, est_R)
        source = quaternion_transform(source, pose_7d)
        return est_R, est_t, source

    def forward(self, template, source, iteration_num=8):
        batch_size = template.size(0)
        est_R = torch.eye(3).to(template).view(1, 3, 3).expand(batch_size, 3, 3).contiguous()
        est_t = torch.zeros(1, 3).to(template).view(1, 1, 3).expand(batch_size, 1, 3).contiguous()
        packed = self.feature_model.packed_params() if hasattr(self.feature_model, "packed_params") else None
        template_features = self.features(template, packed)
        if self.fused_head and self.uses_fused_head(template_features):
            self._packed_head = self.packed_head_params()              # once per forward, as the trunk's
        for _ in range(int(iteration_num)):
            est_R, est_t, source = self.Pose_estimation(template_features, source, est_R, est_t, packed)
        self._packed_head = None
        return {"est_R": est_R, "est_t": est_t, "est_T": convert2transformation(est_R, est_t),
                "r": template_features - self.source_features, "transformed_source": source}


__all__ = ["pointnet_max_features", "pointnet_max_features_composed", "pointnet_supported", "pointnet_param_count",
           "unpack_pointnet_params", "MLP_Architecture", "Pooling", "PCRNet", "qrot", "create_pose_7d", "get_quaternion",
           "get_translation", "quaternion_rotate", "quaternion_transform", "convert2transformation"]
