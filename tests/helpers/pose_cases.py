"""Shared cases of the pose tests (tests/test_pose_cpu.py, tests/test_pose_gpu.py): inputs of `pose_head` and
`pose_update`, and their float64 / float32 references from the composed torch path on the CPU, each computed once.

Error rule (tests/helpers/pcrnet_cases.py): a float32 result is compared with the composed path in float64 on the same
float32 data, per tensor, on max |error| / max |reference entry|; the bound is 4 x the deviation of the float32 composed
CPU path from the float64 one on the same case, floor 1e-6.  The head's parameter gradient is split into its twelve tensors.

Margin condition of the head: a ReLU whose sign differs between the two precisions moves a whole gradient term, so every
head case asserts, in float64, that each hidden pre-activation lies at least MARGIN * max |z| of its layer away from 0.
Seeds are chosen for which this holds (`find_seed` searches them on the CPU).  The float32 composed path deviates
2-6e-7 from float64, so the margin is about 30 x the rounding."""
import numpy as np
import torch

MARGIN = 1e-5
REFERENCE_WIDTHS = (1024, 1024, 512, 512, 256)
SMALL_WIDTHS = (64, 32, 96, 32, 32)
ALL_32 = (32, 32, 32, 32, 32)


# ------------------------------------------------------------------------------------------------ the head
def head_inputs(emb, widths, B, seed, dead_layer=None):
    """template and source features (non-negative, as a max-pooled ReLU output is), packed parameters of unit gain
    (weights uniform in +-sqrt(3 / fan_in), biases uniform in +-0.2) and a cotangent; `dead_layer` = k puts every bias of
    hidden layer k (1..5) at -10"""
    g = torch.Generator().manual_seed(700001 * seed + 1013 * emb + 37 * B + sum(widths))
    tf, sf = torch.randn(B, emb, generator=g).abs(), torch.randn(B, emb, generator=g).abs()
    sizes = (2 * emb,) + tuple(widths) + (7,)
    parts = []
    for k in range(6):
        out, inp = sizes[k + 1], sizes[k]
        parts.append(((torch.rand(out * inp, generator=g, dtype=torch.float64) * 2 - 1) * np.sqrt(3.0 / inp)).float())
        bias = ((torch.rand(out, generator=g, dtype=torch.float64) * 2 - 1) * 0.2).float()
        if dead_layer == k + 1:
            bias.fill_(-10.0)
        parts.append(bias)
    cot = torch.randn(B, 7, generator=g)
    return tf, sf, torch.cat(parts), cot


def head_margin(shw, tf, sf, params, widths):
    """the smallest |z| / max |z| over the five hidden layers' pre-activations, in float64"""
    h = torch.cat([tf, sf], dim=1).double()
    worst = float("inf")
    for weight, bias in shw.unpack_pose_head_params(params.double(), tf.shape[1], widths)[:-1]:
        z = torch.nn.functional.linear(h, weight, bias)
        worst = min(worst, float(z.abs().min() / z.abs().max()))
        h = torch.relu(z)
    return worst


def find_seed(shw, emb, widths, B, dead_layer=None, tries=100):
    """the first seed whose case meets the margin condition (used when the cases of test_pose_gpu.py were written)"""
    for seed in range(tries):
        tf, sf, params, _ = head_inputs(emb, widths, B, seed, dead_layer)
        if head_margin(shw, tf, sf, params, widths) >= MARGIN:
            return seed
    raise AssertionError((emb, widths, B, dead_layer))


def split_head_grads(shw, triple, emb, widths):
    """(value, gtf, gsf, gparams) -> name -> tensor, the parameter gradient as its twelve tensors"""
    out = {"value": triple[0], "d/dtemplate_features": triple[1], "d/dsource_features": triple[2]}
    for n, (weight, bias) in enumerate(shw.unpack_pose_head_params(triple[3], emb, widths), start=1):
        out[f"dW{n}"], out[f"db{n}"] = weight, bias
    return out


def head_reference(shw, tf, sf, params, cot, widths, dtype):
    t, s, p = (v.detach().cpu().to(dtype).requires_grad_() for v in (tf, sf, params))
    y = shw.pose_head_composed(t, s, p, widths)
    (y * cot.detach().cpu().to(dtype)).sum().backward()
    return y.detach(), t.grad, s.grad, p.grad


_HEAD = {}


def head_case(shw, emb, widths, B, seed, dead_layer=None):
    """dict: tf, sf, params, cot (float32) and the f64 / f32 references (value, gtf, gsf, gparams) of the composed CPU
    path; computed once and shared.  Asserts the margin condition."""
    key = (emb, tuple(widths), B, seed, dead_layer)
    if key not in _HEAD:
        tf, sf, params, cot = head_inputs(emb, widths, B, seed, dead_layer)
        margin = head_margin(shw, tf, sf, params, widths)
        assert margin >= MARGIN, (key, margin)
        _HEAD[key] = {"tf": tf, "sf": sf, "params": params, "cot": cot,
                      "f64": head_reference(shw, tf, sf, params, cot, widths, torch.float64),
                      "f32": head_reference(shw, tf, sf, params, cot, widths, torch.float32)}
    return _HEAD[key]


# ------------------------------------------------------------------------------------------------ the pose update
UPDATE_INPUTS = ("vector", "est_R", "est_t", "source")
UPDATE_OUTPUTS = ("est_R", "est_t", "source")


def update_inputs(B, N, seed=0, scale=1.0, quaternion=None):
    """vector (standard normal times `scale`, or with the given quaternion in every cloud), est_R (any 3 x 3 matrices),
    est_t, source and the three cotangents"""
    g = torch.Generator().manual_seed(900007 * seed + 131 * B + N)
    vector = torch.randn(B, 7, generator=g) * scale
    if quaternion is not None:
        vector[:, :4] = torch.tensor(quaternion, dtype=torch.float32)
    inputs = (vector, torch.randn(B, 3, 3, generator=g), torch.randn(B, 1, 3, generator=g), torch.randn(B, N, 3, generator=g))
    cots = (torch.randn(B, 3, 3, generator=g), torch.randn(B, 1, 3, generator=g), torch.randn(B, N, 3, generator=g))
    return inputs, cots


def run_update(fn, inputs, cots, device, dtype, use=(True, True, True), want=(True, True, True, True)):
    """(outputs, gradients) of sum over the used outputs of output * cotangent; a gradient not asked for is None"""
    leaves = [t.detach().to(device=device, dtype=dtype).requires_grad_(w) for t, w in zip(inputs, want)]
    outs = fn(*leaves)
    loss = sum((o * c.to(device=device, dtype=dtype)).sum() for o, c, u in zip(outs, cots, use) if u)
    if any(want) and any(use):
        loss.backward()
    return [o.detach() for o in outs], [t.grad for t in leaves]


_UPDATE = {}


def update_case(shw, B, N, seed=0, scale=1.0, quaternion=None):
    """dict: inputs, cots (float32) and the f64 / f32 (outputs, gradients) of the composed CPU path, all cotangents used"""
    key = (B, N, seed, scale, quaternion)
    if key not in _UPDATE:
        inputs, cots = update_inputs(B, N, seed, scale, quaternion)
        _UPDATE[key] = {"inputs": inputs, "cots": cots,
                        "f64": run_update(shw.pose_update_composed, inputs, cots, "cpu", torch.float64),
                        "f32": run_update(shw.pose_update_composed, inputs, cots, "cpu", torch.float32)}
    return _UPDATE[key]
