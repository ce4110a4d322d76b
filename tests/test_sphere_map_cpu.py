"""CPU checks of the sphere encoder (sphere_map.py): the modules and the composed path against fixture G20, which holds
what the reference's own transform_to_sphere computes and what its two phi-max wrappers do with it
(tools/make_golden_sphere_map.py); the state-dict contract; the C entries' argument handling.

Every test uses shw.sphere_map, shw.sphere_map_composed, shw.transform_to_sphere[_fast] or the shw_sphere_map_* entries:
without the feature each fails on the missing attribute.

Rule (tests/helpers/sphere_map_cases.py): float32 against the composed path in float64 on the same data, per tensor, max
|error| / max |reference entry| at most 4 x the float32 composed path's own deviation, floor 1e-6.  The module's float32
CPU path IS the float32 composed path, so against float64 it sits at a quarter of the bound by construction; against the
reference's stored float32 values it measured 0 on every tensor (the same torch operations in the same order).
The wrappers against fixture (b), measured here, float32 against the reference's float32 run: loss and trace at most
2.0e-7, parameters 2.4e-7, maps 8.0e-7, input gradients 1.8e-5 of the largest entry; float64 against its float64 run:
2.5e-8 (the batched reference sums its value in float32 whatever the input), 2.8e-16, 1.7e-15, 4.2e-14 (bounds 1e-5
relative, 1e-5 absolute twice, 1e-3).
"""
import re

import numpy as np
import pytest
import torch

from helpers.sphere_map_cases import (NAMES, PARAM_COUNT, SHAPES, bound_of, composed_reference, g20_module, g20_run,
                                      g20_state, g20_tensor, max_dev, module_results, split_params)


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    return shw_amd


@pytest.mark.parametrize("fast", [False, True], ids=["transform_to_sphere", "transform_to_sphere_fast"])
@pytest.mark.parametrize("scale", ["s1", "s3"])
def test_fixture_a_module_against_float64_and_against_the_reference(shw, scale, fast):
    """the module strictly loaded from the reference's state at both weight scales: output, d/dx and the six parameter
    gradients against the composed float64 path and against the reference's stored float32 values, under the rule"""
    x, cot = g20_tensor("a.x"), g20_tensor("a.cot")
    got = module_results(g20_module(shw, scale, fast), x, cot)
    assert got[0][1].dtype == torch.float32 and got[0][1].shape == x.shape
    params = g20_tensor(f"a.{scale}.params")
    f64, f32 = ([y, gx] + list(split_params(gp).values())
                for y, gx, gp in (composed_reference(shw, x, params, cot, dt) for dt in (torch.float64, torch.float32)))
    stored = [g20_tensor(f"a.{scale}.out"), g20_tensor(f"a.{scale}.grad_x")]
    stored += list(split_params(g20_tensor(f"a.{scale}.grad_params")).values())
    assert [n for n, _ in got[2:]] == list(NAMES)
    for (name, g), r, f, s in zip(got, f64, f32, stored):
        bound = bound_of(f, r)
        to64, to_ref = max_dev(g, r), max_dev(g, s)
        print(f"fixture (a) {scale} {name}: to float64 {to64:.2e} to the reference {to_ref:.2e} bound {bound:.2e}")
        assert torch.isfinite(g).all() and to64 <= bound and to_ref <= bound, (name, to64, to_ref, bound)


def test_state_dict_contract(shw):
    ref = g20_state("s1")
    for cls in (shw.transform_to_sphere, shw.transform_to_sphere_fast):
        torch.manual_seed(0)
        phi = cls()
        own = phi.state_dict()
        assert list(own) == list(ref) == list(NAMES)
        assert [n for n, _ in phi.named_parameters()] == list(NAMES)
        for name, shape in zip(NAMES, SHAPES):
            assert tuple(own[name].shape) == tuple(ref[name].shape) == shape and own[name].dtype == ref[name].dtype
            assert torch.equal(own[name], ref[name]), name      # nn.Linear's default initialisation from the same seed
        assert [type(m).__name__ for m in phi.net] == ["Linear", "Tanh", "Linear", "Tanh", "Linear"]
        assert sum(p.numel() for p in phi.parameters()) == PARAM_COUNT
        assert torch.equal(phi.packed_params(), g20_tensor("a.s1.params"))
    slow, fast = g20_module(shw, "s3"), shw.transform_to_sphere_fast()
    fast.load_state_dict(slow.state_dict(), strict=True)
    back = shw.transform_to_sphere()
    back.load_state_dict(fast.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), g20_state("s3").values()))
    assert isinstance(fast, shw.transform_to_sphere)


def test_c_entries_without_a_device(shw):
    lib = shw._lib.load()
    header = open(shw._lib.os.path.join(shw._lib._HERE, "..", "include", "shw.h")).read()
    for name in ("shw_sphere_map_supported", "shw_sphere_map_param_count", "shw_sphere_map_backward_blocks",
                 "shw_sphere_map_workspace_bytes", "shw_sphere_map_forward", "shw_sphere_map_backward"):
        assert re.search(r"SHW_API\s+\w+\s+%s\s*\(" % name, header), name
        assert name in shw._lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.shw_abi_version() == 3
    assert lib.shw_sphere_map_supported(3, 16, 4) == 1
    for shape in ((2, 16, 4), (4, 16, 4), (3, 8, 4), (3, 16, 2), (3, 4, 16), (0, 0, 0)):
        assert lib.shw_sphere_map_supported(*shape) == 0, shape
    assert lib.shw_sphere_map_param_count(16, 4) == PARAM_COUNT == 142
    assert lib.shw_sphere_map_param_count(8, 4) == 0 and lib.shw_sphere_map_param_count(16, 5) == 0
    # one wave per 64-point tile up to the cap, one partial vector each
    cap = lib.shw_sphere_map_backward_blocks(1 << 40)
    assert cap >= 1
    assert [lib.shw_sphere_map_backward_blocks(n) for n in (-1, 0, 1, 64, 65, 4099)] == [0, 0, 1, 1, 2, min(65, cap)]
    assert lib.shw_sphere_map_backward_blocks(64 * cap) == cap == lib.shw_sphere_map_backward_blocks(64 * cap + 1)
    for n in (0, -5, 1, 65, 64 * cap + 1):
        assert lib.shw_sphere_map_workspace_bytes(n) == max(lib.shw_sphere_map_backward_blocks(n), 0) * PARAM_COUNT * 4
    # null or invalid arguments: 1 (hipErrorInvalidValue) before any HIP call
    assert lib.shw_sphere_map_forward(None, 8, 64, 8, None) == 1
    assert lib.shw_sphere_map_forward(8, None, 64, 8, None) == 1
    assert lib.shw_sphere_map_forward(8, 8, 64, None, None) == 1
    assert lib.shw_sphere_map_forward(8, 8, -1, 8, None) == 1
    assert lib.shw_sphere_map_forward(8, 8, 0, 8, None) == 0
    assert lib.shw_sphere_map_backward(None, 8, 8, 64, 8, 8, 8, None) == 1
    assert lib.shw_sphere_map_backward(8, None, 8, 64, 8, 8, 8, None) == 1
    assert lib.shw_sphere_map_backward(8, 8, None, 64, 8, 8, 8, None) == 1
    assert lib.shw_sphere_map_backward(8, 8, 8, -1, 8, 8, 8, None) == 1
    assert lib.shw_sphere_map_backward(8, 8, 8, 64, 8, 8, None, None) == 1      # gparams without a workspace
    assert lib.shw_sphere_map_backward(8, 8, 8, 64, None, None, None, None) == 0   # nothing asked for


def test_the_op_refuses_what_it_cannot_take(shw):
    x, params = torch.zeros(8, 3), torch.zeros(PARAM_COUNT)
    with pytest.raises(RuntimeError, match="needs device tensors"):
        shw.sphere_map(x, params)
    with pytest.raises(TypeError):
        shw.sphere_map(x.numpy(), params)
    with pytest.raises(ValueError, match="142"):
        shw.sphere_map_composed(x, torch.zeros(PARAM_COUNT - 1))
    with pytest.raises(ValueError, match="dimension 3"):
        shw.sphere_map_composed(torch.zeros(8, 4), params)
    phi = shw.transform_to_sphere()
    with pytest.raises(ValueError, match=r"\(B, N, 3\)"):
        phi(x)                                                    # the reference indexes x[:, :, 0]: rank 3 only


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
def test_module_on_the_cpu_is_the_composed_path_bit_for_bit(shw, dtype):
    x, cot = g20_tensor("a.x").to(dtype), g20_tensor("a.cot").to(dtype)
    phi = g20_module(shw, "s3").to(dtype)
    got = module_results(phi, x, cot)
    xs, ps = x.clone().requires_grad_(), g20_tensor("a.s3.params").to(dtype).requires_grad_()
    y = shw.sphere_map_composed(xs, ps)
    (y * cot).sum().backward()
    want = [y.detach(), xs.grad] + list(split_params(ps.grad).values())
    assert got[0][1].dtype == dtype
    for (name, g), w in zip(got, want):
        assert torch.equal(g, w), name
    assert (y.detach().norm(dim=-1) - 1).abs().max() < (1e-6 if dtype == torch.float32 else 1e-15)
    # a net edited to another width runs composed, layer by layer
    phi.net[2] = torch.nn.Linear(16, 5).to(dtype)
    phi.net[4] = torch.nn.Linear(5, 2).to(dtype)
    assert (phi(x).norm(dim=-1) - 1).abs().max() < 1e-6


@pytest.mark.parametrize("dtype_name", ["f32", "f64"])
@pytest.mark.parametrize("tag", ["pair", "fast"])
@pytest.mark.parametrize("mode", ["train", "test"])
def test_fixture_b_wrappers_host_logic_with_the_cpu_oracle_as_ssw(shw, tag, mode, dtype_name):
    """The package's wrappers with the CPU module as phi, Adam(lr=0.01, betas=(0.5, 0.999)) and the CPU oracle on the
    fixture's fixed frames as SSW must retrace what the REAL wrappers did with the REAL encoder and sliced_cost
    (max_spherical_sliced_w.py:498-536, _fast.py:346-380): the per-iteration values the reference printed, the parameters
    after max_iter ascent steps, the returned value, the maps and the gradients w.r.t. both inputs.  Bounds as for fixture
    G8 (tests/test_oracle_golden.py): 1e-5 relative on values, 1e-5 absolute on parameters and maps, 1e-3 of the largest
    entry on the input gradients."""
    from oracle import ref_mirror
    dtype = torch.float32 if dtype_name == "f32" else torch.float64
    want = g20_run(dtype_name, tag, mode)
    lr, betas = float(g20_tensor("b.lr")), tuple(float(b) for b in g20_tensor("b.betas"))
    assert (lr, betas, int(g20_tensor("b.max_iter"))) == (0.01, (0.5, 0.999), 2)
    if tag == "pair":
        U = g20_tensor("b.U_pair").to(dtype)
        cls, phi = shw.max_spherical_wassersten_distance, g20_module(shw, "s3")
        ssw = lambda a, b, L, device, p=2: ref_mirror.sliced_cost(a, b, U, p=p)                 # noqa: E731
    else:
        U = g20_tensor("b.U_batch").to(dtype)
        cls, phi = shw.max_spherical_wassersten_distance_fast, g20_module(shw, "s3", fast=True)
        ssw = lambda a, b, L, device, p=2: ref_mirror.sliced_cost_batched(a, b, U, p=p)         # noqa: E731
    phi = phi.to(dtype)
    opt = torch.optim.Adam(phi.parameters(), lr=lr, betas=betas)
    crit = cls(U.shape[-3], phi, ssw, opt, p=2, max_iter=2, device="cpu")
    trace = []
    crit.on_inner_value = trace.append
    a, b = g20_tensor("b.first").to(dtype).requires_grad_(), g20_tensor("b.second").to(dtype).requires_grad_()
    val, fa, fb = crit(a, b, train_or_test=mode)
    opt.zero_grad()
    val.sum().backward()
    rel = lambda got, ref: float(np.max(np.abs(np.asarray(got, np.float64) - ref) / np.abs(ref)))   # noqa: E731
    figures = {"ssw": rel(val.detach().numpy().reshape(-1), want["ssw"])}
    assert len(trace) == len(want["trace"]) == (2 if mode == "train" else 0)
    if trace:
        figures["trace"] = rel(trace, want["trace"])
    figures["params"] = float(np.abs(phi.packed_params().detach().numpy() - want["params"]).max())
    figures["phi_first"] = float(np.abs(fa.detach().numpy() - want["phi_first"]).max())
    figures["phi_second"] = float(np.abs(fb.detach().numpy() - want["phi_second"]).max())
    figures["g_first"] = float(np.abs(a.grad.numpy() - want["g_first"]).max() / np.abs(want["g_first"]).max())
    figures["g_second"] = float(np.abs(b.grad.numpy() - want["g_second"]).max() / np.abs(want["g_second"]).max())
    print(f"fixture (b) {dtype_name} {tag} {mode}:", {k: f"{v:.1e}" for k, v in figures.items()})
    assert fa.dtype == dtype and fa.shape == a.shape
    if mode == "test":
        assert np.array_equal(want["params"].astype(np.float32), g20_tensor("a.s3.params").numpy())
    for name, figure in figures.items():
        assert figure < (1e-3 if name.startswith("g_") else 1e-5), (name, figure)
