"""CPU checks of the frame-gradient entries (csrc/shw_ssw_dirs.hip) and of what the GPU file rests on (no GPU needed).

The three entries are declared, bound and exported at ABI 3, and refuse bad arguments before any HIP call.  The formula
the kernels implement, restated in float64 on the mirror's own coefficient rows (helpers/ssw_dirs_cases.closed_form),
equals autograd through `oracle.ref_mirror` on every case the GPU file uses; and on each of those cases the mirror's
float32 gradient stays within 2e-4 of the largest entry of its float64 gradient -- the condition under which the GPU
file's bound of 1e-3 says something about the kernel and not about the inputs."""
import ctypes
import os
import re

import pytest
import torch

from helpers import ssw_dirs_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("shw_ssw_backward_dirs", "shw_ssw_backward_dirs_dim", "shw_ssw_backward_dirs_f64")


@pytest.fixture(scope="module")
def shw():
    import shw_amd
    if not os.path.exists(shw_amd._lib.LIB_PATH):
        shw_amd._lib.build()
    return shw_amd


def test_entries_are_declared_bound_and_exported(shw):
    header = open(os.path.join(ROOT, "include", "shw.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = shw._lib.load()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in shw._lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    section = header[:header.index("SHW_API int shw_ssw_backward_dirs(")].rsplit("/* ---", 1)[1]
    assert "additive to ABI 3" in section and "shw_ssw_dirs.hip" in section
    assert lib.shw_abi_version() == shw._lib.ABI_VERSION == 3
    assert "max_sliced_wasserstein_sphere" in shw.__all__ and callable(shw.max_sliced_wasserstein_sphere)


def test_invalid_arguments_return_1_before_any_hip_call(shw):
    lib = shw._lib.load()
    one = ctypes.c_void_p(16)             # a non-null pointer that is never dereferenced: validation comes first

    def r3(entry=lib.shw_ssw_backward_dirs, pairs=1, n=8, m=8, slices=2, stride=0, ptrs=(one,) * 6, grad=one):
        return entry(*ptrs[:5], pairs, n, m, slices, stride, 1.0, None, None, grad, None)

    def dim(pairs=1, n=8, m=8, d=8, slices=2, stride=0, ptrs=(one,) * 5, grad=one):
        return lib.shw_ssw_backward_dirs_dim(*ptrs, pairs, n, m, d, slices, stride, 1.0, None, None, grad, None)

    for entry in (lib.shw_ssw_backward_dirs, lib.shw_ssw_backward_dirs_f64):
        for k in range(5):
            assert r3(entry, ptrs=tuple(None if j == k else one for j in range(5))) == 1
        assert r3(entry, grad=None) == 1
        assert r3(entry, n=0) == 1 and r3(entry, m=0) == 1 and r3(entry, pairs=-1) == 1 and r3(entry, slices=-1) == 1
        assert r3(entry, stride=11) == 1                     # per-pair frames need slices * 6 floats per pair
        assert r3(entry, pairs=0) == 0                       # nothing to do, nothing launched
    assert r3(n=lib.shw_max_points() + 1) == 1 and r3(m=lib.shw_max_points() + 1) == 1
    limit64 = max(lib.shw_max_points_f64(), lib.shw_max_points_f64_general())
    assert r3(lib.shw_ssw_backward_dirs_f64, n=limit64 + 1) == 1
    for k in range(5):
        assert dim(ptrs=tuple(None if j == k else one for j in range(5))) == 1
    assert dim(grad=None) == 1
    assert dim(d=1) == 1 and dim(d=65) == 1 and dim(d=0) == 1
    assert dim(n=0) == 1 and dim(m=lib.shw_max_points() + 1) == 1 and dim(pairs=-1) == 1
    assert dim(stride=31) == 1                               # slices * dim * 2 = 32
    assert dim(pairs=0) == 0 and dim(pairs=0, d=64) == 0


def test_case_list_covers_what_the_kernels_branch_on():
    every = cases.CASES
    assert {1, 7, 63, 64, 65, 255, 256, 257, 1000} <= {c.n for c in every if c.n == c.m}
    assert {(300, 200), (65, 7)} <= {(c.n, c.m) for c in every}
    assert any(c.weighted and c.n == c.m == 200 for c in every)
    assert {1, 1.5, 2, 3} <= {c.p for c in every} and {1, 3} <= {c.B for c in every} and {1, 3, 17} <= {c.L for c in every}
    assert {2, 3, 4, 8, 63, 64} <= {c.d for c in every}
    assert {True, False} <= {c.shared for c in every}
    assert any(c.d == 3 and c.B * c.L >= 8192 and c.L % 4 for c in every)   # four rows per wavefront, partial last group
    assert any(c.d != 3 and c.B * c.L >= 4096 and c.L % 4 for c in every)   # the same in the D-generic kernel


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.name)
def test_closed_form_equals_mirror_autograd_and_float32_mirror_is_close(case):
    x, y, U, wu, wv = cases.inputs(case)
    ref = cases.reference(case.name)
    scale = ref.abs().max().item()
    assert scale > 0
    restated = cases.closed_form_total(x, y, U, case.p, wu, wv)
    err = (restated - ref).abs().max().item()
    f32 = torch.float32
    g32 = cases.mirror_grad(x.to(f32), y.to(f32), U.to(f32), case.p, cases.cast(wu, f32), cases.cast(wv, f32))
    gap = (g32.double() - ref).abs().max().item()
    print(f"{case.name}: closed form {err / scale:.2e}, float32 mirror {gap / scale:.2e} of the largest entry {scale:.3e}")
    assert err <= 1e-12 * scale
    assert gap <= 2e-4 * scale


def test_mirror_gradient_satisfies_the_identities_except_rotation_at_p1():
    """Scaling a frame never changes a coordinate, so <g[:,0], u1> + <g[:,1], u2> = 0 for every p.  Rotating it in its
    plane shifts every coordinate by one constant; the circular OT cost for p != 1 does not see that, so
    <g[:,0], u2> - <g[:,1], u1> = 0 there -- but p = 1 is the reference's level-median formula, which leaves out the
    wrap segment and depends on where the seam lies: its float64 gradient breaks the rotation identity, which is why the
    GPU file asks it of p != 1 only."""
    broken = []
    for case in cases.CASES:
        if case.shared:
            continue
        g, U = cases.reference(case.name).reshape(-1, case.d, 2), cases.inputs(case)[2].reshape(-1, case.d, 2)
        norm = g.flatten(1).norm(dim=1)
        rot = (((g[..., 0] * U[..., 1]).sum(-1) - (g[..., 1] * U[..., 0]).sum(-1)).abs() / norm).max().item()
        scl = (((g[..., 0] * U[..., 0]).sum(-1) + (g[..., 1] * U[..., 1]).sum(-1)).abs() / norm).max().item()
        assert scl < 1e-12, (case.name, scl)
        if case.p == 1:
            broken.append(rot)
        else:
            assert rot < 1e-12, (case.name, rot)
    assert broken and min(broken) > 1e-3, broken


def test_gradcheck_inputs_of_the_gpu_file_keep_their_margins():
    x, y, U = cases.gradcheck_equal()
    for p in (1.5, 2):
        assert cases.gradcheck_margins_ok(x, y, U, None, None, p)
    x, y, U, wu, wv = cases.gradcheck_general()
    for p in (1.5, 2):
        assert cases.gradcheck_margins_ok(x, y, U, wu, wv, p)


def test_retraction_is_orthonormal_and_keeps_every_column_sign(shw):
    g = torch.Generator().manual_seed(5)
    Z = torch.randn(50, 7, 2, generator=g, dtype=torch.float64)
    Q = shw.retract_frames(Z)
    eye = torch.eye(2, dtype=torch.float64).expand(50, 2, 2)
    assert (Q.transpose(-1, -2) @ Q - eye).abs().max() < 1e-12
    assert ((Q * Z).sum(-2) > 0).all()
