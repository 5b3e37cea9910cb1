"""h3d_isosurface_count / h3d_isosurface_emit (csrc/isosurface.hip) through lib/components/isosurface.py against the float64
restatement tests/_isosurface_reference.py, on the same fp32 volume.

Exact: the vertex count, the edge every vertex sits on (its rank among the crossing edges in ascending edge id), and the faces row
for row after rotating each face so that its smallest index comes first.
Positions: within 8 * 2^-23 * max|coordinate| of the case.  s = (level - a) / (b - a) takes three roundings, p + s d one, the
product with the spacing one, the sum with the origin one; every one of them is at most half an ulp of a quantity no larger than
the largest coordinate (s <= 1 multiplies an edge of the grid), so the position is within three ulp = 3 * 2^-23 relative of it;
the factor 8 leaves room for fused multiply-adds contracting differently.  Applied with a non-trivial origin and anisotropic
spacing.
Shapes: every case of tests/test_isosurface_cpu.py; 3x5x4 and 65x3x2 (smaller than a tile, one axis longer than four tiles);
40x24x20 (more than one workgroup along every axis of the 8x8x16 tile, ragged on every axis)."""
import importlib

import numpy as np
import pytest
import torch

import _isosurface_reference as R

pytestmark = pytest.mark.gpu
iso = importlib.import_module("3dhumangan_amd.lib.components.isosurface")
DEV = "cuda"
ORIGIN, SPACING = (0.3, -1.2, 2.5), (0.5, 1.25, 0.75)

CASES = {
    "sphere-9": (lambda: R.sphere((9, 9, 9), 3.0), 0.0),
    "sphere-17": (lambda: R.sphere((17, 17, 17), 6.0), 0.0),
    "sphere-12x9x15": (lambda: R.sphere((12, 9, 15), 3.3), 0.0),
    "torus-21x21x11": (lambda: R.torus((21, 21, 11), 6.0, 2.0), 0.0),
    "values-on-the-level": (lambda: R.octahedron(7, 4.0), 2.0),
    "border-6x5x4": (lambda: R.sphere((6, 5, 4), 3.0, centre=(0.2, 0.1, 0.3)), 0.0),
    "smooth-3x5x4": (lambda: R.smooth_random((3, 5, 4), 1), 0.05),
    "smooth-65x3x2": (lambda: R.smooth_random((65, 3, 2), 2), 0.05),
    "smooth-40x24x20": (lambda: R.smooth_random((40, 24, 20), 3), 0.1),
}
_REFERENCE = {}


def case(name):
    """-> (fp32 volume, level, reference vertices, faces, edge ids), computed once per case and never modified"""
    if name not in _REFERENCE:
        make, level = CASES[name]
        volume = make()
        _REFERENCE[name] = (volume, level) + R.marching_tetrahedra(volume, level, ORIGIN, SPACING)
    return _REFERENCE[name]


def run(volume, level, origin=ORIGIN, spacing=SPACING):
    v, f = iso.marching_tetrahedra(torch.as_tensor(volume).to(DEV), level, origin, spacing)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.is_cuda and f.is_cuda
    assert v.dim() == 2 and v.shape[1] == 3 and f.dim() == 2 and f.shape[1] == 3
    return v.cpu().numpy(), f.cpu().numpy()


def vertex_counts(volume, level):
    """h3d_isosurface_count alone -> crossing edges per lower node, int32 [nodes]"""
    L = importlib.import_module("3dhumangan_amd._lib")
    t = torch.as_tensor(volume).to(DEV).contiguous()
    Nx, Ny, Nz = t.shape
    vc = torch.full((Nx * Ny * Nz,), -1, dtype=torch.int32, device=DEV)
    tc = torch.full(((Nx - 1) * (Ny - 1) * (Nz - 1),), -1, dtype=torch.int32, device=DEV)
    L.check(L.load().h3d_isosurface_count(L.ptr(t), Nx, Ny, Nz, float(level), L.ptr(vc), L.ptr(tc), L.stream_handle()), "count")
    return vc.cpu().numpy(), tc.cpu().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_the_restatement(name):
    volume, level, ref_v, ref_f, ref_edges = case(name)
    assert len(ref_f) > 0
    v, f = run(volume, level)
    # edge assignment: vertex i is the i-th crossing edge in ascending edge id on both sides; the crossing edges per lower node are
    # compared exactly, the positions below tell two edges of one node apart
    vc, tc = vertex_counts(volume, level)
    assert np.array_equal(vc, np.bincount(ref_edges // 7, minlength=volume.size))
    assert tc.min() >= 0 and tc.max() <= 12 and int(tc.sum()) == len(ref_f)
    assert len(v) == len(ref_v)
    assert f.shape == ref_f.shape
    assert np.array_equal(R.canonical(f), R.canonical(ref_f))
    err, bar = float(np.abs(v.astype(np.float64) - ref_v).max()), 8 * 2.0 ** -23 * float(np.abs(ref_v).max())
    print(f"{name}: V {len(v)} T {len(f)} position error {err:.3e} bar {bar:.3e}")
    assert err <= bar


def test_every_sign_pattern_of_one_cell():
    total = 0
    for pattern in range(1, 255):
        cell = np.array([(pattern >> c) & 1 for c in range(8)], dtype=np.float32).reshape(2, 2, 2)
        ref_v, ref_f, _ = R.marching_tetrahedra(cell, 0.5)
        v, f = run(cell, 0.5, (0, 0, 0), (1, 1, 1))
        assert np.array_equal(R.canonical(f), R.canonical(ref_f)) and np.array_equal(v, ref_v.astype(np.float32))
        total += len(f)
    assert total == 1920


@pytest.mark.parametrize("value", [1.0, -1.0, 0.0])
def test_no_surface_gives_empty_tensors(value):
    """all inside, all outside, and all equal to the level (outside)"""
    v, f = run(np.full((5, 9, 17), value, dtype=np.float32), 0.0)
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_non_contiguous_view_is_made_contiguous():
    volume, level, ref_v, ref_f, _ = case("sphere-12x9x15")
    t = torch.as_tensor(volume).to(DEV)
    view = t.permute(2, 1, 0).contiguous().permute(2, 1, 0)
    assert not view.is_contiguous() and torch.equal(view, t)
    v, f = iso.marching_tetrahedra(view, level, ORIGIN, SPACING)
    v0, f0 = iso.marching_tetrahedra(t, level, ORIGIN, SPACING)
    assert torch.equal(v, v0) and torch.equal(f, f0) and len(v) == len(ref_v)
    padded = torch.zeros(12, 9, 20, device=DEV)
    padded[..., :15] = t
    v1, f1 = iso.marching_tetrahedra(padded[..., :15], level, ORIGIN, SPACING)
    assert torch.equal(v1, v0) and torch.equal(f1, f0)


def test_two_runs_are_bit_identical():
    volume, level, _, _, _ = case("smooth-40x24x20")
    t = torch.as_tensor(volume).to(DEV)
    a, b = iso.marching_tetrahedra(t, level, ORIGIN, SPACING), iso.marching_tetrahedra(t, level, ORIGIN, SPACING)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_non_finite_values_keep_every_index_in_range():
    volume = R.smooth_random((19, 11, 21), 4).copy()
    flat = volume.reshape(-1)
    flat[::7], flat[3::11], flat[5::13] = np.nan, np.inf, -np.inf
    _, ref_f, _ = R.marching_tetrahedra(volume, 0.0)
    v, f = run(volume, 0.0)
    assert np.array_equal(R.canonical(f), R.canonical(ref_f))         # NaN compares false: outside, on both sides
    assert f.min() >= 0 and f.max() < len(v)


def test_refusals():
    h3dlib = importlib.import_module("3dhumangan_amd._lib")
    with pytest.raises(h3dlib.H3DError, match="at least 2 nodes"):
        iso.marching_tetrahedra(torch.zeros(1, 4, 4, device=DEV), 0.0)
    with pytest.raises(ValueError):
        iso.marching_tetrahedra(torch.zeros(4, 4, 4, device=DEV, dtype=torch.float64), 0.0)
    with pytest.raises(ValueError):
        iso.marching_tetrahedra(torch.zeros(4, 4, device=DEV), 0.0)
