"""The float64 restatement of the iso-surface extraction (tests/_isosurface_reference.py) held to what a correct marching-tetrahedra
surface must satisfy -- so that the GPU tests (tests/test_gpu_isosurface.py) compare the kernel with something that is itself
checked -- plus the parts of the feature that need no GPU: the PLY writer and the argument checks of the two C-ABI entry points."""
import ctypes
import importlib

import numpy as np
import pytest

import _isosurface_reference as R

SPHERES = (((9, 9, 9), 3.0, 490, 976), ((17, 17, 17), 6.0, 2026, 4048), ((12, 9, 15), 3.3, 608, 1212))
_MESHES = {}


def sphere_mesh(shape, radius):
    if (shape, radius) not in _MESHES:
        _MESHES[shape, radius] = R.marching_tetrahedra(R.sphere(shape, radius), 0.0)[:2]
    return _MESHES[shape, radius]


@pytest.mark.parametrize("shape,radius,n_vertices,n_faces", SPHERES)
def test_sphere_is_a_closed_oriented_surface_of_genus_zero(shape, radius, n_vertices, n_faces):
    v, f = sphere_mesh(shape, radius)
    assert (len(v), len(f)) == (n_vertices, n_faces)
    assert R.is_closed_and_oriented(len(v), f)          # every edge in two faces, every directed edge once, every vertex used
    assert R.euler_characteristic(len(v), f) == 2


def test_sphere_volume_is_inscribed_and_converges():
    """The vertices lie on chords of the sphere's distance field, so the surface is inscribed: the signed volume is positive (the
    normals point outwards) and below the analytic one, and the relative deficit shrinks with the resolution."""
    deficit = {}
    for shape, radius, _, _ in SPHERES[:2]:
        v, f = sphere_mesh(shape, radius)
        volume, analytic = R.signed_volume(v, f), 4.0 / 3.0 * np.pi * radius ** 3
        print(f"r={radius}: volume {volume:.3f} analytic {analytic:.3f} deficit {1 - volume / analytic:.4f}")
        assert 0 < volume < analytic
        deficit[radius] = 1 - volume / analytic
    assert deficit[6.0] < deficit[3.0]
    v, f = sphere_mesh(*SPHERES[2][:2])
    assert 0 < R.signed_volume(v, f) < 4.0 / 3.0 * np.pi * 3.3 ** 3


def test_torus_has_genus_one():
    v, f, _ = R.marching_tetrahedra(R.torus((21, 21, 11), 6.0, 2.0), 0.0)
    assert R.is_closed_and_oriented(len(v), f)
    assert R.euler_characteristic(len(v), f) == 0
    assert R.signed_volume(v, f) > 0


def test_node_values_equal_to_the_level():
    """4 - |x - 3|_1 in 7^3 at level 2: 18 nodes sit exactly on the level (they count as outside), triangles collapse onto them.
    The surface stays closed and consistently oriented because the orientation never looks at the positions."""
    field = R.octahedron(7, 4.0)
    assert int((field == 2.0).sum()) > 0
    v, f, _ = R.marching_tetrahedra(field, 2.0)
    assert (len(v), len(f)) == (74, 144)
    assert np.isfinite(v).all()
    assert R.is_closed_and_oriented(len(v), f)
    assert R.euler_characteristic(len(v), f) == 2


def test_every_sign_pattern_of_one_cell():
    total = 0
    for pattern in range(256):
        cell = np.array([(pattern >> c) & 1 for c in range(8)], dtype=np.float32).reshape(2, 2, 2)
        v, f, edges = R.marching_tetrahedra(cell, 0.5)
        assert len(edges) == len(v) and (np.diff(edges) > 0).all()
        if len(f):
            assert f.min() >= 0 and f.max() < len(v)
            assert np.isin(v, (0.0, 0.5, 1.0)).all()                       # values 0 / 1 at level 1/2: every vertex at a midpoint
        total += len(f)
    assert total == 1920           # per tetrahedron 8 patterns with one triangle and 6 with two, each seen 16 times, 6 tetrahedra


def test_surface_leaving_the_grid_is_open_with_indices_in_range():
    v, f, _ = R.marching_tetrahedra(R.sphere((6, 5, 4), 3.0, centre=(0.2, 0.1, 0.3)), 0.0)
    assert len(f) > 0 and f.min() >= 0 and f.max() < len(v)
    directed, counts = R.edge_census(f)
    assert (counts <= 2).all() and (counts == 1).any()                     # a boundary, and no edge in three faces
    assert len(np.unique(directed, axis=0)) == len(directed)               # still consistently oriented


def test_origin_and_spacing_move_the_vertices_only():
    field = R.sphere((9, 9, 9), 3.0)
    v0, f0, e0 = R.marching_tetrahedra(field, 0.0)
    v1, f1, e1 = R.marching_tetrahedra(field, 0.0, origin=(0.3, -1.2, 2.5), spacing=(0.5, 1.25, 0.75))
    assert np.array_equal(f0, f1) and np.array_equal(e0, e1)
    assert np.allclose(v1, np.array([0.3, -1.2, 2.5]) + np.array([0.5, 1.25, 0.75]) * v0, rtol=0, atol=1e-12)


def test_write_ply_round_trip(tmp_path):
    mesh_io = importlib.import_module("3dhumangan_amd.lib.components.mesh_io")
    v, f = sphere_mesh((9, 9, 9), 3.0)
    path = str(tmp_path / "sphere.ply")
    mesh_io.write_ply(path, v.astype(np.float32), f.astype(np.int32))
    v2, f2 = R.parse_ply(path)
    assert np.array_equal(v2, v.astype(np.float32)) and np.array_equal(f2, f)
    import torch
    mesh_io.write_ply(path, torch.as_tensor(v, dtype=torch.float32), torch.as_tensor(f, dtype=torch.int32))     # tensors as well
    v3, f3 = R.parse_ply(path)
    assert np.array_equal(v3, v2) and np.array_equal(f3, f2)
    mesh_io.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))                            # an empty surface
    v4, f4 = R.parse_ply(path)
    assert v4.shape == (0, 3) and f4.shape == (0, 3)
    with pytest.raises(ValueError):
        mesh_io.write_ply(path, v[:10].astype(np.float32), f.astype(np.int32))


@pytest.fixture(scope="module")
def lib():
    build = importlib.import_module("3dhumangan_amd._build")
    handle = ctypes.CDLL(build.build_lib())
    sig = importlib.import_module("3dhumangan_amd._lib")._SIGNATURES
    for name in ("h3d_isosurface_count", "h3d_isosurface_emit", "h3d_last_error"):
        getattr(handle, name).restype, getattr(handle, name).argtypes = sig[name]
    return handle


def test_argument_validation_needs_no_gpu(lib):
    """Both entry points refuse bad arguments by name, with -1, before any HIP call (the pointers below are never dereferenced)."""
    p = ctypes.c_void_p(64)
    three = (ctypes.c_float * 3)(1, 1, 1)
    count = lambda vol, nx, ny, nz, vc=p, tc=p: lib.h3d_isosurface_count(vol, nx, ny, nz, 0.0, vc, tc, None)
    emit = lambda vol, nx, ny, nz, V=1, T=1, vo=p: lib.h3d_isosurface_emit(vol, nx, ny, nz, 0.0, three, three, vo, p, p, V, p, T, None)
    assert count(None, 4, 4, 4) == -1 and b"h3d_isosurface_count: null pointer" in lib.h3d_last_error()
    assert count(p, 4, 4, 4, tc=None) == -1 and b"null pointer" in lib.h3d_last_error()
    assert emit(None, 4, 4, 4) == -1 and b"h3d_isosurface_emit: null pointer" in lib.h3d_last_error()
    assert emit(p, 4, 4, 4, vo=None) == -1 and b"null pointer" in lib.h3d_last_error()
    for fn, who in ((count, b"h3d_isosurface_count"), (emit, b"h3d_isosurface_emit")):
        assert fn(p, 1, 4, 4) == -1 and who in lib.h3d_last_error() and b"at least 2 nodes" in lib.h3d_last_error()
        assert fn(p, 4, 4, 1) == -1 and b"at least 2 nodes" in lib.h3d_last_error()
        # 7 * 675 * 675 * 675 = 2 152 828 125 >= 2^31, 7 * 674^3 < 2^31
        assert fn(p, 675, 675, 675) == -1 and who in lib.h3d_last_error() and b"does not fit int32" in lib.h3d_last_error()
    assert emit(p, 4, 4, 4, V=0) == -1 and b"V=0" in lib.h3d_last_error()
    assert emit(p, 4, 4, 4, V=7 * 64 + 1) == -1 and b"V=" in lib.h3d_last_error()
    assert emit(p, 4, 4, 4, T=12 * 27 + 1) == -1 and b"T=" in lib.h3d_last_error()


def test_cpu_tensor_is_refused():
    import torch
    iso = importlib.import_module("3dhumangan_amd.lib.components.isosurface")
    h3dlib = importlib.import_module("3dhumangan_amd._lib")
    with pytest.raises(h3dlib.H3DError):
        iso.marching_tetrahedra(torch.zeros(4, 4, 4), 0.5)
