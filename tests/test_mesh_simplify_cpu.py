"""Quadric vertex clustering without a GPU: the properties of the definition (include/h3d.h, h3d_mesh_cluster_*) on its numpy
restatement (tests/_mesh_simplify_reference.py) -- what the stage is for, what it keeps, its order contracts and edge cases -- and the
refusals of lib/components/mesh_simplify.py and of the library, none of which touches a device.

Measured with the float64 restatement (printed by the tests, quoted in DESIGN 4.5g):
    sphere r = 16 in 40^3, 28 868 faces      cell 2      3      4      6
        faces left                            2 420  1 056    584    264        (11.9 x, 27.3 x, 49.4 x, 109 x)
        enclosed volume / original           0.9975 0.9938 0.9883 0.9734
    sphere r = 27 in 64^3, 82 240 faces, cell 4: 1 704 faces, volume 0.9961
    rotated box in 32^3, 19 776 faces: rms distance of the referenced output vertices to the true box
        cell 3: quadric 0.0399, mean 0.1452 (3.64 x);  cell 4: quadric 0.0395, mean 0.1886 (4.77 x)
"""
import importlib
import os
import re
import warnings

import numpy as np
import pytest
import torch

import _isosurface_reference as ISO
import _mesh_simplify_reference as R

mesh_simplify = importlib.import_module("3dhumangan_amd.lib.components.mesh_simplify")
mesh_texture = importlib.import_module("3dhumangan_amd.lib.components.mesh_texture")
_lib = importlib.import_module("3dhumangan_amd._lib")
f32, f64 = np.float32, np.float64
SPHERE = (40, 16.0)
# the enclosed volume that the float64 restatement itself keeps on the sphere (r = 16 in 40^3), rounded down at the fourth digit: a
# chord mesh of a convex body lies inside it, and the coarser the cells the more is cut off
VOLUME_KEPT = {2: 0.9974, 3: 0.9937, 4: 0.9882, 6: 0.9734}


def on_grid(mesh, nodes, cell, **kwargs):
    """the restatement on the grid that covers nodes^3 unit voxels from the origin"""
    origin, counts = R.grid_of((0, 0, 0), (nodes - 1,) * 3, cell)
    return R.simplify(mesh[0], mesh[1], cell, origin, counts, **kwargs)


@pytest.mark.parametrize("cell", [2, 3, 4, 6])
def test_a_closed_sphere_keeps_its_edge_balance_and_its_volume(cell):
    v, f = R.sphere_mesh(*SPHERE)
    assert ISO.is_closed_and_oriented(len(v), f) and R.edge_balance(f)
    out = on_grid((v, f), SPHERE[0], cell)
    kept = ISO.signed_volume(out["vertices"], out["faces"]) / ISO.signed_volume(v, f)
    print(f"sphere cell {cell}: {len(f)} -> {len(out['faces'])} faces ({len(f) / len(out['faces']):.1f} x), volume kept {kept:.4f}")
    assert len(out["faces"]) > 0 and R.edge_balance(out["faces"])
    assert VOLUME_KEPT[cell] <= kept <= 1.0


@pytest.mark.parametrize("cell", [3, 4])
def test_merging_equal_faces_would_break_the_edge_balance(cell):
    """two closed shells 0.6 voxels apart: where both fall into the same cells their faces come out twice, equal index for index and
    in the same sense; elsewhere they stay apart.  As it is the output is balanced; with the equal faces merged (one of each kept) it
    is not, and neither with one single face of one equal pair taken away."""
    inner, outer = R.sphere_mesh(*SPHERE), R.sphere_mesh(SPHERE[0], SPHERE[1] + 0.6)
    v, f = np.concatenate([inner[0], outer[0]]), np.concatenate([inner[1], outer[1] + len(inner[0])])
    assert R.edge_balance(f)
    faces = on_grid((v, f), SPHERE[0], cell)["faces"]
    merged, first, count = np.unique(ISO.canonical(faces), axis=0, return_index=True, return_counts=True)
    print(f"two shells cell {cell}: {len(faces)} faces, {int((count > 1).sum())} of {len(merged)} distinct faces occur more than once")
    assert (count > 1).sum() >= len(merged) // 4 and (count == 1).sum() >= len(merged) // 4
    assert R.edge_balance(faces)
    assert not R.edge_balance(merged)
    assert not R.edge_balance(np.delete(faces, first[count > 1][0], axis=0))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_the_fan_cluster_needs_every_one_of_its_records(n):
    """the fan cases of tests/test_gpu_mesh_simplify.py are there for the lane stride and the butterfly of the solve kernel: they
    can see a lost or doubled record only if the cluster's position depends on each.  Every record of the hubs' cluster is taken
    away in turn, and doubled in turn: the cluster moves by more than the bar those cases are held to (8 x the float32 - float64
    gap of the rotated box at cell 4, as that file computes it: 6.9e-4).  Measured: lost 3.5e-1 (1 record), at least 1.3e-2 (63),
    1.6e-2 (64), 1.3e-2 (65), 6.6e-3 (129); doubled at least 1.3e-2, 1.5e-2, 1.2e-2, 6.4e-3."""
    box, (origin, counts) = R.box_mesh(), R.grid_of((0, 0, 0), (R.BOX_NODES - 1,) * 3, 4.0)
    low, high = (R.simplify(box[0], box[1], 4.0, origin, counts, dtype=dtype)["vertices"].astype(f64) for dtype in (f32, f64))
    bar = max(8.0 * float(np.abs(low - high).max()), 4.0 * 2.0 ** -23 * float(np.abs(high).max()))
    v, f = R.fan(n)
    grid = (1.0, (0.0, 0.0, 0.0), (9, 9, 9))
    full = R.simplify(v, f, *grid)
    hub = full["cluster"][0]
    assert (full["cluster"] == hub).sum() == 2 and (full["cluster"][f] == hub).sum() == n
    assert np.array_equal(np.flatnonzero((full["cluster"][f] == hub).reshape(-1)), 3 * np.arange(n))      # record k of the segment is face k
    moved = lambda faces: float(np.abs(R.simplify(v, faces, *grid)["vertices"][hub] - full["vertices"][hub]).max())     # noqa: E731
    lost = [moved(np.delete(f, k, axis=0)) for k in range(n)]
    twice = [moved(np.concatenate([f, f[k:k + 1]])) for k in range(n)]
    print(f"fan {n}: bar {bar:.2e}; one record lost moves the cluster by {min(lost):.2e} .. {max(lost):.2e}, doubled by {min(twice):.2e} .. {max(twice):.2e}")
    assert min(lost) > bar
    if n > 1:                                                # one record alone: doubling it scales A, b and the trace alike, x stays
        assert min(twice) > bar
    else:
        assert max(twice) == 0.0


@pytest.mark.parametrize("name,cell,reach", [("sphere", 2, 1.0), ("sphere", 4, 1.0), ("sphere", 3.5, 0.5), ("box", 3, 1.0), ("box", 4, 0.75)])
def test_no_vertex_moves_further_than_the_bound(name, cell, reach):
    mesh, nodes = (R.sphere_mesh(*SPHERE), SPHERE[0]) if name == "sphere" else (R.box_mesh(), R.BOX_NODES)
    for dtype in (f64, f32):
        out = on_grid(mesh, nodes, cell, reach=reach, dtype=dtype)
        moved = np.abs(out["vertices"][out["cluster"]].astype(f64) - mesh[0]).max()
        print(f"{name} cell {cell} reach {reach} {dtype.__name__}: moved {moved:.3f}, bound {(reach + 0.5) * cell:.3f}")
        assert moved <= (reach + 0.5) * cell * (1 + 2.0 ** -20)


@pytest.mark.parametrize("cell", [3, 4])
def test_quadric_placement_keeps_the_edges_that_the_mean_rounds_off(cell):
    """what the stage is for: on a box that is turned against the grid the quadric's vertices lie 2.5 x closer (rms) to the true
    surface than the means of the same clusters"""
    mesh = R.box_mesh()
    assert len(mesh[1]) == 19776
    rms = {}
    for placement in ("quadric", "mean"):
        out = on_grid(mesh, R.BOX_NODES, cell, placement=placement)
        used = np.unique(out["faces"])
        rms[placement] = float(np.sqrt((R.box_distance(out["vertices"][used]) ** 2).mean()))
    print(f"box cell {cell}: rms distance quadric {rms['quadric']:.4f}, mean {rms['mean']:.4f}, ratio {rms['mean'] / rms['quadric']:.2f}")
    assert rms["mean"] >= 2.5 * rms["quadric"]


def test_reduction_and_the_atlas_cell():
    v, f = R.sphere_mesh(*SPHERE)
    out = on_grid((v, f), SPHERE[0], 4)
    T, T1 = len(f), len(out["faces"])
    before, after = mesh_texture.atlas_layout(T, 2048)[0], mesh_texture.atlas_layout(T1, 2048)[0]
    print(f"sphere cell 4: {T} -> {T1} faces ({T / T1:.1f} x); atlas cell at 2048: {before} -> {after} texels")
    assert T >= 30 * T1
    assert after > before
    # the surface of DESIGN 4.5c: the cell that the issue starts from
    assert mesh_texture.atlas_layout(501_000, 2048)[0] == 4 and mesh_texture.atlas_layout(501_000, 8192)[0] == 16


def test_order_contracts():
    v, f = R.box_mesh()
    out = on_grid((v, f), R.BOX_NODES, 4)
    cells, cluster = out["cells"], out["cluster"]
    assert (np.diff(cells) > 0).all() and cluster.min() == 0 and cluster.max() == len(cells) - 1
    origin, counts = R.grid_of((0, 0, 0), (R.BOX_NODES - 1,) * 3, 4)
    idx = R.cell_indices(v, origin, 4, counts)
    assert np.array_equal(cells[cluster], (idx[:, 0] * counts[1] + idx[:, 1]) * counts[2] + idx[:, 2])
    mapped = cluster[f]
    keep = (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & (mapped[:, 0] != mapped[:, 2])
    assert np.array_equal(out["faces"], mapped[keep]) and 0 < keep.sum() < len(f)        # input order, corner order
    # the float32 restatement clusters as the float64 one does
    low = on_grid((v, f), R.BOX_NODES, 4, dtype=f32)
    assert all(np.array_equal(low[k], out[k]) for k in ("cells", "cluster", "faces")) and low["vertices"].dtype == f32


def test_edge_cases():
    v, f = R.sphere_mesh(24, 9.0)
    # one cell holds the whole mesh
    one = R.simplify(v, f, 100.0, (0, 0, 0), (1, 1, 1))
    assert one["vertices"].shape == (1, 3) and one["faces"].shape == (0, 3) and (one["cluster"] == 0).all()
    assert np.abs(one["vertices"][0] - 50.0).max() <= 100.0           # clamped to reach = 1 cell around the centre (50, 50, 50)
    # no vertices, no faces
    assert R.simplify(np.zeros((0, 3)), np.zeros((0, 3)), 1.0, (0, 0, 0), (2, 2, 2))["vertices"].shape == (0, 3)
    lonely = R.simplify(np.array([[0.25, 1.5, 0.75]]), np.zeros((0, 3)), 1.0, (0, 0, 0), (2, 2, 2))
    assert np.array_equal(lonely["cells"], [2]) and np.allclose(lonely["vertices"], [[0.25, 1.5, 0.75]])
    # a cluster whose faces all have zero area falls back to the mean of its vertices
    flat_v = np.array([[0.2, 0.2, 0.2], [0.6, 0.4, 0.2], [2.5, 0.5, 0.5], [0.5, 2.5, 0.5]], dtype=f32)
    flat_f = np.array([[0, 1, 1], [0, 0, 2], [2, 3, 3]])
    flat = R.simplify(flat_v, flat_f, 1.0, (0, 0, 0), (3, 3, 3))
    assert np.allclose(flat["vertices"][flat["cluster"][0]], flat_v[:2].astype(f64).mean(axis=0)) and len(flat["faces"]) == 0
    # a NaN vertex goes to cell 0 and every output is finite; clusters without it or its faces keep their bits
    base = on_grid((v, f), 24, 3)
    poisoned = v.copy()
    victim = int(f[100, 0])
    poisoned[victim, 1] = np.nan                                      # one coordinate: index 0 on that axis alone
    origin, counts = R.grid_of((0, 0, 0), (23, 23, 23), 3)
    assert np.array_equal(R.cell_indices(poisoned[victim], origin, 3, counts), R.cell_indices(v[victim], origin, 3, counts) * [1, 0, 1])
    poisoned[victim] = [np.nan, np.inf, -np.inf]
    out = on_grid((poisoned, f), 24, 3)
    assert base["cells"][0] > 0                                       # the NaN opens cell 0: every other cluster moves up by one
    assert out["cells"][0] == 0 and out["cluster"][victim] == 0 and np.isfinite(out["vertices"]).all()
    assert np.array_equal(out["vertices"][0], [1.5, 1.5, 1.5])        # the cluster that holds it: its cell centre
    touched = np.unique(base["cluster"][f[(f == victim).any(axis=1)]])
    same = np.setdiff1d(np.arange(len(base["cells"])), touched)
    assert len(same) > len(base["cells"]) // 2 and np.array_equal(out["vertices"][1:][same], base["vertices"][same])
    # out-of-range face indices are clamped
    wrong = f.astype(np.int64).copy()
    wrong[7] = [-5, 2 ** 31 - 1, 10 ** 6]
    clamped = wrong.copy()
    clamped[7] = [0, len(v) - 1, len(v) - 1]
    a, b = on_grid((v, wrong), 24, 3), on_grid((v, clamped), 24, 3)
    assert np.isfinite(a["vertices"]).all() and np.array_equal(a["vertices"], b["vertices"]) and np.array_equal(a["faces"], b["faces"])
    # the last cell is ragged on every axis: the grid of cell 3.5 over 24 nodes has 7 cells of which the last is cut
    origin, counts = R.grid_of((0, 0, 0), (23, 23, 23), 3.5)
    assert counts == (7, 7, 7) and 7 * 3.5 > 23


def test_cluster_grid_is_the_restatement():
    for lo, hi, cell in (((0, 0, 0), (39, 39, 39), 4), ((-1.5, 0.25, 3), (2.5, 0.25, 10.1), 0.7), ((0, 0, 0), (23, 23, 23), 3.5)):
        origin, counts = mesh_simplify.cluster_grid(lo, hi, cell)
        assert (origin, counts) == R.grid_of(lo, hi, cell)
    for lo, hi, cell, said in (((0, 0, 0), (1, 1, 1), 0.0, "cell=0.0"), ((0, 0, 0), (1, 1, 1), float("nan"), "cell=nan"),
                               ((0, 0, 0), (1, float("inf"), 1), 1.0, "must be finite"), ((0, 2, 0), (1, 1, 1), 1.0, "lo <= hi"),
                               ((0, 0), (1, 1, 1), 1.0, "three numbers")):
        with pytest.raises(ValueError, match=said):
            mesh_simplify.cluster_grid(lo, hi, cell)


def test_simplify_refuses_by_name_before_any_device_call():
    V, T = 9, 4
    good = dict(vertices=torch.zeros(V, 3), faces=torch.zeros(T, 3, dtype=torch.int32), cell=1.0, origin=(0, 0, 0), counts=(2, 2, 2))

    def refused(said, error=ValueError, **change):
        with pytest.raises(error, match=said):
            mesh_simplify.simplify(**dict(good, **change))

    refused("vertices must be a tensor", TypeError, vertices=np.zeros((V, 3), f32))
    refused("vertices must be float32", vertices=torch.zeros(V, 3, dtype=torch.float64))
    refused("vertices must be float32", vertices=torch.zeros(V, 4))
    refused("faces must be int32", faces=torch.zeros(T, 3, dtype=torch.int64))
    refused("faces must be int32", faces=torch.zeros(T, 2, dtype=torch.int32))
    refused("triangles without a vertex", vertices=torch.zeros(0, 3))
    refused("cell=0 must be positive", cell=0)
    refused("cell=-2.0 must be positive", cell=-2.0)
    refused("cell=nan must be positive", cell=float("nan"))
    refused("cell=inf must be positive", cell=float("inf"))
    refused("cell=1e-60 must be positive", cell=1e-60)             # zero in float32
    with warnings.catch_warnings():
        warnings.simplefilter("error")                             # infinite in float32: the named refusal, no numpy warning in front of it
        refused("cell=1e\\+60 must be positive", cell=1e60)
    refused("1 / cell is not finite", cell=1e-42)                 # a float32 denormal
    refused("regularization=0.0 must be positive", regularization=0.0)
    refused("regularization=nan must be positive", regularization=float("nan"))
    refused("reach=0.49 must be at least 0.5", reach=0.49)
    refused("reach=nan must be at least 0.5", reach=float("nan"))
    refused("origin and counts go together", counts=None)
    refused("origin and counts go together", origin=None)
    refused("origin must be three finite numbers", origin=(0, float("inf"), 0))
    refused("counts must be three positive integers", counts=(2, 0, 2))
    refused("counts must be three positive integers", counts=(2, 2.5, 2))
    refused("2048 x 1024 x 1024 has 2\\^31 cells or more", counts=(2048, 1024, 1024))
    refused("3 T must stay below 2\\^31", faces=torch.empty(715827883, 3, dtype=torch.int32, device="meta"))
    refused("ROCm device only", _lib.H3DError)                    # every argument is fine: the CPU tensors are what is refused
    refused("ROCm device only", _lib.H3DError, counts=(2047, 1024, 1024), reach=0.5, regularization=1e-9)


def test_the_library_declares_and_refuses():
    """the three entry points: header arity equals _SIGNATURES arity; their own checks run before any device call"""
    import ctypes as C
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "h3d.h")).read(), flags=re.S)
    for name, arity in (("h3d_mesh_cluster_cells", 9), ("h3d_mesh_cluster_faces", 8), ("h3d_mesh_cluster_solve", 19)):
        declared = re.search(name + r"\s*\(([^)]*)\)", header).group(1).split(",")
        assert len(declared) == len(_lib._SIGNATURES[name][1]) == arity
    origin = (C.c_float * 3)(0.0, 0.0, 0.0)
    said = lambda rc: (rc, lib.h3d_last_error().decode())         # noqa: E731

    def cells(V=4, origin=origin, inv_cell=1.0, counts=(2, 2, 2)):
        return said(lib.h3d_mesh_cluster_cells(None, V, origin, inv_cell, *counts, None, None))

    def faces(T=4, V=4):
        return said(lib.h3d_mesh_cluster_faces(None, T, None, V, None, None, None, None))

    def solve(V=4, T=4, n=2, origin=origin, cell=1.0, counts=(2, 2, 2), regularization=1e-2, reach=1.0):
        return said(lib.h3d_mesh_cluster_solve(None, V, None, T, None, None, None, None, None, n, origin, cell, *counts, regularization,
                                               reach, None, None))

    bad_origin = (C.c_float * 3)(0.0, float("nan"), 0.0)
    for call, kwargs, message in ((cells, dict(inv_cell=0.0), "inv_cell=0 must be positive"), (cells, dict(counts=(2, 0, 2)), "must be positive"),
                                  (cells, dict(counts=(2048, 1024, 1024)), "2^31 cells or more"), (cells, dict(V=-1), "V=-1 out of range"),
                                  (cells, dict(V=2 ** 31), "out of range"), (cells, dict(origin=bad_origin), "origin must be finite"),
                                  (cells, dict(origin=None), "null pointer"), (cells, dict(), "null pointer"),
                                  (faces, dict(T=715827883), "3 T must stay below 2^31"), (faces, dict(V=0), "4 triangles without a vertex"),
                                  (faces, dict(), "null pointer"),
                                  (solve, dict(cell=float("inf")), "cell=inf must be positive"), (solve, dict(regularization=0.0), "regularization=0"),
                                  (solve, dict(reach=0.25), "reach=0.25 must be at least 0.5"), (solve, dict(n=5), "C=5 clusters of V=4"),
                                  (solve, dict(T=715827883), "3 T must stay below 2^31"), (solve, dict(counts=(65536, 65536, 1)), "2^31 cells"),
                                  (solve, dict(), "null pointer")):
        rc, text = call(**kwargs)
        assert rc == -1 and message in text, (call.__name__, kwargs, rc, text)
    assert cells(V=0)[0] == 0 and faces(T=0)[0] == 0 and solve(n=0)[0] == 0          # nothing to do: nothing is launched
