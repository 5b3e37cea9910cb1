"""A numpy restatement of quadric vertex clustering (include/h3d.h, h3d_mesh_cluster_cells / _faces / _solve, steps 1 - 5), written
from the text, not from the kernels, and sharing no code with the product.

    simplify(vertices, faces, cell, origin, counts, regularization=1e-2, reach=1.0, dtype=float64, placement="quadric")
        -> dict(vertices [C,3] dtype, faces int64 [T',3], cluster int64 [V], cells int64 [C])

The cell of a vertex is always the fp32 arithmetic of step 1, whatever `dtype` is, and so is the cell centre: the two number formats
cluster alike and differ in the sums and the solve alone.  placement="mean" puts every cluster at the mean of its vertices (plain
vertex clustering): what the quadric is compared with.  The sums run in ascending vertex id and ascending record id (np.add.at), the
solve is numpy's LU -- neither is the kernel's order or method.

For the tests: the meshes (marching tetrahedra of tests/_isosurface_reference.py on a sphere and on a rotated box) and the invariants.
"""
import numpy as np

import _isosurface_reference as ISO

f32, f64 = np.float32, np.float64


def grid_of(lo, hi, cell):
    """-> (origin, counts): counts = floor((hi - lo) / cell) + 1 per axis"""
    lo, hi = np.asarray(lo, dtype=f64), np.asarray(hi, dtype=f64)
    return tuple(float(v) for v in lo), tuple(int(n) for n in np.floor((hi - lo) / float(cell)).astype(np.int64) + 1)


def cell_indices(vertices, origin, cell, counts):
    """step 1 -> int64 [V,3]: one fp32 subtraction, one fp32 multiplication by the fp32 quotient 1 / cell, floor, clamp"""
    v = np.asarray(vertices).astype(f32)
    inv_cell = f32(1.0) / f32(cell)
    with np.errstate(all="ignore"):
        g = np.floor((v - np.asarray(origin, dtype=f32)) * inv_cell)
    assert g.dtype == f32
    top = np.asarray(counts, dtype=f64) - 1.0
    g = np.where(np.isfinite(v), np.clip(np.nan_to_num(g.astype(f64), nan=0.0, posinf=np.inf, neginf=-np.inf), 0.0, top), 0.0)
    return g.astype(np.int64)


def simplify(vertices, faces, cell, origin, counts, regularization=1e-2, reach=1.0, dtype=f64, placement="quadric"):
    assert placement in ("quadric", "mean") and dtype in (f32, f64)
    v32 = np.asarray(vertices).astype(f32).reshape(-1, 3)
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    V, T = len(v32), len(faces)
    nx, ny, nz = (int(n) for n in counts)
    assert nx * ny * nz < 2 ** 31 and 3 * T < 2 ** 31
    cell32 = f32(cell)
    if V == 0:
        return dict(vertices=np.zeros((0, 3), dtype), faces=np.zeros((0, 3), np.int64), cluster=np.zeros(0, np.int64),
                    cells=np.zeros(0, np.int64))
    # 1, 2: cells and clusters
    idx = cell_indices(v32, origin, cell32, counts)
    ids = (idx[:, 0] * ny + idx[:, 1]) * nz + idx[:, 2]
    cells, cluster = np.unique(ids, return_inverse=True)
    cluster = cluster.reshape(-1)
    C = len(cells)
    ijk = np.stack([cells // (ny * nz), (cells // nz) % ny, cells % nz], axis=1)
    centre32 = np.asarray(origin, dtype=f32) + (ijk.astype(f32) + f32(0.5)) * cell32          # fp32, product rounded before the sum
    assert centre32.dtype == f32
    centre, v = centre32.astype(dtype), v32.astype(dtype)
    # 3: mean and quadric, local to the cell centre
    with np.errstate(all="ignore"):
        total, count = np.zeros((C, 3), dtype), np.zeros(C, dtype)
        np.add.at(total, cluster, v - centre[cluster])
        np.add.at(count, cluster, dtype(1))
        mean = total / count[:, None]
        A, b = np.zeros((C, 3, 3), dtype), np.zeros((C, 3), dtype)
        if T and placement == "quadric":
            fc = np.clip(faces, 0, V - 1)
            owner = cluster[fc].reshape(-1)                                  # record 3 t + k belongs to the cluster of corner k
            corner = lambda j: v[np.repeat(fc[:, j], 3)] - centre[owner]    # noqa: E731  the face's j-th vertex, local to the record's cluster
            p0, p1, p2 = corner(0), corner(1), corner(2)
            m = np.cross(p1 - p0, p2 - p0).astype(dtype)
            length = np.sqrt((m * m).sum(axis=1))
            ok = (length > 0) & np.isfinite(length)
            m, p0, own, w = m[ok], p0[ok], owner[ok], (dtype(1) / (dtype(2) * length[ok]))
            wm = w[:, None] * m
            np.add.at(A, own, wm[:, :, None] * m[:, None, :])
            np.add.at(b, own, wm * (-(m * p0).sum(axis=1))[:, None])
        # 4: the representative
        x = mean.copy()
        trace = A[:, 0, 0] + A[:, 1, 1] + A[:, 2, 2]
        solve = (trace > 0) & np.isfinite(A).all(axis=(1, 2)) & np.isfinite(b).all(axis=1) & np.isfinite(mean).all(axis=1)
        x[(trace > 0) & ~solve] = np.nan
        if solve.any():
            M = A[solve] + (dtype(regularization) * trace[solve])[:, None, None] * np.eye(3, dtype=dtype)
            rhs = np.einsum("cij,cj->ci", A[solve], mean[solve]) + b[solve]
            x[solve] = mean[solve] - np.linalg.solve(M, rhs[..., None])[..., 0].astype(dtype)
        x[np.isnan(x).any(axis=1)] = 0
        r = dtype(reach) * dtype(cell32)
        out = centre + np.clip(x, -r, r)
    assert out.dtype == dtype
    # 5: faces
    mapped = cluster[np.clip(faces, 0, V - 1)] if T else np.zeros((0, 3), np.int64)
    keep = (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & (mapped[:, 0] != mapped[:, 2])
    return dict(vertices=out, faces=mapped[keep], cluster=cluster, cells=cells)


# ------------------------------------------------------------------------------------------------------------------ meshes
_MESHES = {}
BOX_HALF, BOX_NODES = 9.7, 32


def sphere_mesh(nodes, radius):
    """marching tetrahedra of the sphere field of tests/_isosurface_reference.py in a nodes^3 grid -> (vertices fp32, faces int32)"""
    key = ("sphere", nodes, radius)
    if key not in _MESHES:
        v, f, _ = ISO.marching_tetrahedra(ISO.sphere((nodes,) * 3, radius), 0.0)
        _MESHES[key] = (v.astype(f32), f.astype(np.int32))
    return _MESHES[key]


def box_frame():
    """-> (Q, c): the box is |Q (x - c)|_inf <= BOX_HALF: the axis-aligned box turned by 0.5 about x, then by 0.3 about z, about the
    centre that ISO.sphere uses (the grid's, moved by (0.13, 0.21, -0.17)); Q is the inverse of that turn"""
    cz, sz, cx, sx = np.cos(0.3), np.sin(0.3), np.cos(0.5), np.sin(0.5)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    Rx = np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return (Rz @ Rx).T, (BOX_NODES - 1) / 2.0 + np.array([0.13, 0.21, -0.17])


def box_mesh():
    """the iso-surface of half - max |R (x - c)| at level 0 in a 32^3 grid: flat sides, sharp edges and corners, none along the grid"""
    if "box" not in _MESHES:
        R, c = box_frame()
        x = np.stack(np.meshgrid(*(np.arange(BOX_NODES, dtype=f64),) * 3, indexing="ij"), axis=-1)
        field = (BOX_HALF - np.abs((x - c) @ R.T).max(axis=-1)).astype(f32)
        v, f, _ = ISO.marching_tetrahedra(field, 0.0)
        _MESHES["box"] = (v.astype(f32), f.astype(np.int32))
    return _MESHES["box"]


def box_distance(points):
    """distance of every point to the surface of the true box"""
    R, c = box_frame()
    y = np.abs((np.asarray(points, dtype=f64) - c) @ R.T)
    outside = np.sqrt((np.maximum(y - BOX_HALF, 0.0) ** 2).sum(axis=1))
    return np.where(outside > 0, outside, BOX_HALF - y.max(axis=1))


def fan(n_faces, radius=3.0):
    """Two fans of triangles around two hubs that share one cell (cell edge 1, grid origin 0; the cell (4, 4, 4)), n_faces triangles
    together -> (vertices fp32, faces int32).  Vertex 0 is the first hub, with the first n_faces - n_faces // 2 faces; the second hub
    (with n_faces = 1: a vertex that no face names) has the other n_faces // 2.  Both fans are gently waved discs across the z axis
    (tilted by 20 degrees at the most), the hubs lie 0.7 apart along it, the rims `radius` away in other cells.  The cell's cluster
    has two vertices and exactly n_faces corner records, record k of its segment being face k.  The planes of one fan meet in its hub,
    the representative lies between the two hubs, on the same side of every plane of a fan: each record pulls it the same way, and
    none can be lost without moving it -- tests/test_mesh_simplify_cpu.py takes every record away in turn and sees the cluster
    move by more than the bar of tests/test_gpu_mesh_simplify.py."""
    second = n_faces // 2
    first = n_faces - second
    centre = np.array([4.5, 4.5, 4.5])
    hubs = np.array([[0.1, -0.1, -0.35], [-0.1, 0.15, 0.35]])

    def ring(n, phase):
        k = np.arange(n + 1, dtype=f64)
        angle = 2 * np.pi * 0.9 * k / (n + 1) + phase
        return np.stack([radius * np.cos(angle), radius * np.sin(angle), 0.5 * np.sin(2 * angle)], axis=1)

    around = lambda hub, n: np.stack([np.full(n, hub, np.int64), hub + np.arange(1, n + 1), hub + np.arange(2, n + 2)], axis=1)  # noqa: E731
    vertices, faces = [hubs[0:1], ring(first, 0.0) + hubs[0], hubs[1:2]], [around(0, first)]
    if second:
        vertices.append(ring(second, 1.0) + hubs[1])
        faces.append(around(first + 2, second))
    return (np.concatenate(vertices) + centre).astype(f32), np.concatenate(faces).astype(np.int32)


def edge_balance(faces):
    """for every directed edge (a, b): as many a -> b as b -> a"""
    f = np.asarray(faces).astype(np.int64)
    if len(f) == 0:
        return True
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    top = int(d.max()) + 1
    forward, back = d[:, 0] * top + d[:, 1], d[:, 1] * top + d[:, 0]
    keys, counts = np.unique(forward, return_counts=True)
    keys_b, counts_b = np.unique(back, return_counts=True)
    return bool(np.array_equal(keys, keys_b) and np.array_equal(counts, counts_b))
