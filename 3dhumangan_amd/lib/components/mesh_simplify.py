"""Fewer triangles for a mesh, on the device: quadric vertex clustering on a uniform grid (csrc/mesh_simplify.hip; the definition --
cells, cluster order, quadric, representative, kept faces -- is in include/h3d.h, h3d_mesh_cluster_cells / _faces / _solve).

    cluster_grid(lo, hi, cell) -> (origin (3 floats), counts (nx, ny, nz))
    simplify(vertices, faces, cell, origin=None, counts=None, regularization=1e-2, reach=1.0)
        -> (vertices fp32 [C,3], faces int32 [T',3], cluster int32 [V]); return_cells=True adds the cell table int32 [C]

Every non-empty grid cell becomes one vertex, placed where the planes of the cluster's triangles meet (pulled towards the cluster's
mean by `regularization`, kept within `reach` cells of the cell centre); a triangle survives iff its corners fall into three different
cells.  Three launches; between them two stable sorts (the cell ids, the 3T corner keys), unique_consecutive for the cluster table,
prefix sums for the segment offsets and a boolean mask for the kept faces are torch's.  Host reads: the number of clusters C and of
kept faces T', and the bounding box when no grid is given.  Nothing is carried across: normals, colours, texture and rig are
evaluated at whatever vertices they are given (isosurface.vertex_normals, mesh_color, mesh_texture, mesh_rig).
"""
import ctypes as C
import math

import numpy as np
import torch

from ... import _lib

INT32_END = 2 ** 31


def cluster_grid(lo, hi, cell):
    """The cluster grid that covers the box lo..hi with cubic cells of edge `cell` -> (origin = lo as 3 floats, counts = floor((hi -
    lo) / cell) + 1 per axis); ValueError where the box or the cell is not finite, hi < lo, or cell <= 0."""
    lo, hi, cell = [float(v) for v in lo], [float(v) for v in hi], float(cell)
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("cluster_grid: lo and hi take three numbers each")
    if not 0.0 < cell < math.inf:
        raise ValueError(f"cluster_grid: cell={cell} must be positive and finite")
    if not all(math.isfinite(a) and math.isfinite(b) and a <= b for a, b in zip(lo, hi)):
        raise ValueError(f"cluster_grid: the box {tuple(lo)} .. {tuple(hi)} must be finite with lo <= hi")
    return tuple(lo), tuple(int(math.floor((b - a) / cell)) + 1 for a, b in zip(lo, hi))


def _check_grid(origin, counts):
    origin = [float(v) for v in origin]
    if len(origin) != 3 or not all(math.isfinite(v) for v in origin):
        raise ValueError(f"simplify: origin must be three finite numbers, got {tuple(origin)}")
    if len(counts) != 3 or any(int(n) != n or int(n) < 1 for n in counts):
        raise ValueError(f"simplify: counts must be three positive integers, got {tuple(counts)}")
    counts = [int(n) for n in counts]
    if counts[0] * counts[1] * counts[2] >= INT32_END:
        raise ValueError(f"simplify: the cluster grid {counts[0]} x {counts[1]} x {counts[2]} has 2^31 cells or more (cell ids are "
                         "int32): take a larger cell")
    return origin, counts


def simplify(vertices, faces, cell, origin=None, counts=None, regularization=1e-2, reach=1.0, return_cells=False):
    """vertices fp32 [V,3], faces int32 [T,3] on the current ROCm device (non-contiguous views are copied); cell: the edge of a cluster
    cell; origin (3 numbers) and counts (nx, ny, nz): the cluster grid, both or neither -- without them the grid of cluster_grid over
    the box of the finite vertices (one more host read).  -> (vertices [C,3], faces [T',3], cluster [V]: the output vertex that stands
    for each input vertex); return_cells: a fourth entry, int32 [C], the grid cell of every output vertex (ascending).

    Output vertex c stands for the c-th non-empty cell in ascending cell id; the kept faces stay in their input order with their
    orientation; equal faces are not merged and a vertex no kept face names stays.  Face indices outside [0, V) are clamped on the
    device.  V = 0 gives three empty tensors; T = 0 clusters the vertices to their means."""
    for name, t in (("vertices", vertices), ("faces", faces)):
        if not torch.is_tensor(t):
            raise TypeError(f"simplify: {name} must be a tensor, got {type(t).__name__}")
    if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"simplify: vertices must be float32 [V,3], got {vertices.dtype} {tuple(vertices.shape)}")
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"simplify: faces must be int32 [T,3], got {faces.dtype} {tuple(faces.shape)}")
    V, T = vertices.shape[0], faces.shape[0]
    if V >= INT32_END:
        raise ValueError(f"simplify: V={V} vertices: 2^31 or more (vertex ids are int32)")
    if 3 * T >= INT32_END:
        raise ValueError(f"simplify: T={T} triangles: 3 T must stay below 2^31 (corner records are int32)")
    if T > 0 and V == 0:
        raise ValueError(f"simplify: {T} triangles without a vertex")
    with np.errstate(over="ignore", under="ignore"):
        cell32 = np.float32(cell)
        inv_cell = np.float32(1.0) / cell32 if cell32 > 0 else np.float32(0.0)       # the one division, in fp32, on the host
    if not (math.isfinite(float(cell)) and float(cell) > 0.0 and 0.0 < float(cell32) < math.inf):
        raise ValueError(f"simplify: cell={cell} must be positive and finite (in float32)")
    if not 0.0 < float(inv_cell) < math.inf:
        raise ValueError(f"simplify: cell={cell} is too small: 1 / cell is not finite in float32")
    regularization, reach = float(regularization), float(reach)
    if not 0.0 < regularization < math.inf:
        raise ValueError(f"simplify: regularization={regularization} must be positive")
    if not 0.5 <= reach < math.inf:
        raise ValueError(f"simplify: reach={reach} must be at least 0.5 (half a cell: the cell itself)")
    if (origin is None) != (counts is None):
        raise ValueError("simplify: origin and counts go together (both, or neither for the vertices' own box)")
    if origin is not None:
        origin, counts = _check_grid(origin, counts)
    _lib.need_cuda(vertices, faces)
    dev, lib = vertices.device, _lib.load()
    empty = lambda *shape, dtype=torch.int32: torch.empty(*shape, dtype=dtype, device=dev)           # noqa: E731
    if V == 0:
        out = (empty(0, 3, dtype=torch.float32), empty(0, 3), empty(0))
        return out + (empty(0),) if return_cells else out
    vertices, faces = vertices.contiguous(), faces.contiguous()
    if origin is None:
        finite = torch.isfinite(vertices)
        lo = torch.where(finite, vertices, torch.full_like(vertices, math.inf)).amin(dim=0)
        hi = torch.where(finite, vertices, torch.full_like(vertices, -math.inf)).amax(dim=0)
        lo, hi = torch.stack([lo, hi]).double().tolist()     # the box: one host read
        lo, hi = zip(*((a, b) if a <= b else (0.0, 0.0) for a, b in zip(lo, hi)))      # an axis without a finite coordinate
        origin, counts = _check_grid(*cluster_grid(lo, hi, float(cell32)))
    origin32 = (C.c_float * 3)(*origin)
    stream = _lib.stream_handle()

    cells = empty(V)
    _lib.check(lib.h3d_mesh_cluster_cells(_lib.ptr(vertices), V, origin32, float(inv_cell), *counts, _lib.ptr(cells), stream),
               "h3d_mesh_cluster_cells")
    sorted_cells, vertex_order = torch.sort(cells, stable=True)
    table, inverse, per_cluster = torch.unique_consecutive(sorted_cells, return_inverse=True, return_counts=True)
    n_clusters = table.shape[0]                              # host read: C
    cluster = empty(V)
    cluster[vertex_order] = inverse.to(torch.int32)          # a permutation: every slot written once
    vertex_offsets = torch.zeros(n_clusters + 1, dtype=torch.int64, device=dev)
    torch.cumsum(per_cluster, 0, out=vertex_offsets[1:])

    if T > 0:
        mapped, keep, keys = empty(T, 3), empty(T, dtype=torch.bool), empty(3 * T)
        _lib.check(lib.h3d_mesh_cluster_faces(_lib.ptr(faces), T, _lib.ptr(cluster), V, _lib.ptr(mapped), _lib.ptr(keep),
                                              _lib.ptr(keys), stream), "h3d_mesh_cluster_faces")
        sorted_keys, record_order = torch.sort(keys, stable=True)
        record_offsets = torch.searchsorted(sorted_keys, torch.arange(n_clusters + 1, dtype=torch.int32, device=dev))
    else:
        mapped, keep, record_order = empty(0, 3), None, None
        record_offsets = torch.zeros(n_clusters + 1, dtype=torch.int64, device=dev)
    out = empty(n_clusters, 3, dtype=torch.float32)
    _lib.check(lib.h3d_mesh_cluster_solve(_lib.ptr(vertices), V, _lib.ptr(faces), T, _lib.ptr(vertex_order),
                                          _lib.ptr(vertex_offsets), _lib.ptr(record_order), _lib.ptr(record_offsets), _lib.ptr(table),
                                          n_clusters, origin32, float(cell32), *counts, regularization, reach, _lib.ptr(out), stream),
               "h3d_mesh_cluster_solve")
    kept = mapped[keep] if T > 0 else mapped                 # host read: T'
    return (out, kept, cluster, table) if return_cells else (out, kept, cluster)
