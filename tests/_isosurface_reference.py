"""Marching tetrahedra on the Kuhn split of every grid cell, restated in float64 numpy with the ids and the output order of
include/h3d.h (h3d_isosurface_count / h3d_isosurface_emit), so that kernel and restatement compare array for array.

Orientation is decided here GEOMETRICALLY, unlike in the kernel: every vertex of a tetrahedron's triangles is placed at the midpoint
of its edge, and a triangle is kept when its normal has a positive component along (centroid of the outside corners - centroid of
the inside corners), else its last two corners are swapped.  The midpoint triangle never degenerates (it does not know the values),
so this is well defined where the real triangle has zero area, and it shares no table with the kernel.

    marching_tetrahedra(volume, level, origin, spacing) -> (vertices float64 [V,3], faces int64 [T,3], edge_ids int64 [V])
and, for the tests, the field builders and mesh invariants below.
"""
import itertools
import struct

import numpy as np

DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
PERMUTATIONS = tuple(itertools.permutations((0, 1, 2)))          # lexicographic


def tetrahedron(perm):
    """corners v0..v3 of the tetrahedron of one axis permutation, as integer offsets inside the cell"""
    v = [np.zeros(3, dtype=np.int64)]
    for axis in perm:
        nxt = v[-1].copy()
        nxt[axis] += 1
        v.append(nxt)
    return np.stack(v)            # v3 = (1,1,1)


def case_triangles(corners, inside):
    """triangles of one tetrahedron (corners [4,3]) for one inside pattern (4 bools) -> list of triangles, each three edges
    (a, b) with a < b indices into v0..v3, oriented from inside to outside by the midpoint rule"""
    ins = [i for i in range(4) if inside[i]]
    outs = [i for i in range(4) if not inside[i]]
    if len(ins) in (0, 4):
        return []
    edge = lambda a, b: (min(a, b), max(a, b))
    if len(ins) == 2:
        (i0, i1), (o0, o1) = ins, outs
        tris = [[edge(i0, o0), edge(i0, o1), edge(i1, o1)], [edge(i0, o0), edge(i1, o1), edge(i1, o0)]]
    else:
        lone, rest = (ins[0], outs) if len(ins) == 1 else (outs[0], ins)
        tris = [[edge(lone, r) for r in rest]]
    c = corners.astype(np.float64)
    outward = c[outs].mean(axis=0) - c[ins].mean(axis=0)
    result = []
    for tri in tris:
        m = [(c[a] + c[b]) / 2 for a, b in tri]
        normal = np.cross(m[1] - m[0], m[2] - m[0])
        d = float(normal @ outward)
        assert abs(d) > 1e-9
        result.append(tri if d > 0 else [tri[0], tri[2], tri[1]])
    return result


def marching_tetrahedra(volume, level, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    vol = np.asarray(volume)
    Nx, Ny, Nz = vol.shape
    val = vol.astype(np.float64)
    level = float(vol.dtype.type(level)) if vol.dtype.kind == "f" else float(level)    # the level in the volume's own format
    with np.errstate(invalid="ignore"):
        inside = val > level
    origin, spacing = np.asarray(origin, dtype=np.float64), np.asarray(spacing, dtype=np.float64)
    node = np.arange(Nx * Ny * Nz, dtype=np.int64).reshape(Nx, Ny, Nz)
    grid = np.stack(np.meshgrid(np.arange(Nx), np.arange(Ny), np.arange(Nz), indexing="ij"), axis=-1).astype(np.float64)

    # vertices: one per existing edge whose ends lie on different sides, in ascending edge id
    ids, pos = [], []
    for t, d in enumerate(DIRECTIONS):
        lo = tuple(slice(0, n - k) for n, k in zip((Nx, Ny, Nz), d))
        hi = tuple(slice(k, n) for n, k in zip((Nx, Ny, Nz), d))
        cross = inside[lo] != inside[hi]
        a, b = val[lo][cross], val[hi][cross]
        with np.errstate(all="ignore"):
            s = (level - a) / (b - a)
        ids.append(node[lo][cross] * 7 + t)
        pos.append(origin + spacing * (grid[lo][cross] + s[:, None] * np.asarray(d, dtype=np.float64)))
    ids, pos = np.concatenate(ids), np.concatenate(pos)
    order = np.argsort(ids, kind="stable")
    edge_ids, vertices = ids[order], pos[order]
    vertex_of_edge = np.full(Nx * Ny * Nz * 7, -1, dtype=np.int64)
    vertex_of_edge[edge_ids] = np.arange(len(edge_ids))

    # faces: per tetrahedron and case, every cell of that case at once; sorted by (cell, tetrahedron, triangle) at the end
    cell = np.arange((Nx - 1) * (Ny - 1) * (Nz - 1), dtype=np.int64).reshape(Nx - 1, Ny - 1, Nz - 1)
    corner = lambda arr, off: arr[off[0]:off[0] + Nx - 1, off[1]:off[1] + Ny - 1, off[2]:off[2] + Nz - 1]
    type_of = {d: t for t, d in enumerate(DIRECTIONS)}
    keys, rows = [], []
    for k, perm in enumerate(PERMUTATIONS):
        corners = tetrahedron(perm)
        pattern = sum(corner(inside, corners[i]).astype(np.int64) << i for i in range(4))
        for case in range(1, 15):
            sel = pattern == case
            if not sel.any():
                continue
            for j, tri in enumerate(case_triangles(corners, [bool(case >> i & 1) for i in range(4)])):
                idx = []
                for a, b in tri:
                    edge = corner(node, corners[a])[sel] * 7 + type_of[tuple(int(v) for v in corners[b] - corners[a])]
                    idx.append(vertex_of_edge[edge])
                rows.append(np.stack(idx, axis=1))
                keys.append(cell[sel] * 12 + k * 2 + j)
    if not rows:
        return vertices, np.zeros((0, 3), dtype=np.int64), edge_ids
    keys, rows = np.concatenate(keys), np.concatenate(rows)
    faces = rows[np.argsort(keys, kind="stable")]
    assert (faces >= 0).all()
    return vertices, faces, edge_ids


# ---------------------------------------------------------------------------------------------------------------- fields
def _coordinates(shape):
    return np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")


def sphere(shape, radius, centre=None):
    """radius - distance to `centre` (default: the grid's centre moved by (0.13, 0.21, -0.17)): positive inside, level 0"""
    x, y, z = _coordinates(shape)
    c = [(n - 1) / 2 + o for n, o in zip(shape, (0.13, 0.21, -0.17))] if centre is None else centre
    return (radius - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)).astype(np.float32)


def torus(shape, R, r):
    x, y, z = _coordinates(shape)
    c = [(n - 1) / 2 for n in shape]
    ring = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2) - R
    return (r - np.sqrt(ring ** 2 + (z - c[2]) ** 2)).astype(np.float32)


def octahedron(n=7, size=4.0):
    """the integer field size - |x - centre|_1: at an integer level many node values EQUAL the level"""
    x, y, z = _coordinates((n, n, n))
    c = (n - 1) / 2
    return (size - (np.abs(x - c) + np.abs(y - c) + np.abs(z - c))).astype(np.float32)


def smooth_random(shape, seed):
    """a few random low-frequency waves: a smooth field with both signs and no symmetry"""
    rng = np.random.default_rng(seed)
    x, y, z = _coordinates(shape)
    out = np.zeros(shape)
    for _ in range(4):
        k = rng.uniform(0.5, 1.7, size=3)
        ph = rng.uniform(0, 2 * np.pi, size=3)
        out += rng.uniform(0.5, 1.0) * np.sin(k[0] * x + ph[0]) * np.sin(k[1] * y + ph[1]) * np.sin(k[2] * z + ph[2])
    return out.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ invariants
def canonical(faces):
    """each face rotated so that its smallest index comes first (the orientation is kept)"""
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    shift = np.argmin(faces, axis=1)
    return np.stack([faces[np.arange(len(faces)), (shift + j) % 3] for j in range(3)], axis=1)


def edge_census(faces):
    """-> (directed edges [3T,2], count of every undirected edge)"""
    f = np.asarray(faces).astype(np.int64)
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    undirected = np.sort(directed, axis=1)
    _, counts = np.unique(undirected, axis=0, return_counts=True)
    return directed, counts


def is_closed_and_oriented(n_vertices, faces):
    directed, counts = edge_census(faces)
    every_edge_twice = bool((counts == 2).all())
    each_direction_once = len(np.unique(directed, axis=0)) == len(directed)
    every_vertex_used = len(np.unique(faces)) == n_vertices
    return every_edge_twice and each_direction_once and every_vertex_used


def euler_characteristic(n_vertices, faces):
    _, counts = edge_census(faces)
    return n_vertices - len(counts) + len(faces)


def signed_volume(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


# -------------------------------------------------------------------------------------------------------------- mesh files
def parse_ply(path):
    """A reader for exactly what write_ply promises: binary little-endian, float x y z, uchar-int face lists."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elements = [l.split() for l in lines if l.startswith("element")]
    assert [e[1] for e in elements] == ["vertex", "face"]
    props = [l for l in lines if l.startswith("property")]
    assert props == ["property float x", "property float y", "property float z", "property list uchar int vertex_indices"]
    nv, nf = int(elements[0][2]), int(elements[1][2])
    body = data[end:]
    assert len(body) == nv * 12 + nf * 13
    v = np.frombuffer(body[:nv * 12], dtype="<f4").reshape(nv, 3)
    faces = []
    for i in range(nf):
        n, a, b, c = struct.unpack_from("<Biii", body, nv * 12 + i * 13)
        assert n == 3
        faces.append((a, b, c))
    return v, np.array(faces, dtype=np.int64).reshape(nf, 3)
