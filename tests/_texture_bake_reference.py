"""A numpy restatement of the texture atlas and its bake (include/h3d.h, h3d_mesh_bake_texture), written from the text, not from the
kernel or the host module: the layout over whole index arrays, the per-texel colour through the per-point restatement of
tests/_mesh_attributes_reference.py (view_weight, _bilinear).  bake() takes dtype=: float64 is the reference, float32 runs the SAME
code in the kernel's number format and is the yardstick of its rounding (tests/test_gpu_texture_bake.py takes its bars from the
distance of the two).  Beside it: the sphere meshes, the scene and a viewer's bilinear lookup, shared by the CPU and the GPU tests."""
import math

import numpy as np

from _mesh_attributes_reference import _bilinear, sphere_scene, view_weight

f32, f64 = np.float32, np.float64
LAYOUT_CASES = [(1, 4), (2, 4), (3, 8), (7, 9), (8, 8), (128, 50), (513, 100), (512, 256)]


# ------------------------------------------------------------------------------------------------------------------ layout
def layout(T, S):
    """-> (c, R): cell edge and cells per row"""
    cells = -(-T // 2)
    R = 1 if T == 0 else math.isqrt(cells - 1) + 1
    return S // R, R


def ownership(T, S, dtype=f64):
    """-> (owner int64 [S,S]: the triangle of every texel, -1 where nobody owns it; barycentrics [S,S,3] in dtype, unclamped)"""
    c, R = layout(T, S)
    r, q = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    cy, cx, j, i = r // c, q // c, r % c, q % c
    upper = i + j >= c - 1
    t = 2 * (cy * R + cx) + upper
    owned = (cy < R) & (cx < R) & (t < T)
    ii, jj = np.where(upper, c - 1 - i, i), np.where(upper, c - 1 - j, j)
    b1, b2 = ii.astype(dtype) / dtype(c - 3), jj.astype(dtype) / dtype(c - 3)
    b0 = dtype(1) - b1 - b2
    return np.where(owned, t, -1), np.stack([b0, b1, b2], axis=-1).astype(dtype)


def uvs(T, S):
    """corner UVs float64 [T,3,2], v = 0 at the top row"""
    c, R = layout(T, S)
    out = np.empty((T, 3, 2))
    for t in range(T):
        x0, y0, m = (t // 2 % R) * c, (t // 2 // R) * c, c - 3
        if t % 2 == 0:
            out[t] = [(x0 + .5, y0 + .5), (x0 + m + .5, y0 + .5), (x0 + .5, y0 + m + .5)]
        else:
            out[t] = [(x0 + c - .5, y0 + c - .5), (x0 + 2.5, y0 + c - .5), (x0 + c - .5, y0 + 2.5)]
    return out / S


def lookup_taps(uv, S):
    """A viewer's LINEAR / CLAMP_TO_EDGE sampling at uv [n,2] -> (rows [n,4], columns [n,4], weights [n,4]); texel centres lie at
    (index + 1/2) / S"""
    x, y = np.clip(uv[:, 0] * S - 0.5, 0, S - 1), np.clip(uv[:, 1] * S - 0.5, 0, S - 1)
    x0, y0 = np.minimum(np.floor(x).astype(np.int64), S - 1), np.minimum(np.floor(y).astype(np.int64), S - 1)
    x1, y1 = np.minimum(x0 + 1, S - 1), np.minimum(y0 + 1, S - 1)
    ax, ay = x - x0, y - y0
    return (np.stack([y0, y0, y1, y1], axis=1), np.stack([x0, x1, x0, x1], axis=1),
            np.stack([(1 - ax) * (1 - ay), ax * (1 - ay), (1 - ax) * ay, ax * ay], axis=1))


def lookup(texture, uv):
    """texture [S,S,C] sampled as a viewer samples it -> [n,C]"""
    rows, cols, w = lookup_taps(uv, texture.shape[0])
    return (texture[rows, cols] * w[..., None]).sum(axis=1)


# -------------------------------------------------------------------------------------------------------------- definition
def _unit(v, dtype):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        length = np.sqrt((v * v).sum(axis=-1))
        usable = np.isfinite(length) & (length > 0)
        return np.where(usable[..., None], v / np.where(usable, length, 1)[..., None], 0).astype(dtype)


def colour_at(x, n, images, depths, focals, cam2world, depth_tolerance, normal_power, fill, eps, dtype):
    """the per-point definition of h3d_mesh_project_colors at positions x [n,3] with normals n -> (colour [n,3], coverage [n])"""
    images, depths = np.asarray(images, dtype=dtype), np.asarray(depths, dtype=dtype)
    K, _, H, W = images.shape
    h, w = depths.shape[1:]
    coverage, total = np.zeros(len(x), dtype=dtype), np.zeros((len(x), 3), dtype=dtype)
    for k in range(K):
        wk, u, v = view_weight(x, n, depths[k], np.asarray(focals).reshape(-1)[k], np.asarray(cam2world)[k], depth_tolerance, normal_power,
                               dtype)
        with np.errstate(all="ignore"):
            c = _bilinear(images[k], (u + dtype(0.5)) * (dtype(W) / dtype(w)) - dtype(0.5),
                          (v + dtype(0.5)) * (dtype(H) / dtype(h)) - dtype(0.5)).T
        coverage += wk
        total += np.where((wk > 0)[:, None], wk[:, None] * c, 0).astype(dtype)
    eps, fill = dtype(eps), dtype(fill)
    return ((total + eps * fill) / (coverage + eps)[:, None]).astype(dtype), coverage


def surface_point(vertices, normals, faces, triangles, bary, dtype):
    """x = b0 v0 + b1 v1 + b2 v2 and the normalised interpolated normal, face indices clamped into the vertex range"""
    f = np.clip(np.asarray(faces)[triangles], 0, len(vertices) - 1)
    v, nr = np.asarray(vertices, dtype=dtype)[f], np.asarray(normals, dtype=dtype)[f]           # [n,3,3]
    b = bary.astype(dtype)[..., None]
    with np.errstate(invalid="ignore"):
        x = b[:, 0] * v[:, 0] + b[:, 1] * v[:, 1] + b[:, 2] * v[:, 2]
        n = b[:, 0] * nr[:, 0] + b[:, 1] * nr[:, 1] + b[:, 2] * nr[:, 2]
    return x.astype(dtype), _unit(n, dtype)


def bake(vertices, faces, normals, scene, depth_tolerance, S, normal_power=2, fill=0.0, eps=1e-3, dtype=f64):
    """-> (texture [S,S,3], coverage [S,S], owner [S,S])"""
    T = len(faces)
    owner, bary = ownership(T, S, dtype)
    texture, coverage = np.full((S, S, 3), dtype(fill), dtype=dtype), np.zeros((S, S), dtype=dtype)
    own = owner >= 0
    if own.any():
        x, n = surface_point(vertices, normals, faces, owner[own], bary[own], dtype)
        texture[own], coverage[own] = colour_at(x, n, scene["images"], scene["depths"], scene["focals"], scene["cam2world"], depth_tolerance,
                                                normal_power, fill, eps, dtype)
    return texture, coverage, owner


# ------------------------------------------------------------------------------------------------------------------ scenes
def octa_sphere(n, centre=(0, 0, 0), radius=1.0):
    """An octahedron subdivided n times, every vertex pushed onto the sphere: 8 * 4^n triangles wound outwards
    -> (vertices float64 [V,3], unit normals [V,3], faces int32 [T,3])"""
    v = [np.array(p, dtype=f64) for p in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    faces = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(n):
        middle, out = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in middle:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                middle[key] = len(v) - 1
            return middle[key]

        for a, b, c in faces:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        faces = out
    d = np.stack(v)
    return np.asarray(centre) + radius * d, d, np.asarray(faces, dtype=np.int32)


_SCENES = {}


def detailed_scene(K, h, w, H, W):
    """sphere_scene with image detail far above a coarse mesh's resolution: sin(0.7 k + c + 25 X) cos(20 Y + c).  Made once per
    shape and shared: treat it as read-only."""
    key = (K, h, w, H, W)
    if key not in _SCENES:
        s = sphere_scene(K, h, w, H, W)
        X, Y = np.meshgrid(np.linspace(0, 1, W), np.linspace(0, 1, H), indexing="xy")
        s["images"] = np.stack([np.stack([np.sin(0.7 * k + c + 25 * X) * np.cos(20 * Y + c) for c in range(3)]) for k in range(K)])
        _SCENES[key] = s
    return _SCENES[key]


def mesh_points(vertices, faces, n, seed):
    """n points uniform over the surface of the mesh -> (triangles [n], barycentrics [n,3])"""
    rng = np.random.default_rng(seed)
    a, b, c = (vertices[faces[:, k]] for k in range(3))
    area = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    triangles = rng.choice(len(faces), size=n, p=area / area.sum())
    r1, r2 = np.sqrt(rng.uniform(size=n)), rng.uniform(size=n)
    return triangles, np.stack([1 - r1, r1 * (1 - r2), r1 * r2], axis=1)
