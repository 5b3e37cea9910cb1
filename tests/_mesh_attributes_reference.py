"""A numpy restatement of the two mesh-attribute definitions of include/h3d.h (h3d_isosurface_normals, h3d_mesh_project_colors),
written from the text, not from the kernels: node gradients as a whole array, views in a python loop.  Every function takes
dtype=: float64 is the reference, float32 runs the SAME code in the kernels' number format and is the yardstick of their rounding
(tests/test_gpu_mesh_attributes.py takes its bars from the distance of the two).
"""
import numpy as np


def node_gradient(volume, spacing):
    """G [Nx,Ny,Nz,3]: central differences, one-sided over one spacing at the two border planes of each axis"""
    G = np.empty(volume.shape + (3,), dtype=volume.dtype)
    for a in range(3):
        v = np.moveaxis(volume, a, 0)
        d = np.empty_like(v)
        d[1:-1] = (v[2:] - v[:-2]) / (2 * spacing[a])
        d[0] = (v[1] - v[0]) / spacing[a]
        d[-1] = (v[-1] - v[-2]) / spacing[a]
        G[..., a] = np.moveaxis(d, 0, a)
    return G


def vertex_gradient(volume, vertices, origin=(0, 0, 0), spacing=(1, 1, 1), dtype=np.float64):
    """G^ [V,3]: the trilinear interpolation of the node gradient at every vertex; 0 at a vertex with a non-finite coordinate"""
    volume, vertices = np.asarray(volume, dtype=dtype), np.asarray(vertices, dtype=dtype).reshape(-1, 3)
    origin, spacing = np.asarray(origin, dtype=dtype), np.asarray(spacing, dtype=dtype)
    G = node_gradient(volume, spacing)
    N = np.array(volume.shape)
    good = np.isfinite(vertices).all(axis=1)
    with np.errstate(invalid="ignore"):
        g = (np.where(good[:, None], vertices, origin) - origin) / spacing
    g = np.clip(g, 0, (N - 1).astype(dtype))
    c = np.minimum(np.floor(g).astype(np.int64), N - 2)
    f = g - c.astype(dtype)
    out = np.zeros((len(vertices), 3), dtype=dtype)
    for corner in range(8):
        o = np.array([corner & 1, corner >> 1 & 1, corner >> 2])
        w = np.prod(np.where(o == 1, f, 1 - f), axis=1)
        p = c + o
        out += w[:, None] * G[p[:, 0], p[:, 1], p[:, 2]]
    out[~good] = 0
    return out


def vertex_normals(volume, vertices, origin=(0, 0, 0), spacing=(1, 1, 1), dtype=np.float64):
    """-> (normals [V,3] = -G^ / |G^|, (0,0,0) where |G^| is zero or not finite; G^ [V,3])"""
    G = vertex_gradient(volume, vertices, origin, spacing, dtype)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        length = np.sqrt((G * G).sum(axis=1))
        usable = np.isfinite(length) & (length > 0)
        normals = np.where(usable[:, None], -G / np.where(usable, length, 1)[:, None], 0).astype(dtype)
    return normals, G


def _bilinear(plane, x, y):
    """plane [..., rows, cols] sampled at (x, y) [V], coordinates clamped to the plane"""
    rows, cols = plane.shape[-2:]
    x, y = np.clip(np.nan_to_num(x, nan=0.0), 0, cols - 1), np.clip(np.nan_to_num(y, nan=0.0), 0, rows - 1)
    x0, y0 = np.minimum(np.floor(x).astype(np.int64), cols - 1), np.minimum(np.floor(y).astype(np.int64), rows - 1)
    x1, y1 = np.minimum(x0 + 1, cols - 1), np.minimum(y0 + 1, rows - 1)
    ax, ay = x - x0.astype(x.dtype), y - y0.astype(y.dtype)
    top = plane[..., y0, x0] * (1 - ax) + plane[..., y0, x1] * ax
    bottom = plane[..., y1, x0] * (1 - ax) + plane[..., y1, x1] * ax
    return top * (1 - ay) + bottom * ay


def view_weight(x, n, depth, focal, cam2world, depth_tolerance, normal_power, dtype=np.float64, parts=False):
    """One view: -> (w [V], u [V], v [V]) -- the weight (0 where not ok or not finite) and the render-grid coordinates"""
    h, w = depth.shape
    c2w = np.asarray(cam2world, dtype=np.float64)
    w2c = np.linalg.inv(c2w).astype(dtype)                 # inverted in float64, as the host side does
    o = c2w[:3, 3].astype(dtype)
    focal = dtype(focal)
    with np.errstate(all="ignore"):
        p = x @ w2c[:3, :3].T + w2c[:3, 3]
        ok = p[:, 2] > 1e-6
        xn, yn = focal * p[:, 0] / p[:, 2], focal * p[:, 1] / p[:, 2]
        span = dtype(w) / dtype(h)
        u = (xn + span) / (2 * span) * dtype(w - 1)
        v = (yn + 1) / 2 * dtype(h - 1)
        rel = x - o
        t = np.sqrt((rel * rel).sum(axis=1))
        d = rel / t[:, None]
        base = np.maximum(0, -(n * d).sum(axis=1))
        face = base.copy()
        for _ in range(int(normal_power) - 1):
            face = face * base
        edge = np.clip(np.minimum(np.minimum(u, dtype(w - 1) - u), np.minimum(v, dtype(h - 1) - v)), 0, 1)
        D = _bilinear(depth, u, v)
        vis = np.clip(1 - np.abs(t - D) / dtype(depth_tolerance), 0, 1)
        wk = edge * vis * face
        wk = np.where(ok & np.isfinite(wk), wk, 0).astype(dtype)
    if parts:
        return wk, u, v, dict(ok=ok, face=face, edge=edge, vis=vis, t=t, D=D)
    return wk, u, v


def project_colors(vertices, normals, images, depths, focals, scales, cam2world, depth_tolerance, normal_power=2, fill=0.0, eps=1e-3,
                   dtype=np.float64):
    """-> (colors [V,3], coverage [V]); `scales` is not read (the depths are ray distances already)"""
    x, n = np.asarray(vertices, dtype=dtype).reshape(-1, 3), np.asarray(normals, dtype=dtype).reshape(-1, 3)
    images, depths = np.asarray(images, dtype=dtype), np.asarray(depths, dtype=dtype)
    K, _, H, W = images.shape
    h, w = depths.shape[1:]
    coverage, total = np.zeros(len(x), dtype=dtype), np.zeros((len(x), 3), dtype=dtype)
    for k in range(K):
        wk, u, v = view_weight(x, n, depths[k], np.asarray(focals).reshape(-1)[k], np.asarray(cam2world)[k], depth_tolerance, normal_power,
                               dtype)
        with np.errstate(all="ignore"):
            ui = (u + dtype(0.5)) * (dtype(W) / dtype(w)) - dtype(0.5)
            vi = (v + dtype(0.5)) * (dtype(H) / dtype(h)) - dtype(0.5)
            c = _bilinear(images[k], ui, vi).T               # [V,3]
        seen = wk > 0
        coverage += wk
        total += np.where(seen[:, None], wk[:, None] * c, 0).astype(dtype)
    eps, fill = dtype(eps), dtype(fill)
    return ((total + eps * fill) / (coverage + eps)[:, None]).astype(dtype), coverage


# ------------------------------------------------------------------------------------------------------------------ scenes
def look_at(origin, target):
    """cam2world [4,4] of the camera of csrc/ray_setup.hip at `origin` whose +z axis (the rays' (x, y, focal)) points at `target`"""
    origin, target = np.asarray(origin, dtype=np.float64), np.asarray(target, dtype=np.float64)
    fwd = (target - origin) / np.linalg.norm(target - origin)
    up = np.array([0.0, 1.0, 0.0]) if abs(fwd[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, fwd)
    x /= np.linalg.norm(x)
    y = np.cross(fwd, x)
    M = np.eye(4)
    M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = x, y, fwd, origin
    return M


def pixel_rays(cam2world, focal, h, w):
    """world-space unit directions [h,w,3] of the render grid: x in linspace(-w/h, w/h, w), y in linspace(-1, 1, h)"""
    x, y = np.meshgrid(np.linspace(-w / h, w / h, w), np.linspace(-1, 1, h), indexing="xy")
    d = np.stack([x, y, np.full_like(x, focal)], axis=-1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return d @ cam2world[:3, :3].T


def sphere_depth(cam2world, focal, h, w, centre, radius, miss):
    """the analytic distance along every ray of the render grid to the sphere [h,w]; `miss` where the ray passes it"""
    d, oc = pixel_rays(cam2world, focal, h, w), cam2world[:3, 3] - np.asarray(centre)
    b = d @ oc
    disc = b * b - (oc @ oc - radius * radius)
    return np.where(disc > 0, -b - np.sqrt(np.maximum(disc, 0)), miss)


def sphere_scene(K, h, w, H, W, radius=1.0, distance=4.0, focal=1.5, centre=(0.3, -0.2, 0.5)):
    """K cameras around a sphere, each looking at its centre, with the analytic depth maps and smooth images in [-1, 1]
    -> dict(centre, radius, images [K,3,H,W], depths [K,h,w], focals [K], scales [K], cam2world [K,4,4]), float64"""
    centre = np.asarray(centre, dtype=np.float64)
    cams = []
    for k in range(K):
        a = 0.3 + 0.8 * 2 * np.pi * k / K
        direction = np.array([np.sin(a), 0.3 * np.sin(2 * a + 1), np.cos(a)])
        cams.append(look_at(centre + distance * direction / np.linalg.norm(direction), centre))
    cams = np.stack(cams)
    focals = focal * (1 + 0.05 * np.arange(K))
    depths = np.stack([sphere_depth(cams[k], focals[k], h, w, centre, radius, distance + 2 * radius) for k in range(K)])
    X, Y = np.meshgrid(np.linspace(0, 1, W), np.linspace(0, 1, H), indexing="xy")
    images = np.stack([np.stack([np.sin(0.7 * k + c + 3 * X) * np.cos(2 * Y + c) for c in range(3)]) for k in range(K)])
    return dict(centre=centre, radius=radius, images=images, depths=depths, focals=focals, scales=np.full(K, 1.6), cam2world=cams)


def sphere_points(n, centre, radius, seed):
    """n points spread over the sphere -> (positions [n,3], outward unit normals [n,3])"""
    d = np.random.default_rng(seed).normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.asarray(centre) + radius * d, d


# -------------------------------------------------------------------------------------------------------------- mesh files
def parse_attributed_ply(path):
    """A reader for what write_ply promises with attributes: binary little-endian, float and uchar vertex properties in the header's
    order, packed rows, uchar-int face lists -> (property names, structured vertex rows, faces [T,3])"""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elements = [l.split() for l in lines if l.startswith("element")]
    assert [e[1] for e in elements] == ["vertex", "face"]
    props = [l.split()[1:] for l in lines if l.startswith("property")]
    assert props[-1] == ["list", "uchar", "int", "vertex_indices"]
    dtype = np.dtype([(name, {"float": "<f4", "uchar": "u1"}[kind]) for kind, name in props[:-1]])
    nv, nf = int(elements[0][2]), int(elements[1][2])
    body = data[end:]
    assert len(body) == nv * dtype.itemsize + nf * 13
    vertices = np.frombuffer(body[:nv * dtype.itemsize], dtype=dtype)
    faces = np.frombuffer(body[nv * dtype.itemsize:], dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    assert (faces["n"] == 3).all()
    return [name for _, name in props[:-1]], vertices, faces["i"]
