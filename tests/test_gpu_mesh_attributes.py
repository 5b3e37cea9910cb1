"""h3d_isosurface_normals and h3d_mesh_project_colors against the float64 restatement (tests/_mesh_attributes_reference.py, itself
checked by tests/test_mesh_attributes_cpu.py), on every vertex: both definitions are continuous, nothing is left undecided.

Bars.  No constant of this file enters one: bar = 8 x max |restatement in float32 - restatement in float64| on the case's own inputs,
and not less than 4 * 2^-23 x max |float64 output|.  The float32 restatement is the same numpy code in the kernels' format -- the
size of honest rounding for these inputs; 8 because a kernel may contract to FMAs and sum in another order.  A lost term (a view, a
stencil value, a weight) is of order 0.1 - 1.  The maximum is taken over at least 257 vertices: a case that launches fewer launches
the first V of a pool of 257 made by the same generator, and the pool gives the bar (the error of one vertex is one draw of the
rounding, not its size).  Measured errors and bars are printed and stand in DESIGN 4.5d."""
import importlib

import numpy as np
import pytest
import torch

import _isosurface_reference as R
import _mesh_attributes_reference as M

pytestmark = pytest.mark.gpu
iso = importlib.import_module("3dhumangan_amd.lib.components.isosurface")
mesh_color = importlib.import_module("3dhumangan_amd.lib.components.mesh_color")
DEV = "cuda"
POOL = 257
f32, f64 = np.float32, np.float64


def bar_of(low, high):
    return max(8.0 * float(np.abs(low.astype(f64) - high).max()), 4.0 * 2.0 ** -23 * float(np.abs(high).max()))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=f32)).to(DEV)


# ----------------------------------------------------------------------------------------------------------------- normals
def volume_of(kind, shape):
    if kind == "sphere":
        return R.sphere(shape, 5.0)
    return np.random.default_rng(0).normal(size=shape).astype(f32)


def vertex_pool(shape, origin, spacing, n, seed):
    """n positions (fp32-representable): first the special ones -- the first and the last node, the last node of each axis, points
    exactly on nodes, points outside the grid on every side -- then uniform ones in the grid's box"""
    rng = np.random.default_rng(seed)
    top = np.array(shape) - 1.0
    special = [np.zeros(3), top] + [np.where(np.arange(3) == a, top, top / 2) for a in range(3)]
    special += [np.floor(rng.uniform(size=3) * (top + 1)) for _ in range(8)]                   # on nodes
    special += [np.where(np.arange(3) == a, side, rng.uniform(size=3) * top) for a in range(3) for side in (-1.7, top[a] + 2.3)]
    special += [top + 5.0, -np.ones(3)]
    g = np.concatenate([rng.uniform(size=(1, 3)) * top, np.stack(special), rng.uniform(size=(max(n - len(special) - 1, 0), 3)) * top])[:n]
    return (np.asarray(origin) + np.asarray(spacing) * g).astype(f32)


FRAME = ((0.25, -1.5, 3.0), (0.5, 0.125, 0.75))
CUBIC = ((0.25, -1.5, 3.0), (0.5, 0.5, 0.5))               # noise: with unequal spacings one axis dominates |G| and the 5 % rule leaves out more
NORMAL_CASES = [("noise", (2, 2, 2), 257, FRAME), ("noise", (5, 3, 2), 1, CUBIC), ("noise", (5, 3, 2), 257, ((0, 0, 0), (1, 1, 1))),
                ("sphere", (13, 21, 34), None, ((0, 0, 0), (1, 1, 1))), ("sphere", (13, 21, 34), 257, FRAME),
                ("noise", (13, 21, 34), 5000, CUBIC), ("noise", (13, 21, 34), 1, ((0, 0, 0), (1, 1, 1)))]


@pytest.mark.parametrize("kind,shape,V,frame", NORMAL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_normals_against_the_restatement(kind, shape, V, frame):
    origin, spacing = frame
    volume = volume_of(kind, shape)
    pool = vertex_pool(shape, origin, spacing, max(V or 0, POOL), seed=sum(shape))
    if max(shape) > 5:
        # the level-0 surface's own vertices, every one on a grid edge (the sphere's all of them, the noise's first ones), behind the
        # special ones; on a grid edge the gradient is interpolated between two nodes only, so that few vertices fall under the 5 % rule
        surface = (np.asarray(origin) + np.asarray(spacing) * R.marching_tetrahedra(volume, 0.0)[0]).astype(f32)
        pool = np.concatenate([pool[:32], surface])
        V = len(pool) if V is None else V
        pool = pool[:max(V, POOL)]
    n64, g64 = M.vertex_normals(volume, pool, origin, spacing, dtype=f64)
    n32, g32 = M.vertex_normals(volume, pool, origin, spacing, dtype=f32)
    normals, gradient = iso.vertex_normals(dev(volume), dev(pool[:V]), origin, spacing, return_gradient=True)
    assert normals.shape == (V, 3) and gradient.shape == (V, 3) and normals.dtype == gradient.dtype == torch.float32
    normals, gradient = normals.cpu().numpy().astype(f64), gradient.cpu().numpy().astype(f64)
    g_err, g_bar, g_max = np.abs(gradient - g64[:V]).max(), bar_of(g32, g64), np.abs(g64).max()
    length = np.linalg.norm(g64, axis=1)
    steep = length >= 0.05 * length.max()
    left_out = 1.0 - steep.mean()
    n_err, n_bar = np.abs(normals - n64[:V])[steep[:V]].max(initial=0.0), bar_of(n32[steep], n64[steep])
    print(f"normals {kind} {shape} V={V}: gradient err {g_err:.2e} bar {g_bar:.2e} (max |G| {g_max:.2e}); normal err {n_err:.2e} "
          f"bar {n_bar:.2e}; left out {100 * left_out:.2f} %")
    assert g_err <= g_bar
    assert left_out <= 0.02
    assert n_err <= n_bar
    only_normals = iso.vertex_normals(dev(volume), dev(pool[:V]), origin, spacing)
    assert torch.equal(only_normals.cpu(), torch.as_tensor(normals.astype(f32)))


def test_normals_twice_noncontiguous_nonfinite_and_empty():
    shape, (origin, spacing) = (13, 21, 34), FRAME
    volume, pool = dev(volume_of("noise", shape)), vertex_pool(shape, *FRAME, 5000, seed=9)
    vertices = dev(pool)
    a = iso.vertex_normals(volume, vertices, origin, spacing, return_gradient=True)
    b = iso.vertex_normals(volume, vertices, origin, spacing, return_gradient=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # a permuted view of a volume stored in another order is copied
    stored = volume.permute(2, 0, 1).contiguous()
    view = stored.permute(1, 2, 0)
    assert not view.is_contiguous() and torch.equal(view, volume)
    c = iso.vertex_normals(view, vertices, origin, spacing, return_gradient=True)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    # NaN and +-inf: those rows are zero, every other row keeps its bits
    bad = vertices.clone()
    rows = [0, 63, 64, 255, 256, 4999]
    for r, (column, value) in zip(rows, [(0, float("nan")), (1, float("inf")), (2, float("-inf")), (0, float("inf")), (1, float("nan")),
                                         (2, float("nan"))]):
        bad[r, column] = value
    bad[64] = float("nan")
    n, g = iso.vertex_normals(volume, bad, origin, spacing, return_gradient=True)
    keep = torch.ones(len(bad), dtype=torch.bool)
    keep[rows] = False
    assert (n[rows] == 0).all() and (g[rows] == 0).all()
    assert torch.equal(n[keep], a[0][keep]) and torch.equal(g[keep], a[1][keep])
    n, g = iso.vertex_normals(volume, vertices[:0], origin, spacing, return_gradient=True)
    assert n.shape == (0, 3) and g.shape == (0, 3) and n.device.type == "cuda"
    assert iso.vertex_normals(volume, vertices[:0]).shape == (0, 3)


# -------------------------------------------------------------------------------------------------------------- projection
def scene_pool(K, h, w, H, W, tolerance, n, seed):
    """A sphere scene with, in view 0, a nearer surface over the left half of its depth map (an occluder), and n vertices: points
    placed on the depth maps themselves within +-1.5 tolerances along their ray (so that tiny render grids, which miss the sphere,
    have seen vertices too; the first of them well inside, for a launch of one vertex), sphere points (facing, back-facing, occluded,
    near the silhouette), and in rows 1..4 the special ones: behind a camera, outside the image, a zero normal, the camera origin."""
    s = M.sphere_scene(K, h, w, H, W)
    s["depths"][0][:, : w // 2] -= 1.0
    rng = np.random.default_rng(seed)
    n_sphere = n // 2
    x, nrm = M.sphere_points(n_sphere, s["centre"], s["radius"], seed)
    nrm = nrm + 0.1 * rng.normal(size=nrm.shape)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    xs, ns = [], []
    for i in range(n - n_sphere):
        k = int(rng.integers(K))
        c2w, focal = s["cam2world"][k], s["focals"][k]
        u, v = rng.uniform(-0.25, w - 0.75), rng.uniform(-0.25, h - 0.75)
        if i == 0:                                          # the one vertex of a V = 1 launch: well inside its image
            u, v = 0.7 * (w - 1), 0.6 * (h - 1)
        d = np.array([(2 * u / (w - 1) - 1) * w / h, 2 * v / (h - 1) - 1, focal])
        d = c2w[:3, :3] @ (d / np.linalg.norm(d))
        D = M._bilinear(s["depths"][k], np.array([u]), np.array([v]))[0]
        xs.append((c2w[:3, 3] + (D + (0.3 if i == 0 else rng.uniform(-1.5, 1.5)) * tolerance) * d)[None])
        m = -d + 0.3 * rng.normal(size=3)
        ns.append((m / np.linalg.norm(m))[None])
    x, nrm = np.concatenate(xs + [x]), np.concatenate(ns + [nrm])           # the placed points first, then the sphere's
    c2w = s["cam2world"][0]
    o, right, fwd = c2w[:3, 3], c2w[:3, 0], c2w[:3, 2]
    if n >= 8:
        x[1], nrm[1] = o - 2.0 * fwd, fwd                                   # behind camera 0, facing it
        x[2], nrm[2] = o + 3.0 * fwd + 5.0 * right, -fwd                     # outside its image
        nrm[3] = 0.0                                                         # a zero normal
        x[4], nrm[4] = o, -fwd                                               # at the camera origin: t = 0, the direction is 0/0
    s["vertices"], s["normals"] = x.astype(f32), nrm.astype(f32)
    for key in ("images", "depths", "focals", "cam2world"):                  # the kernel's inputs: every format sees the same numbers
        s[key] = s[key].astype(f32)
    return s


def run_reference(s, V, tolerance, power, fill, eps, dtype):
    colors, coverage = M.project_colors(s["vertices"][:V], s["normals"][:V], s["images"], s["depths"], s["focals"], s["scales"],
                                        s["cam2world"], tolerance, power, fill, eps, dtype=dtype)
    numerator = colors.astype(f64) * (coverage.astype(f64) + eps)[:, None] - eps * fill
    return colors, coverage, numerator


def run_kernel(s, V, tolerance, power, fill, eps, images=None):
    images = dev(s["images"]) if images is None else images
    return mesh_color.project_colors(dev(s["vertices"][:V]), dev(s["normals"][:V]), images, dev(s["depths"]), dev(s["focals"]),
                                     dev(s["scales"]), dev(s["cam2world"]), tolerance, power, fill, eps)


GRIDS = [(2, 2, 2, 2), (5, 3, 12, 7), (32, 16, 64, 32)]
PROJECT_CASES = [(1, GRIDS[0], 257, 2, 0.05), (5, GRIDS[0], 1, 1, 0.01), (1, GRIDS[1], 1, 8, 0.05), (5, GRIDS[1], 257, 2, 0.01),
                 (5, GRIDS[1], 4000, 1, 0.05), (1, GRIDS[2], 4000, 2, 0.05), (5, GRIDS[2], 4000, 2, 0.05), (5, GRIDS[2], 4000, 8, 0.01),
                 (5, GRIDS[2], 257, 1, 0.01), (1, GRIDS[2], 1, 2, 0.01)]


@pytest.mark.parametrize("K,grid,V,power,tolerance", PROJECT_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_projection_against_the_restatement(K, grid, V, power, tolerance):
    fill, eps = 0.25, 1e-3
    s = scene_pool(K, *grid, tolerance, max(V, POOL), seed=K + V + power)
    n = len(s["vertices"])
    c64, cov64, num64 = run_reference(s, n, tolerance, power, fill, eps, f64)
    c32, cov32, num32 = run_reference(s, n, tolerance, power, fill, eps, f32)
    colors, coverage = run_kernel(s, V, tolerance, power, fill, eps)
    assert colors.shape == (V, 3) and coverage.shape == (V,) and colors.dtype == coverage.dtype == torch.float32
    colors, coverage = colors.cpu().numpy().astype(f64), coverage.cpu().numpy().astype(f64)
    numerator = colors * (coverage + eps)[:, None] - eps * fill
    seen = cov64 >= 0.1
    cov_err, cov_bar = np.abs(coverage - cov64[:V]).max(), bar_of(cov32, cov64)
    num_err, num_bar = np.abs(numerator - num64[:V]).max(), bar_of(num32, num64)
    col_err = np.abs(colors - c64[:V])[seen[:V]].max(initial=0.0)
    col_bar = bar_of(c32[seen], c64[seen]) if seen.any() else 0.0
    print(f"project K={K} grid={grid} V={V} power={power} tol={tolerance}: coverage err {cov_err:.2e} bar {cov_bar:.2e}; numerator err "
          f"{num_err:.2e} bar {num_bar:.2e}; colour err {col_err:.2e} bar {col_bar:.2e} on {int(seen[:V].sum())} of {V} (max coverage "
          f"{cov64.max():.2f}, {int((cov64 > 0).sum())} of {n} seen)")
    assert (cov64 > 0).sum() >= n // 16 and seen.sum() >= 4              # the case is not empty
    assert cov_err <= cov_bar and num_err <= num_bar and col_err <= col_bar
    if n >= 8 and V >= 8:
        assert (coverage[1:5] == 0).all() and np.allclose(colors[1:5], fill, rtol=1e-6, atol=0)


def test_projection_twice_noncontiguous_nonfinite_and_empty():
    K, grid, V, tolerance, fill, eps = 5, GRIDS[1], 4000, 0.05, -0.5, 1e-3
    s = scene_pool(K, *grid, tolerance, V, seed=3)
    a = run_kernel(s, V, tolerance, 2, fill, eps)
    b = run_kernel(s, V, tolerance, 2, fill, eps)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert float(a[1].max()) > 0.5
    # channels-last images are a non-contiguous [K,3,H,W] view: copied
    images = dev(s["images"])
    view = images.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not view.is_contiguous() and torch.equal(view, images)
    c = run_kernel(s, V, tolerance, 2, fill, eps, images=view)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    # NaN and +-inf positions: coverage 0 and the fill colour; every other row keeps its bits
    clean = s["vertices"].copy()
    rows = [0, 63, 64, 255, 256, 3999]
    for r, (column, value) in zip(rows, [(0, np.nan), (1, np.inf), (2, -np.inf), (0, np.inf), (1, np.nan), (2, np.nan)]):
        s["vertices"][r, column] = value
    s["vertices"][64] = np.nan
    colors, coverage = run_kernel(s, V, tolerance, 2, fill, eps)
    keep = torch.ones(V, dtype=torch.bool)
    keep[rows] = False
    assert (coverage[rows] == 0).all() and torch.allclose(colors[rows], torch.full_like(colors[rows], fill), rtol=1e-6, atol=0)
    assert torch.equal(colors[keep], a[0][keep]) and torch.equal(coverage[keep], a[1][keep])
    s["vertices"] = clean
    colors, coverage = run_kernel(s, 0, tolerance, 2, fill, eps)
    assert colors.shape == (0, 3) and coverage.shape == (0,) and colors.device.type == "cuda"
