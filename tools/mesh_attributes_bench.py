"""Time the two mesh-attribute launches and the textured export.

(a) h3d_isosurface_normals and h3d_mesh_project_colors alone, on the capsule surface of tools/isosurface_bench.py (about 250 k vertices
    in the 179 x 256 x 178 grid of a resolution-256 export) with K = 8 views of 512 x 256 over a 64 x 32 render grid: cameras on a
    +-30 degree pan looking at the capsule, depth maps splatted from the vertices themselves (the nearest vertex per render pixel),
    smooth images.  Device events, medians of --reps calls after warm-up.  Each beside its HBM floor, bytes it must move over the
    measured streaming rate:
        normals: 12 V read + 12 V written + 4 x (distinct volume nodes in the vertices' stencils)
        colours: 24 V read + 16 V written  (+ the views, 4 K (3 H W + h w), counted whole in a second figure: how much of an image
                 a body covers is the scene's business)
(b) Map3DGenerator.extract_textured_mesh beside extract_mesh on the flagship config (MAP3DBN512 at 512 x 256 over 96 x 48 rays, 32
    steps, random-init weights, the procedural body), 8 views, at the density grid's median (random-init weights have no surface at
    the derived level: a surface through half of the volume, far more vertices than a body has).
No time here is a pass / fail bar.  Writes one JSON (profiles/mesh_attributes.json).

    python tools/mesh_attributes_bench.py [--resolution 256] [--views 8] [--reps 10] [--out profiles/mesh_attributes.json]
"""
import argparse
import ctypes as C
import importlib
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402  (the flagship generator and its inputs)
from isosurface_bench import HBM_MEASURED, capsule, timed  # noqa: E402

L = importlib.import_module("3dhumangan_amd._lib")
iso = importlib.import_module("3dhumangan_amd.lib.components.isosurface")
mesh_color = importlib.import_module("3dhumangan_amd.lib.components.mesh_color")
synthetic = importlib.import_module("3dhumangan_amd.synthetic")
geometry_export = importlib.import_module("3dhumangan_amd.lib.generators.geometry_export")

GRID = (179, 256, 178)


def stencil_nodes(vertices, shape):
    """distinct volume nodes in the 32-value stencils of the vertices (unit frame): the volume bytes the normals kernel must read"""
    N = torch.tensor(shape, device=vertices.device)
    c = torch.minimum(vertices.clamp(min=0).floor().long(), N - 2)
    seen = torch.zeros(shape, dtype=torch.bool, device=vertices.device)
    for dx in range(-1, 3):
        for dy in range(-1, 3):
            for dz in range(-1, 3):
                if sum(d in (-1, 2) for d in (dx, dy, dz)) > 1:
                    continue                                # a stencil leaves the cell along one axis at a time
                p = torch.minimum((c + torch.tensor([dx, dy, dz], device=c.device)).clamp(min=0), N - 1)
                seen[p[:, 0], p[:, 1], p[:, 2]] = True
    return int(seen.sum())


def pan_cameras(centre, distance, K, half_range, device):
    """cam2world [K,4,4] of cameras on a pan of +-half_range radians about the y axis, looking at `centre`"""
    out = []
    for a in torch.linspace(-half_range, half_range, K).tolist():
        fwd = torch.tensor([-math.sin(a), 0.0, -math.cos(a)])
        x = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0]), fwd)
        M = torch.eye(4)
        M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = x, torch.linalg.cross(fwd, x), fwd, centre.cpu() - distance * fwd
        out.append(M)
    return torch.stack(out).to(device)


def splat_depths(vertices, cam2world, focal, h, w, far):
    """[K,h,w]: per render pixel the distance of the nearest vertex that projects onto it, `far` where none does"""
    maps = []
    for M in cam2world:
        rel = vertices - M[:3, 3]
        p = rel @ M[:3, :3]                                 # world -> camera: the rotation's transpose
        u = ((focal * p[:, 0] / p[:, 2] + w / h) / (2 * w / h) * (w - 1)).round().long()
        v = ((focal * p[:, 1] / p[:, 2] + 1) / 2 * (h - 1)).round().long()
        ok = (p[:, 2] > 0) & (u >= 0) & (u < w) & (v >= 0) & (v < h)
        depth = torch.full((h * w,), far, device=vertices.device)
        depth.scatter_reduce_(0, (v * w + u)[ok], rel.norm(dim=1)[ok], reduce="amin")
        maps.append(depth.reshape(h, w))
    return torch.stack(maps)


def kernels(reps, K, dev):
    volume = capsule(GRID, dev)
    vertices, faces = iso.marching_tetrahedra(volume, 0.0)
    V, N = len(vertices), volume.numel()
    H, W, h, w = 512, 256, 64, 32
    out = {"grid": list(GRID), "vertices": V, "triangles": len(faces), "views": K, "image": [H, W], "render_grid": [h, w]}
    one = (C.c_float * 3)(1, 1, 1)
    zero = (C.c_float * 3)(0, 0, 0)
    lib = L.load()
    normals = torch.empty(V, 3, device=dev)

    def run_normals():
        L.check(lib.h3d_isosurface_normals(L.ptr(volume), *GRID, zero, one, L.ptr(vertices), V, L.ptr(normals), None, L.stream_handle()),
                "normals")

    out["normals_ms"], out["normals_ms_all"] = timed(run_normals, reps)
    nodes = stencil_nodes(vertices, GRID)
    out["normals_stencil_nodes"] = nodes

    centre = torch.tensor([(n - 1) / 2 for n in GRID], device=dev)
    focal, distance = 2.0, 1.3 * max(GRID)                  # the capsule fills about three quarters of the image height
    cams = pan_cameras(centre, distance, K, math.radians(30), dev)
    depths = splat_depths(vertices, cams, focal, h, w, far=2 * distance)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, device=dev), torch.linspace(0, 1, W, device=dev), indexing="ij")
    images = torch.stack([torch.stack([torch.sin(0.7 * k + c + 3 * xx) * torch.cos(2 * yy + c) for c in range(3)]) for k in range(K)]).contiguous()
    table = torch.from_numpy(mesh_color.camera_table(torch.full((K,), focal), cams)).to(dev)
    colors, coverage = torch.empty(V, 3, device=dev), torch.empty(V, device=dev)
    tolerance = 4.0                                         # voxels: about one render pixel's width at this distance

    def run_colors():
        L.check(lib.h3d_mesh_project_colors(L.ptr(vertices), L.ptr(normals), V, L.ptr(images), K, H, W, L.ptr(depths), h, w, L.ptr(table),
                                            tolerance, 2, 0.0, 1e-3, L.ptr(colors), L.ptr(coverage), L.stream_handle()), "colors")

    out["colors_ms"], out["colors_ms_all"] = timed(run_colors, reps)
    out["colors_covered_share"] = float((coverage > 0).float().mean())
    out["colors_mean_views_per_covered_vertex_weight"] = float(coverage[coverage > 0].mean()) if (coverage > 0).any() else 0.0
    views_bytes = 4 * K * (3 * H * W + h * w)
    floor = {"normals": (24 * V + 4 * nodes) / HBM_MEASURED * 1e3, "colors": 40 * V / HBM_MEASURED * 1e3,
             "colors_with_whole_views": (40 * V + views_bytes) / HBM_MEASURED * 1e3}
    out["floor_ms"] = floor
    out["times_floor"] = {"normals": out["normals_ms"] / floor["normals"], "colors": out["colors_ms"] / floor["colors"],
                          "colors_with_whole_views": out["colors_ms"] / floor["colors_with_whole_views"]}
    out["ns_per_vertex"] = {"normals": out["normals_ms"] * 1e6 / V, "colors": out["colors_ms"] * 1e6 / V,
                            "colors_per_view": out["colors_ms"] * 1e6 / V / K}
    return out


def whole(reps, K, resolution, dev):
    G, cfg = bench.build_generator("MAP3DBN512", (512, 256), (96, 48), 32, dev)
    z, cond, _ = bench.make_inputs(cfg, 1, dev)
    cfg = dict(cfg, truncation_psi=0.7, cache_avg_latent=True, resolution=resolution)
    pre = synthetic.SyntheticPreprocessor(torch.device(dev))
    views = []
    for a in torch.linspace(-math.radians(30), math.radians(30), K).tolist():
        angle = torch.full((1, 1), a, device=dev)
        views.append(pre.forward_with_rotation(dict(cond), angle, torch.zeros_like(angle), torch.zeros_like(angle), **cfg))
    body = {k: cond[k] for k in G.MESH_CONDITIONS}
    sigma, _, _ = G.density_grid(z, body, **cfg)
    level = float(sigma[0].median())
    plain = lambda: G.extract_mesh(z, body, level=level, **cfg)
    with_normals = lambda: G.extract_textured_mesh(z, body, [], level=level, **cfg)
    textured = lambda: G.extract_textured_mesh(z, body, views, level=level, **cfg)
    frames = lambda: [geometry_export.view_frame(G, z, view, cfg) for view in views]
    out = {"config": "MAP3DBN512 at 512x256 over 96x48 rays, 32 steps, random-init weights, procedural body", "views": K,
           "grid": list(sigma.shape[1:]), "level": level}
    n = max(3, reps // 2)
    out["extract_mesh_ms"], out["extract_mesh_ms_all"] = timed(plain, n, warmup=1)
    out["extract_textured_mesh_no_views_ms"], out["extract_textured_mesh_no_views_ms_all"] = timed(with_normals, n, warmup=1)
    out["extract_textured_mesh_ms"], out["extract_textured_mesh_ms_all"] = timed(textured, n, warmup=1)
    out["the_views_alone_ms"], out["the_views_alone_ms_all"] = timed(frames, n, warmup=1)
    mesh, = textured()
    out["vertices"], out["triangles"] = len(mesh["vertices"]), len(mesh["faces"])
    out["covered_share"] = float((mesh["coverage"] > 0).float().mean()) if len(mesh["vertices"]) else 0.0
    out["times_extract_mesh"] = out["extract_textured_mesh_ms"] / out["extract_mesh_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_attributes.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = "cuda"
    result = {"device": torch.cuda.get_device_name(0), "hbm_rate_used_for_floors_bytes_per_s": HBM_MEASURED}
    with torch.no_grad():
        result["kernels_capsule"] = kernels(a.reps, a.views, dev)
        result["whole_export"] = whole(a.reps, a.views, a.resolution, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
