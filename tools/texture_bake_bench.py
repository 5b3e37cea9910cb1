"""Time the texture bake.

h3d_mesh_bake_texture alone, on the capsule surface of tools/isosurface_bench.py at 64 nodes along the longest axis (a 45 x 64 x 45
grid: the mesh resolution one wants for a file that opens quickly), a texture of --size 2048 texels a side and K = 8 views of 512 x 256
over a 64 x 32 render grid, set up as tools/mesh_attributes_bench.py sets up its views: cameras on a +-30 degree pan looking at the
capsule, depth maps splatted from the vertices, smooth images.  Device events, median of --reps calls after warm-up, beside the floor
of writing the outputs -- 16 S^2 bytes (12 of colour, 4 of coverage per texel) at the measured streaming rate; the mesh and the views
are small beside that and stay in the caches.  h3d_mesh_project_colors on the same mesh and views stands beside it: what the per-vertex
colours cost.  No time here is a pass / fail bar.  Writes one JSON (profiles/texture_bake.json).

    python tools/texture_bake_bench.py [--size 2048] [--views 8] [--reps 10] [--out profiles/texture_bake.json]
"""
import argparse
import importlib
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from isosurface_bench import HBM_MEASURED, capsule, timed  # noqa: E402
from mesh_attributes_bench import pan_cameras, splat_depths  # noqa: E402

L = importlib.import_module("3dhumangan_amd._lib")
iso = importlib.import_module("3dhumangan_amd.lib.components.isosurface")
mesh_color = importlib.import_module("3dhumangan_amd.lib.components.mesh_color")
mesh_texture = importlib.import_module("3dhumangan_amd.lib.components.mesh_texture")

GRID = (45, 64, 45)


def measure(S, K, reps, dev):
    volume = capsule(GRID, dev)
    vertices, faces = iso.marching_tetrahedra(volume, 0.0)
    normals = iso.vertex_normals(volume, vertices)
    V, T = len(vertices), len(faces)
    cell, per_row = mesh_texture.atlas_layout(T, S)
    H, W, h, w = 512, 256, 64, 32
    out = {"grid": list(GRID), "vertices": V, "triangles": T, "texture": S, "cell": cell, "cells_per_row": per_row, "views": K,
           "image": [H, W], "render_grid": [h, w]}
    centre = torch.tensor([(n - 1) / 2 for n in GRID], device=dev)
    focal, distance = 2.0, 1.3 * max(GRID)
    cams = pan_cameras(centre, distance, K, math.radians(30), dev)
    depths = splat_depths(vertices, cams, focal, h, w, far=2 * distance)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, device=dev), torch.linspace(0, 1, W, device=dev), indexing="ij")
    images = torch.stack([torch.stack([torch.sin(0.7 * k + c + 3 * xx) * torch.cos(2 * yy + c) for c in range(3)]) for k in range(K)]).contiguous()
    table = torch.from_numpy(mesh_color.camera_table(torch.full((K,), focal), cams)).to(dev)
    texture, coverage = torch.empty(S, S, 3, device=dev), torch.empty(S, S, device=dev)
    colors, seen = torch.empty(V, 3, device=dev), torch.empty(V, device=dev)
    tolerance = 1.0                                         # voxels: about one render pixel's width at this distance
    lib = L.load()

    def bake():
        L.check(lib.h3d_mesh_bake_texture(L.ptr(vertices), L.ptr(normals), V, L.ptr(faces), T, S, L.ptr(images), K, H, W, L.ptr(depths), h,
                                          w, L.ptr(table), tolerance, 2, 0.0, 1e-3, L.ptr(texture), L.ptr(coverage), L.stream_handle()),
                "bake")

    def vertex_colours():
        L.check(lib.h3d_mesh_project_colors(L.ptr(vertices), L.ptr(normals), V, L.ptr(images), K, H, W, L.ptr(depths), h, w, L.ptr(table),
                                            tolerance, 2, 0.0, 1e-3, L.ptr(colors), L.ptr(seen), L.stream_handle()), "colors")

    out["bake_ms"], out["bake_ms_all"] = timed(bake, reps)
    out["vertex_colours_ms"], out["vertex_colours_ms_all"] = timed(vertex_colours, reps)
    owned = int(min(T, 2 * per_row * per_row)) * cell * cell // 2
    out["owned_texel_share"] = owned / (S * S)
    out["covered_texel_share"] = float((coverage > 0).float().mean())
    out["floor_ms"] = 16 * S * S / HBM_MEASURED * 1e3
    out["times_floor"] = out["bake_ms"] / out["floor_ms"]
    out["ns_per_texel"] = out["bake_ms"] * 1e6 / (S * S)
    out["ns_per_texel_and_view"] = out["ns_per_texel"] / K
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_bake.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    result = {"device": torch.cuda.get_device_name(0), "hbm_rate_used_for_floors_bytes_per_s": HBM_MEASURED}
    with torch.no_grad():
        result["bake_capsule_64"] = measure(a.size, a.views, a.reps, "cuda")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
