"""Time quadric vertex clustering (lib/components/mesh_simplify.py) on the app's default mesh.

simplify on the capsule surface of tools/isosurface_bench.py (about 250 k vertices and 501 k faces in the 179 x 256 x 178 grid of a
resolution-256 export) at cluster cells of 2, 4 and 8 voxels, on the grid's own box.  The whole call, and its parts one by one: the
three launches, the two stable sorts, and the rest of the plumbing with its host reads (unique_consecutive: C; the face mask: T').
Device events, medians of --reps calls after warm-up, ONE run: single measurements.  Each launch beside the bytes it must move at
the least over the measured streaming rate:
    cells: 12 V read, 4 V written
    faces: 12 T + 4 V read (the cluster table once), 12 T + T + 12 T written
    solve: 8 V + 12 V (the vertex list and every vertex once) + 24 T + 12 T (the record list and every face once) + 20 C read,
           12 C written -- the gathers of a face's three vertices by each of its three records are counted once
No time here is a pass / fail bar.  Writes one JSON (profiles/mesh_simplify.json).

    python tools/mesh_simplify_bench.py [--cells 2 4 8] [--reps 10] [--out profiles/mesh_simplify.json]
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
from isosurface_bench import HBM_MEASURED, capsule, timed  # noqa: E402

L = importlib.import_module("3dhumangan_amd._lib")
iso = importlib.import_module("3dhumangan_amd.lib.components.isosurface")
mesh_simplify = importlib.import_module("3dhumangan_amd.lib.components.mesh_simplify")
mesh_texture = importlib.import_module("3dhumangan_amd.lib.components.mesh_texture")

GRID = (179, 256, 178)
EXTRACTION_MS = 0.26           # marching_tetrahedra on this surface, DESIGN 4.5c (profiles/isosurface.json)


def parts(vertices, faces, cell, counts, reps):
    """the steps of mesh_simplify.simplify, timed one by one on tensors that the steps before them made"""
    lib, dev, stream = L.load(), vertices.device, L.stream_handle()
    V, T = len(vertices), len(faces)
    origin = (C.c_float * 3)(0.0, 0.0, 0.0)
    cells = torch.empty(V, dtype=torch.int32, device=dev)
    launch_cells = lambda: L.check(lib.h3d_mesh_cluster_cells(L.ptr(vertices), V, origin, 1.0 / cell, *counts, L.ptr(cells), stream), "cells")  # noqa: E731
    launch_cells()
    sort_cells = lambda: torch.sort(cells, stable=True)                                            # noqa: E731
    sorted_cells, vertex_order = sort_cells()

    def table_and_offsets():
        table, inverse, per_cluster = torch.unique_consecutive(sorted_cells, return_inverse=True, return_counts=True)
        cluster = torch.empty(V, dtype=torch.int32, device=dev)
        cluster[vertex_order] = inverse.to(torch.int32)
        offsets = torch.zeros(table.shape[0] + 1, dtype=torch.int64, device=dev)
        torch.cumsum(per_cluster, 0, out=offsets[1:])
        return table, cluster, offsets

    table, cluster, vertex_offsets = table_and_offsets()
    n = table.shape[0]
    mapped = torch.empty(T, 3, dtype=torch.int32, device=dev)
    keep, keys = torch.empty(T, dtype=torch.bool, device=dev), torch.empty(3 * T, dtype=torch.int32, device=dev)
    launch_faces = lambda: L.check(lib.h3d_mesh_cluster_faces(L.ptr(faces), T, L.ptr(cluster), V, L.ptr(mapped), L.ptr(keep), L.ptr(keys),  # noqa: E731
                                                              stream), "faces")
    launch_faces()
    sort_keys = lambda: torch.sort(keys, stable=True)                                              # noqa: E731
    sorted_keys, record_order = sort_keys()
    segment = lambda: torch.searchsorted(sorted_keys, torch.arange(n + 1, dtype=torch.int32, device=dev))      # noqa: E731
    record_offsets = segment()
    out = torch.empty(n, 3, dtype=torch.float32, device=dev)
    launch_solve = lambda: L.check(lib.h3d_mesh_cluster_solve(L.ptr(vertices), V, L.ptr(faces), T, L.ptr(vertex_order),       # noqa: E731
                                                              L.ptr(vertex_offsets), L.ptr(record_order), L.ptr(record_offsets),
                                                              L.ptr(table), n, origin, cell, *counts, 1e-2, 1.0, L.ptr(out), stream), "solve")
    mask = lambda: mapped[keep]                                                                    # noqa: E731
    kept = len(mask())
    steps = {"cells_kernel": launch_cells, "sort_cells": sort_cells, "cluster_table_and_host_read": table_and_offsets,
             "faces_kernel": launch_faces, "sort_keys": sort_keys, "record_offsets": segment, "solve_kernel": launch_solve,
             "face_mask_and_host_read": mask}
    res = {"clusters": n, "faces_kept": kept}
    for name, fn in steps.items():
        res[name + "_ms"], res[name + "_ms_all"] = timed(fn, reps)
    res["bytes"] = {"cells_kernel": 16 * V, "faces_kernel": 37 * T + 4 * V, "solve_kernel": 20 * V + 36 * T + 32 * n}
    res["floor_ms"] = {k: b / HBM_MEASURED * 1e3 for k, b in res["bytes"].items()}
    res["times_floor"] = {k: res[k + "_ms"] / res["floor_ms"][k] for k in res["bytes"]}
    res["records_per_cluster"] = 3 * T / n
    res["solve_ns_per_record"] = res["solve_kernel_ms"] * 1e6 / (3 * T)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=float, nargs="+", default=[2.0, 4.0, 8.0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_simplify.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = "cuda"
    with torch.no_grad():
        vertices, faces = iso.marching_tetrahedra(capsule(GRID, dev), 0.0)
        V, T = len(vertices), len(faces)
        out = {"device": torch.cuda.get_device_name(0), "hbm_rate_used_for_floors_bytes_per_s": HBM_MEASURED, "grid": list(GRID),
               "vertices": V, "triangles": T, "atlas_cell_at_2048": mesh_texture.atlas_layout(T, 2048)[0],
               "extraction_ms_of_DESIGN_4_5c": EXTRACTION_MS, "note": "one run, medians of --reps calls: single measurements", "cells": {}}
        for cell in a.cells:
            counts = [int(math.floor((n - 1) / cell)) + 1 for n in GRID]
            whole = lambda: mesh_simplify.simplify(vertices, faces, cell, origin=(0.0, 0.0, 0.0), counts=counts)      # noqa: E731
            small, kept, _ = whole()
            res = {"cluster_grid": counts, "vertices_out": len(small), "triangles_out": len(kept), "reduction": T / max(len(kept), 1),
                   "atlas_cell_at_2048": mesh_texture.atlas_layout(len(kept), 2048)[0]}
            res["whole_op_ms"], res["whole_op_ms_all"] = timed(whole, a.reps)
            res["times_the_extraction"] = res["whole_op_ms"] / EXTRACTION_MS
            res.update(parts(vertices, faces, cell, counts, a.reps))
            assert res["clusters"] == len(small) and res["faces_kept"] == len(kept)
            out["cells"][f"{cell:g}"] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
