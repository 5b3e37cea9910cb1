"""Time the two mesh-rig launches at the app's default mesh.

h3d_mesh_bind (K = 4, with normals) and h3d_mesh_pose (n = 8 poses, with normals) on the capsule surface of tools/isosurface_bench.py
(about 250 k vertices in the 179 x 256 x 178 grid of a resolution-256 export) scaled into the box of the procedural body (V = 6 890, J =
24, synthetic.make_conditions), whose vertices, skin weights and bone transforms are the rig.  Device events, medians of --reps calls
after warm-up, ONE run: single measurements.  Each beside the bytes it must move over the measured streaming rate:
    bind: 24 M read (positions, normals) + 60 M written (rest positions and normals, 4 joints, 4 weights, det) + the body once
          (12 V + 4 V J + 64 J)
    pose: 56 M read (rest positions and normals, joints, weights) + 24 n M written
No time here is a pass / fail bar.  Writes one JSON (profiles/mesh_rig.json).

    python tools/mesh_rig_bench.py [--k 4] [--poses 8] [--reps 10] [--out profiles/mesh_rig.json]
"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from isosurface_bench import HBM_MEASURED, capsule, timed  # noqa: E402

iso = importlib.import_module("3dhumangan_amd.lib.components.isosurface")
mesh_rig = importlib.import_module("3dhumangan_amd.lib.components.mesh_rig")
synthetic = importlib.import_module("3dhumangan_amd.synthetic")

GRID = (179, 256, 178)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--poses", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_rig.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = "cuda"
    with torch.no_grad():
        cond = {k: v.to(dev) for k, v in synthetic.make_conditions(a.poses, 6890, seed=1).items()}
        body, weights, fk = cond["vertices"][0], cond["lbs_weights"][0], cond["fk_matrices"]
        lo, hi = body.amin(dim=0), body.amax(dim=0)
        volume = capsule(GRID, dev)
        vertices, faces = iso.marching_tetrahedra(volume, 0.0)
        normals = iso.vertex_normals(volume, vertices, (0, 0, 0), (1, 1, 1))
        top = torch.tensor([n - 1.0 for n in GRID], device=dev)
        longest = int(torch.argmax(top))
        order = [longest] + [i for i in range(3) if i != longest]              # the capsule's axis onto the body's longest
        target = [int(torch.argmax(hi - lo))] + [i for i in range(3) if i != int(torch.argmax(hi - lo))]
        X, N = torch.empty_like(vertices), torch.empty_like(normals)
        scale = float((hi - lo).max() / top.max())
        for src, dst in zip(order, target):
            X[:, dst] = (vertices[:, src] - top[src] / 2) * scale + (lo[dst] + hi[dst]) / 2
            N[:, dst] = normals[:, src]
        M, V, J = len(X), body.shape[0], weights.shape[1]
        out = {"device": torch.cuda.get_device_name(0), "hbm_rate_used_for_floors_bytes_per_s": HBM_MEASURED, "vertices": M,
               "triangles": len(faces), "smpl_vertices": V, "joints": J, "k": a.k, "poses": a.poses,
               "note": "one run, medians of --reps calls: single measurements"}
        rig = mesh_rig.bind(X, body, weights, fk[0], normals=N, k=a.k)
        out["bind_ms"], out["bind_ms_all"] = timed(lambda: mesh_rig.bind(X, body, weights, fk[0], normals=N, k=a.k), a.reps)
        out["pose_ms"], out["pose_ms_all"] = timed(
            lambda: mesh_rig.pose(rig["rest_vertices"], rig["joints"], rig["weights"], fk, rig["rest_normals"]), a.reps)
        posed, posed_normals = mesh_rig.pose(rig["rest_vertices"], rig["joints"], rig["weights"], fk, rig["rest_normals"])
        out["round_trip_max_abs"] = float((posed[0] - X).abs().max())
        out["round_trip_normals_max_abs"] = float((posed_normals[0] - N).abs().max())
        out["det_min"], out["det_max"] = float(rig["det"].min()), float(rig["det"].max())
        out["bytes"] = {"bind": 84 * M + 12 * V + 4 * V * J + 64 * J, "pose": 56 * M + 24 * a.poses * M + 64 * J * a.poses}
        out["floor_ms"] = {k: v / HBM_MEASURED * 1e3 for k, v in out["bytes"].items()}
        out["times_floor"] = {"bind": out["bind_ms"] / out["floor_ms"]["bind"], "pose": out["pose_ms"] / out["floor_ms"]["pose"]}
        out["ns_per_vertex"] = {"bind": out["bind_ms"] * 1e6 / M, "pose_per_pose": out["pose_ms"] * 1e6 / M / a.poses}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
