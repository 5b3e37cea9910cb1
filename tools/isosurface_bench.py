"""Time the two halves of the geometry export on the flagship config (MAP3DBN512, random-init weights, the procedural body).

(a) Map3DGenerator.density_grid at --resolution (256) for one body, device events around whole calls, against the same number of
    samples in the fused render of bench.py's config 3 (96x96 rays x 64 samples, batch 16; stages geo_features + render_fused of
    the same generator, per-stage events).  The grid pays for what the render never writes: the [N, 31] geometry features and the
    [N, F + 4] field output of every chunk.
(b) marching_tetrahedra on that grid, launch by launch -- count, the two prefix sums with the one host read, emit -- at two levels:
    the grid's own median (random-init weights: a surface through half of the volume, far more triangles than a body has) and a
    capsule's distance field in the same grid (a body-sized smooth surface).  Against the floor: the bytes each launch needs at
    the least over the measured HBM rate.
        count: 4 N read, 4 N + 4 C written             emit: 4 N + 4 N + 8 C read, 12 V + 12 T written        (N nodes, C cells)
Writes one JSON (profiles/isosurface.json).

    python tools/isosurface_bench.py [--resolution 256] [--reps 10] [--out profiles/isosurface.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the flagship generator and its inputs)

L = importlib.import_module("3dhumangan_amd._lib")
iso = importlib.import_module("3dhumangan_amd.lib.components.isosurface")
StageTimer = importlib.import_module("3dhumangan_amd._stages").StageTimer

HBM_MEASURED = 6.3e12          # bytes/s, achievable streaming rate of the MI355X (spec 8e12)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def timed(fn, reps, warmup=2):
    """-> (median ms, all ms) of fn() between device events; the host read inside fn, if any, is part of the time"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return median(ms), ms


def extraction(volume, level, reps):
    """The launches of lib/components/isosurface.marching_tetrahedra, timed one by one."""
    lib, dev = L.load(), volume.device
    Nx, Ny, Nz = volume.shape
    N, cells = Nx * Ny * Nz, (Nx - 1) * (Ny - 1) * (Nz - 1)
    vcount = torch.zeros(N + 1, dtype=torch.int32, device=dev)
    tcount = torch.zeros(cells + 1, dtype=torch.int32, device=dev)
    behind = lambda t: C.c_void_p(t.data_ptr() + 4)
    one = (C.c_float * 3)(1, 1, 1)

    def count():
        L.check(lib.h3d_isosurface_count(L.ptr(volume), Nx, Ny, Nz, level, behind(vcount), behind(tcount), L.stream_handle()), "count")

    def scan():
        voff, toff = torch.cumsum(vcount, 0, dtype=torch.int32), torch.cumsum(tcount, 0)
        return voff, toff, torch.stack([voff[-1].long(), toff[-1]]).tolist()

    count()
    voff, toff, (V, T) = scan()
    vertices = torch.empty(max(V, 1), 3, dtype=torch.float32, device=dev)
    faces = torch.empty(max(T, 1), 3, dtype=torch.int32, device=dev)

    def emit():
        L.check(lib.h3d_isosurface_emit(L.ptr(volume), Nx, Ny, Nz, level, one, one, L.ptr(voff), L.ptr(toff), L.ptr(vertices), V,
                                        L.ptr(faces), T, L.stream_handle()), "emit")

    whole = lambda: iso.marching_tetrahedra(volume, level)
    out = {"grid": [Nx, Ny, Nz], "level": level, "vertices": V, "triangles": T}
    stages = {"count": count, "prefix_sums_and_host_read": scan, "whole_op": whole}
    if V and T:
        stages["emit"] = emit
    for name, fn in stages.items():
        out[name + "_ms"], out[name + "_ms_all"] = timed(fn, reps)
    floor = {"count": (4 * N + 4 * N + 4 * cells) / HBM_MEASURED * 1e3, "emit": (8 * N + 8 * cells + 12 * V + 12 * T) / HBM_MEASURED * 1e3}
    out["floor_ms"] = floor
    out["times_floor"] = {k: out[k + "_ms"] / floor[k] for k in floor if k + "_ms" in out}
    return out


def capsule(shape, device):
    """distance field of a capsule along the longest axis, about a quarter of the box wide: positive inside, level 0"""
    Nx, Ny, Nz = shape
    x, y, z = torch.meshgrid(*(torch.arange(n, device=device, dtype=torch.float32) for n in shape), indexing="ij")
    c, half = [(n - 1) / 2 for n in shape], [(n - 1) / 2 for n in shape]
    axis = max(range(3), key=lambda k: shape[k])
    p = [x - c[0], y - c[1], z - c[2]]
    radius = 0.5 * min(half[k] for k in range(3) if k != axis)
    p[axis] = (p[axis].abs() - (half[axis] * 0.8 - radius)).clamp(min=0)
    return (radius - torch.sqrt(p[0] ** 2 + p[1] ** 2 + p[2] ** 2)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "isosurface.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = "cuda"
    G, cfg = bench.build_generator("MAP3DBN512", (512, 512), (96, 96), 64, dev)
    z, cond, jitter = bench.make_inputs(cfg, 16, dev)
    result = {"device": torch.cuda.get_device_name(0), "config": "MAP3DBN512, random-init weights, procedural body (6890 vertices)",
              "field_engine": G.neural_field.precision, "hbm_rate_used_for_floors_bytes_per_s": HBM_MEASURED}

    # (a) the render of config 3, per stage
    with torch.no_grad():
        for _ in range(2):
            G.forward(z, cond, jitter=jitter, **cfg)
        G.stage_timer = StageTimer()
        for _ in range(5):
            G.forward(z, cond, jitter=jitter, **cfg)
        torch.cuda.synchronize()
        stages = {k: v[0] for k, v in G.stage_timer.summary_ms().items()}
        G.stage_timer = None
    samples = 16 * cfg["render_height"] * cfg["render_width"] * cfg["num_steps"]
    render_ms = stages.get("geo_features", 0.0) + stages.get("render_fused", 0.0)
    result["render_config3"] = {"samples": samples, "stage_ms": stages, "geo_plus_render_ms": render_ms,
                                "ns_per_sample": render_ms * 1e6 / samples}

    body = {k: cond[k][:1] for k in G.MESH_CONDITIONS}
    grid = lambda: G.density_grid(z[:1], body, resolution=a.resolution, **cfg)
    ms, all_ms = timed(grid, max(3, a.reps // 2), warmup=1)
    sigma, origin, spacing = grid()
    n = sigma[0].numel()
    result["density_grid"] = {"resolution": a.resolution, "grid": list(sigma.shape[1:]), "samples": n, "ms": ms, "ms_all": all_ms,
                              "ns_per_sample": ms * 1e6 / n, "spacing": float(spacing[0, 0]),
                              "render_ms_for_the_same_samples": render_ms * n / samples,
                              "times_the_render": ms / (render_ms * n / samples)}

    # (b) the extraction
    volume = sigma[0].contiguous()
    default_level = 0.6931471805599453 * cfg["num_steps"] / (cfg["ray_end"] - cfg["ray_start"])
    v, f = iso.marching_tetrahedra(volume, default_level)
    result["default_level"] = {"level": default_level, "vertices": len(v), "triangles": len(f),
                               "density_range": [float(volume.min()), float(volume.max())]}
    result["extraction_field_median"] = extraction(volume, float(volume.median()), a.reps)
    result["extraction_capsule"] = extraction(capsule(tuple(volume.shape), dev), 0.0, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({k: v for k, v in result.items()}, indent=1))


if __name__ == "__main__":
    main()
