"""Time h3d_mesh_rasterize (csrc/mesh_raster.hip) on the procedural SMPL-sized mesh (synthetic.tube_body: F = 13 776) at
512 x 256 for B in {1, 4, 32}: device events around each call after warm-up, every output written (pix_to_face, zbuf, bary,
segments, semantics).  Also prints the bytes the design moves: the raster launch streams every face box (8 B) once per tile.

    python tools/raster_bench.py [--calls 50] [--warmup 5] [--json out.json]
"""
import argparse
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
_lib = importlib.import_module("3dhumangan_amd._lib")
synthetic = importlib.import_module("3dhumangan_amd.synthetic")
conditions = importlib.import_module("3dhumangan_amd.lib.data.conditions")


def bench(B, H, W, calls, warmup):
    cond, faces, labels = synthetic.make_mesh_conditions(B, seed=0, scale=0.8)
    hs = torch.linspace(-1.0, 2.0, B)
    view = conditions.CameraPreprocessor().forward_with_rotation(cond, hs, torch.zeros(B), torch.zeros(B), gen_height=H, gen_width=W)
    dev = torch.device("cuda")
    verts = cond["vertices"].to(dev).contiguous()
    R = view["raster_rotation"].to(dev).contiguous()
    T = conditions.raster_translation(view).to(dev).contiguous()
    f32 = faces.to(dev, torch.int32).contiguous()
    lab = labels.to(dev, torch.int32).contiguous()
    table = cond["tpose_vertices"][0].to(dev).contiguous()
    V, F = verts.shape[1], f32.shape[0]
    lib = _lib.load()
    ws = torch.empty(int(lib.h3d_mesh_raster_bytes(B, F)), dtype=torch.uint8, device=dev)
    pix = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    zbuf = torch.empty(B, H, W, device=dev)
    bary = torch.empty(B, H, W, 3, device=dev)
    seg = torch.empty(B, H, W, dtype=torch.int64, device=dev)
    sem = torch.empty(B, 3, H, W, device=dev)
    P = _lib.ptr

    def call():
        rc = lib.h3d_mesh_rasterize(P(verts), P(f32), P(R), P(T), -conditions.FOCAL_RASTER, P(lab), P(table), P(pix), P(zbuf), P(bary),
                                    P(seg), P(sem), P(ws), B, V, F, H, W, _lib.stream_handle())
        _lib.check(rc, "h3d_mesh_rasterize")

    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        call()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    box_stream = tiles * B * F * 8
    setup = B * F * (12 + 36 + 8 + 64)
    out_bytes = B * H * W * (4 + 4 + 12 + 8 + 12)
    return {"B": B, "H": H, "W": W, "F": F, "V": V, "calls": calls, "median_ms": ms[len(ms) // 2], "min_ms": ms[0],
            "max_ms": ms[-1], "box_stream_bytes": box_stream, "setup_bytes": setup, "output_bytes": out_bytes,
            "covered_fraction": float((pix >= 0).float().mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 32])
    ap.add_argument("--json", type=str, default=None)
    opt = ap.parse_args()
    rows = []
    for B in opt.batches:
        r = bench(B, 512, 256, max(opt.calls, 20), opt.warmup)
        rows.append(r)
        print(f"B={B:3d} {r['H']}x{r['W']} F={r['F']}: median {r['median_ms'] * 1e3:8.1f} us (min {r['min_ms'] * 1e3:.1f}, max "
              f"{r['max_ms'] * 1e3:.1f}) | box stream {r['box_stream_bytes'] / 1e6:.1f} MB, setup {r['setup_bytes'] / 1e6:.1f} MB, "
              f"outputs {r['output_bytes'] / 1e6:.1f} MB | covered {r['covered_fraction']:.3f}", flush=True)
    if opt.json:
        with open(opt.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
