"""Time the dataset ingest.

(a) The fused kernel (lib/data/ingest.ingest, csrc/ingest.hip) against the torch composition (ingest_torch) on the device: source
    1024x512 to 512x256 and to 256x128, B = 4 and 32, both warmed up, then timed in alternation with device events.  The bytes a
    call needs at the least -- 5 source bytes per source pixel read once, 24 bytes per output pixel written -- over its time give
    the achieved rate.  At B = 4 a call is a few microseconds of traffic: expect launch overhead, not bandwidth.
(b) DatasetTrainingSource alone over a written 64-item dataset at 1024x512 (seeded noise added to the images so that the PNGs
    decode like photographs, not like smooth gradients), batch 4, 4 workers; the consumer only synchronises.  Steady-state
    items/s with prefetch on and off and the host time inside batches(), next to the trainer's need of 4 / iteration time
    (--iteration-ms: config 4's iteration on the same lease, from `bench.py --mode trainstep`).  Reported, not gated: the host
    CPUs are shared.
--parity writes the worst error of the fused kernel against the float64 restatement over the cases of tests/test_gpu_ingest.py
(profiles/ingest_parity.json).

    python tools/ingest_bench.py [--calls 200] [--warmup 20] [--source] [--parity] [--iteration-ms 130]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ing = importlib.import_module("3dhumangan_amd.lib.data.ingest")

HBM_MEASURED = 6.29e12


def median(xs):
    return sorted(xs)[len(xs) // 2]


def alternate(fns, calls, warmup):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in fns}
    for _ in range(calls):
        for name, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            ev[name].append((s, e))
    torch.cuda.synchronize()
    return {k: [s.elapsed_time(e) for s, e in v] for k, v in ev.items()}


def bench_op(B, src, size, calls, warmup):
    g = torch.Generator().manual_seed(B + size[0])
    rgb = torch.randint(0, 256, (B, *src, 3), generator=g, dtype=torch.uint8).cuda()
    mask = (torch.randint(0, 3, (B, *src), generator=g) * 127).to(torch.uint8).cuda()
    seg = torch.randint(0, 25, (B, *src), generator=g, dtype=torch.uint8).cuda()
    a, b = ing.ingest(rgb, mask, seg, size), ing.ingest_torch(rgb, mask, seg, size)
    assert torch.equal(a["body_segments"], b["body_segments"])
    ms = alternate({"hip": lambda: ing.ingest(rgb, mask, seg, size), "torch": lambda: ing.ingest_torch(rgb, mask, seg, size)}, calls, warmup)
    med = {k: median(v) for k, v in ms.items()}
    need = B * (src[0] * src[1] * 5 + size[0] * size[1] * 24)
    rate = need / (med["hip"] * 1e-3)
    return {"B": B, "source": list(src), "size": list(size), "calls": calls, "hip_median_ms": med["hip"], "torch_median_ms": med["torch"],
            "hip_min_ms": min(ms["hip"]), "torch_min_ms": min(ms["torch"]), "speedup": med["torch"] / med["hip"], "necessary_bytes": need,
            "achieved_bytes_per_s": rate, "fraction_of_measured_hbm_rate": rate / HBM_MEASURED,
            "max_abs_image_difference": float((a["images"] - b["images"]).abs().max())}


def bench_source(iteration_ms, length=64, batch=4, workers=4, steps=40):
    from PIL import Image
    synthetic = importlib.import_module("3dhumangan_amd.synthetic")
    data = importlib.import_module("3dhumangan_amd.lib.data")
    out = {"dataset": f"{length} items at 1024x512, batch {batch}, {workers} workers, ingest to 512x256"}
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        synthetic.write_example_dataset(root, length=length, height=1024, width=512, seed=0)
        rng = np.random.default_rng(0)
        for name in sorted(os.listdir(os.path.join(root, "images"))):
            path = os.path.join(root, "images", name)
            im = np.asarray(Image.open(path)).astype(np.int16) + rng.integers(-8, 9, (1024, 512, 3))
            Image.fromarray(im.clip(0, 255).astype(np.uint8)).save(path)
        out["write_seconds"] = time.perf_counter() - t0
        ds = data.SHHQDataset(dataroot=root, dataset_length=length, gen_height=512, gen_width=256, latent_dim=512, joints=list(range(24)),
                              smpl_model=os.path.join(root, "smpl_model.npz"))
        t0 = time.perf_counter()
        for i in range(8):
            ds.raw(i)
        out["raw_item_ms_one_thread"] = (time.perf_counter() - t0) / 8 * 1e3
        for name, prefetch in (("prefetch_2", 2), ("prefetch_0", 0)):
            src = data.DatasetTrainingSource(ds, seed=0, num_workers=workers, prefetch=prefetch)
            for g in range(4):
                src.batches(batch, g, "cuda")
            torch.cuda.synchronize()
            src.host_seconds = 0.0
            t0 = time.perf_counter()
            for g in range(4, 4 + steps):
                src.batches(batch, g, "cuda")
                torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out[name] = {"items_per_s": steps * batch / dt, "ms_per_batch": dt / steps * 1e3, "host_ms_inside_batches": src.host_seconds / steps * 1e3}
            src.close()
        # a consumer that works for iteration_ms between requests: what the trainer's thread waits for with the look-ahead running
        if iteration_ms:
            src = data.DatasetTrainingSource(ds, seed=0, num_workers=workers, prefetch=2)
            for g in range(3):
                src.batches(batch, g, "cuda")
            src.host_seconds = 0.0
            for g in range(3, 3 + 12):
                time.sleep(iteration_ms * 1e-3)
                src.batches(batch, g, "cuda")
                torch.cuda.synchronize()
            out["behind_a_busy_consumer"] = {"consumer_ms": iteration_ms, "host_ms_inside_batches": src.host_seconds / 12 * 1e3}
            src.close()
    if iteration_ms:
        out["trainer_need_items_per_s"] = batch / (iteration_ms * 1e-3)
        out["iteration_ms"] = iteration_ms
    return out


def parity_table():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _ingest_reference import SHAPES, ingest_f64, make_inputs
    worst, rows = 0.0, []
    for src, size in SHAPES + [((32, 16), (16, 8)), ((5, 24), (10, 12))]:
        e = 0.0
        for B in (1, 3):
            for geo_only in (False, True):
                for kind in ("zero", "full", "random"):
                    arrays = make_inputs(B, src[0], src[1], seed=11 * B + src[0], mask_kind=kind)
                    wi, wm, ws = ingest_f64(*arrays, size, geo_only)
                    got = ing.ingest(*[torch.from_numpy(a).cuda() for a in arrays], size, geo_only)
                    assert np.array_equal(got["body_segments"].cpu().numpy(), ws)
                    e = max(e, float(np.abs(got["images"].cpu().numpy().astype(np.float64) - wi).max()),
                            float(np.abs(got["masks"].cpu().numpy().astype(np.float64) - wm).max()))
        rows.append({"source": list(src), "size": list(size), "max_abs_error": e})
        worst = max(worst, e)
    return {"bar": 1e-6, "derivation": "values in [-1, 1]; two roundings in the normalisation, six in three lerps, lambda exact to one rounding: "
            "at most 8 x 2^-24 = 4.8e-7", "body_segments": "bit-equal in every case", "max_abs_error": worst, "shapes": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--source", action="store_true")
    ap.add_argument("--iteration-ms", type=float, default=0.0)
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--json", type=str, default=os.path.join(ROOT, "profiles", "ingest_bench.json"))
    ap.add_argument("--parity-json", type=str, default=os.path.join(ROOT, "profiles", "ingest_parity.json"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ingest_bench needs a GPU: a CPU run says nothing about these times")
    out = {"op": []}
    for size in ((512, 256), (256, 128)):
        for B in (4, 32):
            r = bench_op(B, (1024, 512), size, opt.calls, opt.warmup)
            out["op"].append(r)
            print(f"1024x512 -> {size[0]}x{size[1]} B={B:2d}: HIP {r['hip_median_ms'] * 1e3:8.1f} us | torch {r['torch_median_ms'] * 1e3:8.1f} us | "
                  f"x{r['speedup']:.2f} | {r['achieved_bytes_per_s'] / 1e12:.2f} TB/s", flush=True)
    out["fused_not_slower_anywhere"] = all(r["speedup"] >= 1 for r in out["op"])
    if opt.source:
        out["source"] = bench_source(opt.iteration_ms)
        print(json.dumps(out["source"]), flush=True)
    with open(opt.json, "w") as f:
        json.dump(out, f, indent=1)
    if opt.parity:
        t = parity_table()
        with open(opt.parity_json, "w") as f:
            json.dump(t, f, indent=1)
        print(json.dumps(t), flush=True)


if __name__ == "__main__":
    main()
