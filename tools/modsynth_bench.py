"""Time the fused synthesis engine of spatial_normalization="none" (h3d_synthesis_mod, csrc/synthesis_mod.hip) against the same
network composed layer by layer from the stand-alone entry points (h3d_bilinear_resize_cl, 18 x h3d_modconv1x1, torch for
LeakyReLU / skip / ToRGB: modsynth_pack.LayerwiseModSynthesis).

Shape: MAP3DBN512 native (512 x 256 image, 96 x 48 render, width 256, mod_blocks = [0, 1, 2], "mixed"), B = 4.
Protocol: both paths in ONE process on one device; warm-up, then device events around every call, median of >= 20 calls; the
layer-by-layer path is timed twice, before and after the fused one, and the difference of its two medians is the run-to-run
spread the comparison is held against.  The fused time includes the per-forward host folding (modulation maps, per-image vectors).

    python tools/modsynth_bench.py [--calls 20] [--warmup 3] [--batch 4] [--json profiles/modsynth_bench.json]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gens = importlib.import_module("3dhumangan_amd.lib.generators")
impl = importlib.import_module("3dhumangan_amd.lib.implicit_funcitions")
configs = importlib.import_module("3dhumangan_amd.configs")
pack = importlib.import_module("3dhumangan_amd.lib.generators.modsynth_pack")


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "calls": calls}


def git_head():
    try:
        return subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--json", type=str, default=os.path.join(ROOT, "profiles", "modsynth_bench.json"))
    opt = ap.parse_args()
    calls = max(opt.calls, 20)

    cfg = {k: v for k, v in configs.MAP3DBN512.items() if isinstance(k, str)}
    cfg.update(spatial_normalization="none", map3d_mode="mixed", mod_blocks=[0, 1, 2], dataset_length=4)
    cfg["neural_field_cls"] = impl.COORDCONCATSIREN
    torch.manual_seed(0)
    G = gens.Map3DGenerator(**cfg).to("cuda").eval()
    G.set_device("cuda")
    B, C = opt.batch, cfg["hidden_dim"]
    hw, HW = (cfg["render_height"], cfg["render_width"]), (cfg["gen_height"], cfg["gen_width"])
    fmap = torch.rand(B, hw[0] * hw[1], C, device="cuda")
    styles = torch.randn(B, C, device="cuda")
    plan = G.synthesis_plan("cuda")
    hand = pack.LayerwiseModSynthesis(G.state_dict(), "synthesis_network", "synthesis_input", cfg["synthesis_blocks"],
                                      cfg["mod_blocks"], cfg["map3d_mode"], "cuda")
    fused = lambda: plan.run(fmap, styles, hw, HW)
    layerwise = lambda: hand(fmap, styles, hw, HW)

    a, b = fused(), layerwise()
    err = float((a - b).abs().max() / b.abs().max())
    del a, b
    b1 = timed(layerwise, calls, opt.warmup)
    f = timed(fused, calls, opt.warmup)
    b2 = timed(layerwise, calls, opt.warmup)
    base = 0.5 * (b1["median_ms"] + b2["median_ms"])
    spread = abs(b1["median_ms"] - b2["median_ms"])
    gemms = 2 * len(plan.pixel_ids) + len(plan.vec_ids)
    flop = 2.0 * plan.HdP * plan.HdP * gemms * B * HW[0] * HW[1]
    res = {"shape": {"config": "MAP3DBN512", "B": B, "image": list(HW), "render": list(hw), "width": C,
                     "mod_blocks": cfg["mod_blocks"], "map3d_mode": cfg["map3d_mode"]},
           "fused": f, "layerwise_first": b1, "layerwise_second": b2,
           "layerwise_median_ms": base, "layerwise_spread_ms": spread, "ratio_layerwise_over_fused": base / f["median_ms"],
           "fused_not_slower": f["median_ms"] <= base + spread,
           "per_pixel_gemms_fused": gemms, "per_pixel_gemms_layerwise": 54, "flop_issued_fused": flop,
           "fused_tflops": flop / (f["median_ms"] * 1e-3) / 1e12, "fused_vs_layerwise_rel_err": err,
           "device": torch.cuda.get_device_name(0), "git_head": git_head()}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(opt.json)), exist_ok=True)
    with open(opt.json, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
