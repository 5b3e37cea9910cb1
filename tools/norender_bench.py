"""Time the fused style input of the generator without the 3D render (h3d_style_input, csrc/style_input.hip) against the
same arithmetic composed layer by layer from torch ops -- conv1x1, sin, expand + cat, conv1x1, leaky_relu (, conv1x1,
leaky_relu): the reference's SynthesisStyleInput as written -- and report the kernel's share of the whole
forward(disable_render=True).

Shape: MAP3DBN512 native (512 x 256 image, width 256), B = 4, a 512 x 256 segment map.
Protocol: everything in ONE process on one device; warm-up, then device events around every call, median of >= 20 calls; the
torch composition is timed twice, before and after the kernel, and the difference of its two medians is the run-to-run spread
the comparison is held against.  The composition is the baseline, not the code under test.

    python tools/norender_bench.py [--calls 20] [--warmup 3] [--batch 4] [--json profiles/norender_bench.json]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gens = importlib.import_module("3dhumangan_amd.lib.generators")
impl = importlib.import_module("3dhumangan_amd.lib.implicit_funcitions")
configs = importlib.import_module("3dhumangan_amd.configs")
synthetic = importlib.import_module("3dhumangan_amd.synthetic")
pack = importlib.import_module("3dhumangan_amd.lib.generators.style_input_pack")


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


def torch_composition(G):
    """SynthesisStyleInput.forward from torch ops on the module's own parameters (NCHW, as the reference runs it)."""
    m = G.synthesis_style_input
    convs = [l for l in m.network if isinstance(l, torch.nn.Conv2d)]

    def run(condition, latent):
        B, _, H, W = condition.shape
        z = pack.normalize_2nd_moment(latent)
        f = torch.sin(F.conv2d(condition, m.from_coords[0].weight, m.from_coords[0].bias))
        x = torch.cat([f, z.view(B, -1, 1, 1).expand(B, z.shape[1], H, W)], dim=1)
        for conv in convs:
            x = F.leaky_relu(F.conv2d(x, conv.weight, conv.bias), 0.2)
        return x
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--json", type=str, default=os.path.join(ROOT, "profiles", "norender_bench.json"))
    opt = ap.parse_args()
    calls = max(opt.calls, 20)

    cfg = {k: v for k, v in configs.MAP3DBN512.items() if isinstance(k, str)}
    cfg.update(dataset_length=4, disable_render=True)
    cfg["neural_field_cls"] = impl.COORDCONCATSIREN
    torch.manual_seed(0)
    G = gens.Map3DGenerator(**cfg).to("cuda").eval()
    G.set_device("cuda")
    with torch.no_grad():
        for p in G.synthesis_style_input.parameters():
            if p.dim() == 1:
                p.copy_(0.1 * torch.randn_like(p))
    B, Lw, Fw = opt.batch, cfg["latent_dim"], cfg["feature_dim"]
    HW = (cfg["gen_height"], cfg["gen_width"])
    seg = torch.randint(0, cfg["label_dim"], (B,) + HW, device="cuda")
    condition = (seg.unsqueeze(1).float() / (cfg["label_dim"] - 1) * 2 - 1).contiguous()
    z = torch.randn(B, Lw, device="cuda")
    cond = {k: v.to("cuda") for k, v in synthetic.make_conditions(B, n_vertices=256, seed=1).items()}
    cond["rasterized_segments"] = seg

    plan = G.style_input_plan("cuda")
    table = plan.bias_table(z)
    compose = torch_composition(G)
    with torch.no_grad():
        kernel = lambda: plan.launch(condition, table)
        fused = lambda: plan.run(condition, z)                   # kernel + the per-forward fold
        baseline = lambda: compose(condition, z)
        forward = lambda: G.forward(z, cond, **cfg)

        a, b = kernel(), baseline()
        err = float((a - b.flatten(2).transpose(1, 2)).abs().max() / b.abs().max())
        del a, b
        b1 = timed(baseline, calls, opt.warmup)
        k = timed(kernel, calls, opt.warmup)
        f = timed(fused, calls, opt.warmup)
        b2 = timed(baseline, calls, opt.warmup)
        whole = timed(forward, calls, opt.warmup)
    base = 0.5 * (b1["median_ms"] + b2["median_ms"])
    spread = abs(b1["median_ms"] - b2["median_ms"])
    P = B * HW[0] * HW[1]
    flop = 2.0 * P * (plan.LP * plan.FP + (plan.n_layers - 1) * plan.FP * plan.FP)
    res = {"shape": {"config": "MAP3DBN512", "B": B, "image": list(HW), "segment_map": list(HW), "latent_dim": Lw,
                     "feature_dim": Fw, "gemm_layers": plan.n_layers},
           "kernel": k, "kernel_plus_fold": f, "torch_composition_first": b1, "torch_composition_second": b2,
           "torch_composition_median_ms": base, "torch_composition_spread_ms": spread,
           "ratio_composition_over_kernel": base / k["median_ms"], "kernel_faster": k["median_ms"] < base - spread,
           "flop_issued_kernel": flop, "kernel_tflops": flop / (k["median_ms"] * 1e-3) / 1e12,
           "bytes_written_kernel": 4.0 * P * Fw, "kernel_write_gbps": 4.0 * P * Fw / (k["median_ms"] * 1e-3) / 1e9,
           "forward_disable_render": whole, "synthesis_engine": getattr(G.synthesis_plan("cuda"), "engine", None),
           "kernel_share_of_forward": k["median_ms"] / whole["median_ms"],
           "kernel_vs_composition_rel_err": err, "device": torch.cuda.get_device_name(0), "git_head": git_head()}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(opt.json)), exist_ok=True)
    with open(opt.json, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
