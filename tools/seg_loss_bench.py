"""Time the fused segmentation loss (csrc/seg_loss.hip through losses.segmentation_loss_fused) against the torch composition
(losses.segmentation_loss), forward + backward, in the layout the discriminator hands over: fp32 logits, the last L = 26 of
L + 3 channels of a channels-last tensor, B = 4, at 512x256 and 256x128.  Both sides warmed up, then timed in alternation
(device events around each call, the device synchronised before the medians are taken).  The bytes the fused op needs at the
least -- the logits once per pass and dlogits once, computed from the shapes -- over its time give the achieved rate, reported
as a fraction of the HBM rate (6.29 TB/s measured by a float4 copy, 8.0 TB/s specified).

--iteration also times config 4's whole adversarial iteration (bench.py's trainstep set-up, B = 4, fp32) with the torch loss
and with the fused one, alternating: what the three loss calls per iteration cost inside it.
--parity writes the worst ratio to tests/test_gpu_seg_loss.py's bar per mode and layout (profiles/seg_loss_parity.json).

    python tools/seg_loss_bench.py [--calls 50] [--warmup 10] [--iteration] [--parity] [--json profiles/seg_loss_bench.json]
"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
losses = importlib.import_module("3dhumangan_amd.lib.trainers.losses")

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12


def median(xs):
    return sorted(xs)[len(xs) // 2]


def alternate(fns, calls, warmup):
    """{name: fn} -> {name: [ms per call]}: all warmed up, then one call of each in turn, `calls` times"""
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


def bench_op(B, L, H, W, calls, warmup, mode="cross_entropy_balanced"):
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(H)
    y = torch.randn(B, H, W, L + 3, generator=g).to(dev).permute(0, 3, 1, 2)            # the discriminator's last activation
    x = y[:, 3:].detach().requires_grad_(True)                                          # y[:, semantic_dim:]
    gt = torch.randint(0, L, (B, H, W), generator=g).to(dev)

    def run(fn):
        loss = fn(x, gt, L, None, mode)[0]
        return loss, torch.autograd.grad(loss, x)[0]

    (la, ga), (lb, gb) = run(losses.segmentation_loss_fused), run(losses.segmentation_loss)
    ms = alternate({"hip": lambda: run(losses.segmentation_loss_fused), "torch": lambda: run(losses.segmentation_loss)}, calls, warmup)
    med = {k: median(v) for k, v in ms.items()}
    need = 3 * B * L * H * W * 4                     # logits read forward and backward, dlogits written
    rate = need / (med["hip"] * 1e-3)
    return {"B": B, "L": L, "H": H, "W": W, "mode": mode, "layout": f"channels-last, last {L} of {L + 3} channels, fp32", "calls": calls,
            "hip_median_ms": med["hip"], "torch_median_ms": med["torch"], "hip_min_ms": min(ms["hip"]), "torch_min_ms": min(ms["torch"]),
            "speedup": med["torch"] / med["hip"], "necessary_bytes": need, "achieved_bytes_per_s": rate,
            "fraction_of_measured_hbm_rate": rate / HBM_MEASURED, "fraction_of_spec_hbm_rate": rate / HBM_SPEC,
            "note": "forward + backward per call incl. the host side of ~10 launches; the tensors fit the 256 MiB Infinity Cache",
            "loss_difference": abs(float(la.detach()) - float(lb.detach())), "max_abs_dlogits_difference": float((ga - gb).abs().max())}


def bench_iteration(steps, warmup, batch=4):
    """config 4's iteration as `bench.py --mode trainstep` sets it up, the torch loss and the fused one alternating"""
    import bench
    trainers = importlib.import_module("3dhumangan_amd.lib.trainers")
    disc = importlib.import_module("3dhumangan_amd.lib.discriminators")
    dev = torch.device("cuda")
    G, cfg = bench.build_generator("MAP3DBN", (512, 256), (96, 48), 32, dev)
    G.train()
    z, cond, jitter = bench.make_inputs(cfg, batch, dev, seed=1234)
    torch.manual_seed(99)
    D = disc.UNetDiscriminator(**{k: v for k, v in cfg.items() if k != "neural_field_cls"}).to(dev)
    meta = {k: v for k, v in cfg.items() if k != "neural_field_cls"}
    meta.update(gan_lambda=1.0, segmentation_lambda=1.0, r1_lambda=10.0, gen_lr=5e-5, betas=(0.0, 0.9))
    opt_d = torch.optim.Adam(D.parameters(), lr=cfg.get("disc_lr", 2e-4), betas=(0.0, 0.9))
    opt_g = trainers.make_generator_optimizer(G, meta)
    g = torch.Generator().manual_seed(7)
    real = torch.randn(batch, 3, 512, 256, generator=g).clamp(-1, 1).to(dev)
    gt = torch.randint(0, max(1, cfg.get("label_dim", 1)), (batch, 512, 256), generator=g).to(dev)

    def it(seg_loss):
        def run():
            trainers.adversarial_iteration(G, D, opt_d, opt_g, z, cond, real, gt, meta, generator_kwargs=dict(jitter=jitter),
                                           grad_clip=cfg.get("grad_clip", 10.0), seg_loss=seg_loss)
            torch.cuda.synchronize()
        return run

    ms = alternate({"torch_loss": it(None), "fused_loss": it(losses.segmentation_loss_fused)}, steps, warmup)
    med = {k: median(v) for k, v in ms.items()}
    return {"workload": f"config 4 iteration (D step + G step), B = {batch}, 512x256, fp32, three loss calls per iteration", "steps": steps,
            "torch_loss_median_ms": med["torch_loss"], "fused_loss_median_ms": med["fused_loss"],
            "torch_loss_min_max_ms": [min(ms["torch_loss"]), max(ms["torch_loss"])],
            "fused_loss_min_max_ms": [min(ms["fused_loss"]), max(ms["fused_loss"])],
            "saved_ms_per_iteration": med["torch_loss"] - med["fused_loss"]}


def parity_table():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _seg_loss_reference import LAYOUTS, MODES, hard_cases, parity
    from conftest import load_golden
    cases = {k: (c["logits"].float(), c["labels"].long(), c["prior"].numpy()) for k, c in load_golden("seg_loss_modes").items()}
    cases.update(hard_cases())
    cache, table = {}, {}
    for mode in MODES:
        table[mode] = {}
        for layout in LAYOUTS:
            worst = {}
            for name, (logits, labels, prior) in cases.items():
                r = parity(losses.segmentation_loss_fused, losses.segmentation_loss, logits, labels, prior, mode, layout, "cuda", 2.5, cache, name)
                for k in ("loss", "real_prob", "dlogits"):
                    if r[k]["ratio"] >= worst.get(k, {"ratio": -1})["ratio"]:
                        worst[k] = dict(ratio=r[k]["ratio"], case=name, err=r[k]["err"], e_ref=r[k]["e_ref"])
                assert r["correct"][0] == r["correct"][1], (mode, layout, name)
            table[mode][layout] = worst
    return {"bar": "max(4 e_ref, 4 ulp of fp32 at the compared magnitude); e_ref: the torch fp32 composition's error against float64",
            "cases": len(cases), "correct_count": "equal in every case", "worst_ratio_to_the_bar": table}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iteration", action="store_true")
    ap.add_argument("--iteration-steps", type=int, default=8)
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--json", type=str, default=os.path.join(ROOT, "profiles", "seg_loss_bench.json"))
    ap.add_argument("--parity-json", type=str, default=os.path.join(ROOT, "profiles", "seg_loss_parity.json"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg_loss_bench needs a GPU: a CPU run says nothing about these times")
    out = {"op": []}
    for H, W in ((512, 256), (256, 128)):
        r = bench_op(4, 26, H, W, opt.calls, opt.warmup)
        out["op"].append(r)
        print(f"{H}x{W}: HIP {r['hip_median_ms'] * 1e3:8.1f} us | torch {r['torch_median_ms'] * 1e3:8.1f} us | x{r['speedup']:.2f} | "
              f"{r['achieved_bytes_per_s'] / 1e12:.2f} TB/s = {r['fraction_of_measured_hbm_rate']:.2f} of the measured HBM rate", flush=True)
    out["fused_faster_at_both_shapes"] = all(r["speedup"] > 1 for r in out["op"])
    if opt.iteration:
        out["iteration"] = bench_iteration(opt.iteration_steps, 2)
        print(json.dumps(out["iteration"]), flush=True)
    with open(opt.json, "w") as f:
        json.dump(out, f, indent=1)
    if opt.parity:
        t = parity_table()
        with open(opt.parity_json, "w") as f:
            json.dump(t, f, indent=1)
        print(json.dumps({m: {l: {k: round(v["ratio"], 3) for k, v in w.items()} for l, w in t["worst_ratio_to_the_bar"][m].items()}
                          for m in t["worst_ratio_to_the_bar"]}), flush=True)


if __name__ == "__main__":
    main()
