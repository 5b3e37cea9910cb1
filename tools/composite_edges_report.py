#!/usr/bin/env python
"""Record the compositing edge-ray bars (tests/_composite_reference.py): for every (S, width) and mode of
tests/test_gpu_composite_edges.py the bars, the float32 restatement's own errors and every emulated defect against its bar; and,
on a GPU, the worst error of each of the six kernels (the fused renders per engine) per quantity with the ray it occurred on.

    python tools/composite_edges_report.py [--out profiles/composite_edges.json] [--cpu-only]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch                                        # noqa: E402

import _composite_reference as CR                   # noqa: E402

mode_key = lambda m: f"{m[0]}/last_back={int(m[1])}/white_back={int(m[2])}"


class Worst:
    """Per quantity: the largest error, the ray and case it occurred on, and the smallest bar / error."""

    def __init__(self):
        self.rows = {}

    def add(self, err, bar, names, case):
        for q, (e, ray) in CR.worst(err, names).items():
            r = self.rows.setdefault(q, dict(error=-1.0, headroom=float("inf")))
            if e > r["error"]:
                r.update(error=e, ray=ray, case=case, bar=bar[q])
            if bar[q] / max(e, 1e-300) < r["headroom"]:
                r.update(headroom=bar[q] / max(e, 1e-300), tightest_case=case, tightest_ray=ray)


def cpu_part(G):
    shapes = sorted({(S, 64) for S in G["forward_s"] + G["backward_s"]} | {(S, CR.ENGINE_WIDTH[e]) for e, S, _ in G["fused"]})
    bars, f32, defects = {}, {}, {}
    smallest = {}
    for S, width in shapes:
        key = f"S{S}-w{width}"
        bars[key] = {mode_key(m): CR.bars(S, width, m) for m in CR.MODES}
        f32[key] = {mode_key(m): {q: dict(error=e, ray=ray) for q, (e, ray) in CR.float32_errors(S, width, m).items()} for m in CR.MODES}
        rows = CR.defect_ratios(S, width, backward=width == 64 and S in G["backward_s"])
        defects[key] = [dict(mode=mode_key(m), defect=d, over_bar=r, quantity=q, ray=ray) for m, d, r, q, ray in rows]
        for m, d, r, q, ray in rows:
            if q not in smallest or r < smallest[q]["over_bar"]:
                smallest[q] = dict(over_bar=r, defect=d, case=key, mode=mode_key(m), ray=ray)
            print(f"{key:10s} {mode_key(m):34s} {d:22s} {r:9.3g} x bar on {q} of {ray}")
    return dict(bars=bars, float32_restatement=f32, defects=defects, smallest_defect_over_bar=smallest)


def gpu_part():
    import _composite_edges_gpu as G
    kernels = {}
    for C, fwd, bwd in ((7, "ray_integrate_vec4", "ray_integrate_bwd_kernel<4>"), (6, "ray_integrate_scalar", "ray_integrate_bwd_kernel<1>")):
        w = kernels.setdefault(fwd, Worst())
        for S in G.FORWARD_S:
            for m in CR.MODES:
                w.add(G.forward_errors(S, C, m), CR.bars(S, 64, m), CR.case_inputs(S, C)["names"], f"S={S} {mode_key(m)}")
        w = kernels.setdefault(bwd, Worst())
        for S in G.BACKWARD_S:
            for m in CR.MODES:
                w.add(G.backward_errors(S, C, m), CR.bars(S, 64, m), CR.case_inputs(S, C)["names"], f"S={S} {mode_key(m)}")
    for engine, S, hidden in G.fused_cases():
        w = kernels.setdefault(engine, Worst())
        for m, err in G.fused_errors(engine, S, hidden).items():
            w.add(err, CR.fused_bars(S, hidden, 32, engine, m), CR.fused_case(S, hidden, 32)["names"], f"S={S} hidden={hidden} {mode_key(m)}")
    S, hidden, feature, m = G.GEO_CASE
    err, listed = G.render_geo_errors()
    w = kernels.setdefault("render_geo (f16x2 + x3 relaunch)", Worst())
    w.add(err, CR.fused_bars(S, hidden, feature, "f16x2", m, geo=True), CR.fused_case(S, hidden, feature, geo=True)["names"], f"S={S} {mode_key(m)}")
    out = {k: v.rows for k, v in kernels.items()}
    out["render_geo (f16x2 + x3 relaunch)"]["units_listed_per_item"] = listed
    for k, rows in out.items():
        for q, r in rows.items():
            if isinstance(r, dict):
                print(f"{k:34s} {q:8s} worst {r['error']:.3e} (bar {r['bar']:.3e}) on {r['ray']} [{r['case']}]; tightest {r['headroom']:.2f} x under")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "composite_edges.json"))
    ap.add_argument("--cpu-only", action="store_true", help="the bars and the defect table alone (no kernel is run)")
    args = ap.parse_args()
    shapes = dict(forward_s=(1, 7, 64, 65, 128, 200), backward_s=(8, 64, 65, 200))
    if args.cpu_only:
        shapes["fused"] = [(e, S, 32) for e, w in CR.ENGINE_WIDTH.items() for S in ((8, 16, 32, 64, 96) if w == 32 else (8, 16, 32, 64, 128))]
    else:
        import _composite_edges_gpu as G
        shapes = dict(forward_s=G.FORWARD_S, backward_s=G.BACKWARD_S, fused=G.fused_cases())
    doc = dict(description="compositing edge rays: bars = 10 x the float32 restatement's error against the float64 oracle (floor 1e-6), every "
                           "emulated defect against them, and the six kernels' worst errors measured on the GPU",
               bar_factor=CR.BAR_FACTOR, bar_floor=CR.BAR_FLOOR, margin=CR.MARGIN, **cpu_part(shapes))
    doc["kernels"] = None if args.cpu_only else gpu_part()
    if not args.cpu_only:
        doc["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("smallest defect / bar:", {q: f"{r['over_bar']:.3g}" for q, r in doc["smallest_defect_over_bar"].items()}, "->", args.out)


if __name__ == "__main__":
    main()
