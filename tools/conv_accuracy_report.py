#!/usr/bin/env python
"""Record the accuracy ladder of the convolution family: for every case, tier and group of tests/test_gpu_conv_ladder.py the bar (from
the CPU emulation, tests/_conv_arithmetic.py), the figure of the emulation with fp32 accumulation (an upper-bound model: one rounding per product), the figure measured on the GPU and the
headroom -- plus the smallest and largest declared single-defect emulation against each bar.

    python tools/conv_accuracy_report.py [--out profiles/conv_accuracy_ladder.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import _conv_arithmetic as A                       # noqa: E402
import _conv_ladder_gpu as G                       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_accuracy_ladder.json"))
    args = ap.parse_args()
    cases = []
    worst = {"kernel_headroom": float("inf"), "defect_over_bar": float("inf"), "bar_over_healthy": float("inf")}
    for case in A.CASES:
        tiers = []
        for tier in case.tiers:
            L = A.ladder_of(case, tier)
            defects = {}
            for g, d in L["defects"].items():
                lo, hi = min(d, key=d.get), max(d, key=d.get)
                defects[g] = dict(bar=L["bars"][g], declared=len(d), smallest=d[lo], smallest_unit=lo, largest=d[hi], largest_unit=hi,
                                  smallest_over_bar=d[lo] / L["bars"][g])
                worst["defect_over_bar"] = min(worst["defect_over_bar"], defects[g]["smallest_over_bar"])
            with G.weight_planes(tier):
                rows = G.measure(case, tier)
            for r in rows:
                r.pop("case")
                r.pop("tier")
                worst["kernel_headroom"] = min(worst["kernel_headroom"], r["headroom"])
                worst["bar_over_healthy"] = min(worst["bar_over_healthy"], r["bar"] / max(r["healthy_reference"], 1e-300))
                print(f"{case.name:20s} {tier:6s} {r['group']:9s} measured {r['measured']:.3e} bar {r['bar']:.3e} "
                      f"healthy {r['healthy_reference']:.3e} headroom {r['headroom']:.1f}", flush=True)
            plans = {k: v._asdict() for k, v in L["plans"].items()}
            tiers.append(dict(tier=tier, plans=plans, undeclared=[list(u) for u in case.undeclared], single_defects=defects,
                              x3_emulation_vs_float64={k: v for k, v in L["x3"].items()} if tier == "f32" else None, groups=rows))
        cases.append(dict(case=case.name, shape=dict(B=case.B, H=case.H, W=case.W, ci=case.ci, co=case.co, k=case.k, dense=case.dense),
                          tiers=tiers))
    doc = dict(description="accuracy ladder of the convolution family (conv_x3.hip, wgrad_x3.hip, their AMP instantiations, ops/linear.py): "
                           "bars from the CPU emulation, figures measured on the GPU",
               margin=A.MARGIN, worst=worst, cases=cases)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("worst:", worst, "->", args.out)


if __name__ == "__main__":
    main()
