#!/usr/bin/env python
"""Record the accuracy ladder of the field and render engines: for every case, engine and output group of
tests/test_gpu_field_ladder.py the bar (from the CPU emulation, tests/_field_arithmetic.py), the healthy reference arithmetic's
own error, the error measured on the GPU and the headroom -- plus every single-defect emulation against its bar.

    python tools/field_accuracy_report.py [--out profiles/field_accuracy_ladder.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import _field_arithmetic as A                      # noqa: E402
from _field_ladder_gpu import measure              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_accuracy_ladder.json"))
    args = ap.parse_args()
    cases = []
    worst = {"engine_headroom": float("inf"), "defect_over_bar": float("inf")}
    for case in A.CASES:
        L = A.ladder_of(case)
        defects = {}
        for assertion, kinds, table in (("x3", ("D1", "D2"), L["vs_exact"]), ("x2_dist", ("D3",), L["vs_x2"])):
            for g in L["groups"]:
                d = {f"{k}@{l}": table[f"{k}@{l}"][g] for k in kinds for l in range(A.TOUCHED_BY.get(g, A.N_CONTRACTIONS))}
                if not A.asserted(case, assertion, g):
                    continue
                defects[f"{assertion}/{g}"] = dict(bar=L["bars"][assertion][g], smallest=min(d.values()), largest=max(d.values()),
                                                   smallest_over_bar=min(d.values()) / L["bars"][assertion][g])
                worst["defect_over_bar"] = min(worst["defect_over_bar"], defects[f"{assertion}/{g}"]["smallest_over_bar"])
        rows = []
        for engine in case.engines:
            for r in measure(case, engine):
                r.pop("case")
                rows.append(r)
                if r["asserted"]:
                    worst["engine_headroom"] = min(worst["engine_headroom"], r["headroom"])
                print(f"{case.name:36s} {engine:7s} {r['assertion']:8s}{r['group']:9s} measured {r['measured']:.3e} bar {r['bar']:.3e} "
                      f"healthy {r['healthy_reference']:.3e} headroom {r['headroom']:.1f}", flush=True)
        cases.append(dict(case=case.name, single_defects=defects, engines=rows))
    doc = dict(description="accuracy ladder of the field / render engines: bars from the CPU emulation, errors measured on the GPU",
               margin=A.MARGIN, worst=worst, cases=cases)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("worst:", worst, "->", args.out)


if __name__ == "__main__":
    main()
