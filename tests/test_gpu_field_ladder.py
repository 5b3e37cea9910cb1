"""The field and render engines against the bars of their own arithmetic (tests/_field_arithmetic.py; derivation and the CPU
side: tests/test_field_ladder_cpu.py).  The 1e-3 bar of test_gpu_field.py lets an engine pass that lost a product in
one layer; these do not:
    f32, f16x3, f16x3t   against float64:            (smallest single-defect error D1 / D2 that touches the group) / 3
    f16x2, f16x2t        against float64:            3 x the healthy x2 emulation's error
                         against the x2 emulation:   (smallest distance of a one-layer dead fp6 product, D3) / 3
Weights are seeded fp32 initialisations (non-zero lo planes), B = 2; the CPU side of a case is computed once and shared by its
engines.  tools/field_accuracy_report.py records the same figures in profiles/field_accuracy_ladder.json."""
import pytest

import _field_arithmetic as A
from _field_ladder_gpu import measure

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case,engine", [pytest.param(c, e, id=f"{c.name}-{e}") for c in A.CASES for e in c.engines])
def test_engine_meets_the_bars_of_its_arithmetic(case, engine):
    records = measure(case, engine)
    for r in records:
        print(f"{engine:7s} {case.name:36s} {r['assertion']:8s}{r['group']:9s} measured {r['measured']:.3e}  bar {r['bar']:.3e}  "
              f"headroom {r['headroom']:7.1f} x" + ("" if r["asserted"] else "  (not asserted: does not separate on the CPU)"))
    failed = [(r["assertion"], r["group"], r["measured"], r["bar"]) for r in records if r["asserted"] and not r["measured"] < r["bar"]]
    assert not failed, failed
