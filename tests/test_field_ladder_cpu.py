"""The accuracy ladder of the field and render engines on the CPU (tests/_field_arithmetic.py): the restated arithmetic is the
oracle's, every case's bars separate a healthy engine from one that lost a single product in a single contraction, every render
case is well conditioned, and no weight operand has an empty lo plane.  No GPU; tests/test_gpu_field_ladder.py holds the kernels
to these bars."""
import pytest
import torch

import h3d_oracle as O
import _field_arithmetic as A
from conftest import rel_err
from x2_emulation import f16, x2_matmul, x3_matmul

CASES = [pytest.param(c, id=c.name) for c in A.CASES]


@pytest.mark.parametrize("case", CASES)
def test_restatement_is_the_oracle(case):
    """_field / field_render with exact contractions == O.neural_field (+ O.ray_integration) in float64, to 1e-12 -- also with the
    feature head applied once per ray."""
    i = A.inputs_of(case)
    sd = {k: v.double() for k, v in i["state"].items()}
    ref = O.neural_field(sd, i["pts"].double(), i["freq"].double(), i["phase"].double(), i["geo"].double(), i["dirs"].double(), i["scaler"])
    got = A.outputs_of(case)["exact"]
    if case.kind == "field":
        assert rel_err(got, ref) < 1e-12
        return
    clamp, last_back, white_back = case.mode
    ref = O.ray_integration(ref.reshape(A.B, case.R, case.S, -1), i["z"].double(), i["noise"].double(), clamp, last_back, white_back)
    args = (i["state"], i["pts"], i["freq"], i["phase"], i["geo"], i["dirs"], i["scaler"], A.exact_matmul, i["z"], i["noise"], case.S,
            clamp, last_back, white_back)
    for per_ray in (False, True):
        for a, b in zip(A.field_render(*args, per_ray_head=per_ray), ref):
            assert a.shape == b.shape and rel_err(a, b) < 1e-12, per_ray
    for a, b in zip(got, ref):
        assert rel_err(a, b) < 1e-12


def test_the_term_by_term_contractions_are_the_emulations():
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(9, 200, generator=g, dtype=torch.float64) * 2 - 1).float()
    W = (torch.rand(70, 200, generator=g) * 2 - 1) * 0.01
    assert torch.equal(A.x3_terms(x, W), x3_matmul(x, W))
    assert rel_err(A.x2_terms(x, W), x2_matmul(x, W)) < 1e-14
    assert torch.equal(A.d3(x, W), A.f16_matmul(x, W))                 # x2 without its fp6 product IS the single f16 product
    exact = A.exact_matmul(x, W)
    assert rel_err(A.x2_terms(x, W, per_ray_head=True), exact) < rel_err(x2_matmul(x, W), exact)     # hi(W).lo(x) in full f16 there


@pytest.mark.parametrize("case", CASES)
def test_bars_separate_a_lost_product_from_a_healthy_engine(case):
    """Every single-defect variant that touches a group is >= 3 x over the group's bar (by construction: the bar is the smallest
    of them / 3) and the healthy reference arithmetic >= 3 x under it: the fp32 oracle for the x3 class, the x2 emulation itself
    against float64, and its distance to itself under fp32 accumulation for the x2 class's distance bar."""
    L = A.ladder_of(case)
    print(f"\n{case.name}")
    for assertion, kinds, table in (("x3", ("D1", "D2"), L["vs_exact"]), ("x2_dist", ("D3",), L["vs_x2"])):
        for g in L["groups"]:
            bar, healthy = L["bars"][assertion][g], L["healthy"][assertion][g]
            defects = {f"{k}@{l}": table[f"{k}@{l}"][g] for k in kinds for l in range(A.TOUCHED_BY.get(g, A.N_CONTRACTIONS))}
            worst = min(defects, key=defects.get)
            print(f"  {assertion:8s}{g:9s} bar {bar:.2e}  healthy {healthy:.2e} ({bar / max(healthy, 1e-300):6.1f} x under)  "
                  f"smallest defect {worst} {defects[worst]:.2e}  largest {max(defects.values()):.2e}")
            assert bar > 0
            assert all(v >= A.MARGIN * bar * (1 - 1e-12) for v in defects.values()), (assertion, g)
            if A.asserted(case, assertion, g):
                assert A.MARGIN * healthy <= bar, (assertion, g, healthy, bar)
            else:
                # listed as not separating (0.8-2.8 x under where it was chosen, printed above; the healthy figure is fp32 rounding
                # noise, so that it stays under 3 x on every host is not asserted): only the colours' x2 distance under a white
                # background may ever be listed
                assert (assertion, g) == ("x2_dist", "rgb") and case.mode == A.MODES[0], (assertion, g)
    for g in L["groups"]:
        # the x2 class against float64: 3 x the healthy emulation; the fp32 oracle's own error (what the kernel adds to the emulation:
        # fp32 accumulation, fp32 sines) is a small part of that
        bar = L["bars"]["x2"][g]
        print(f"  x2      {g:9s} bar {bar:.2e}  x2 emulation {L['healthy']['x2'][g]:.2e}  fp32 oracle {L['vs_exact']['fp32'][g]:.2e}  "
              f"single f16 product in every layer {L['vs_exact']['f16x1'][g]:.2e}")
        assert L["vs_exact"]["fp32"][g] <= bar / A.MARGIN, g
        assert L["vs_exact"]["f16x1"][g] >= A.MARGIN * bar, g         # a whole engine on single products is far over every bar


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in A.CASES if c.kind != "field"])
def test_render_cases_are_well_conditioned(case):
    """delta = 1e9 on the last sample: a ray's background term flips with the sign of its last density.  EVERY ray of every case
    has |sigma_last + noise| >= 1e-2 of its largest |density| in the float64 oracle (10 x the refinement band of DESIGN 4.3b)."""
    c = A.sigma_conditioning(case)
    print(f"{case.name}: min |sigma_last + noise| / max|sigma| = {c:.3e}")
    assert c >= 1e-2


@pytest.mark.parametrize("key", sorted({(c.hidden, c.feature, c.seed, c.kind != "field") for c in A.CASES}))
def test_weights_have_a_lo_plane(key):
    """fp32 weights whose f16 residual is non-zero in more than 99 % of the entries of every hidden matrix (as the packers scale
    it): float16-stored fixtures have none, and an engine without lo(W) passes them bit for bit."""
    hidden, feature, seed, render = key
    state, _ = A.make_state(hidden, feature, seed, sigma_gain=40.0 if render else 1.0)
    for name, W in A.hidden_matrices(state).items():
        assert W.dtype == torch.float32
        Ws = W.double() * A._matrix_scale(W.double())
        frac = float(((Ws - f16(Ws)) != 0).double().mean())
        assert frac > 0.99, (name, frac)
