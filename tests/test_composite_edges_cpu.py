"""The compositing restatement, its edge rays and its bars (tests/_composite_reference.py), without a GPU: the restatement is the
oracle, every emulated defect is caught on a named ray wherever it applies, the float32 arithmetic stays well under the bars."""
import math

import pytest
import torch

import _composite_reference as CR

# (S, width) of every case of tests/test_gpu_composite_edges.py: the stand-alone kernels (width 64), the fused renders of
# field_x3.hip (32) and of field_x3t.hip / neural_field.hip (64)
STANDALONE = tuple((S, 64) for S in (1, 7, 8, 64, 65, 128, 200))
FUSED = tuple((S, 32) for S in (8, 16, 32, 64, 96)) + tuple((S, 64) for S in (8, 16, 32, 64, 128))
SHAPES = tuple(sorted(set(STANDALONE + FUSED)))
BACKWARD_S = (8, 64, 65, 200)                 # the sizes of the backward's GPU cases: its defects are shown at these
ids = lambda p: f"S{p[0]}-w{p[1]}"


@pytest.mark.parametrize("S", sorted({s for s, _ in SHAPES}))
def test_ray_list_properties(S):
    names, pat, z = CR.edge_rays(S)
    assert len(set(names)) == len(names)
    assert pat.shape == z.shape == (len(names), S)
    assert float(pat[:, -1].abs().min()) >= 5.0
    assert bool((z[:, 1:] >= z[:, :-1]).all())
    for r, n in enumerate(names):                                # cyclic: the rule also holds for the rolled item
        if CR.is_opaque(n):
            assert not CR.is_opaque(names[(r + 1) % len(names)]), n
    if S >= 8:
        want = {"empty", "empty_then_last_hit", "five_opaque", "dense_lastneg", "dense_lastpos", "thin_lastneg", "softplus_thr",
                "softplus_thr_scaled", "softplus_tail", "zero_delta"}
        ks = {k for k in (0, S // 2, S - 2) + CR.OPAQUE_AT if k < S - 1}
        want |= {f"opaque_at_{k}" for k in ks} | {f"opaque_at_{k}_lastneg" for k in ks}
        assert want <= set(names), want - set(names)
    i = CR.case_inputs(S)
    assert i["names"][1][1:] == i["names"][0][:-1] and torch.equal(i["noise"][1, 1:], i["noise"][0, :-1])


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_restatement_equals_the_oracle(shape):
    S, width = shape
    for mode in CR.MODES:
        err = CR.worst(CR.forward_errors_of(CR.restated_forward(S, width, mode, torch.float64), S, mode), CR.case_inputs(S)["names"])
        assert all(e <= 1e-12 for e, _ in err.values()), (mode, err)
        if width == 64:
            err = CR.worst(CR.backward_errors(CR.restated_backward(S, mode, torch.float64), CR.oracle_backward(S, mode)),
                           CR.case_inputs(S)["names"])
            assert all(e <= 1e-10 for e, _ in err.values()), (mode, err)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_float32_restatement_is_well_under_the_bars(shape):
    S, width = shape
    for mode in CR.MODES:
        bar, err = CR.bars(S, width, mode), CR.float32_errors(S, width, mode)
        for q, (e, ray) in err.items():
            assert math.isfinite(e) and e <= bar[q] / CR.MARGIN, (mode, q, e, bar[q], ray)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_every_defect_is_caught_on_a_named_ray(shape):
    """A condition, not a measurement: wherever a defect applies, the float32 restatement with that one defect exceeds 3 x a bar.
    The backward's defects are shown at the sizes of its GPU cases."""
    S, width = shape
    rows = CR.defect_ratios(S, width, backward=width == 64 and S in BACKWARD_S)
    for mode, defect, ratio, q, ray in rows:
        print(f"S={S} width={width} {mode[0]:8s} last_back={mode[1]:d} white_back={mode[2]:d} {defect:22s} {ratio:9.3g} x bar on {q} of {ray}")
    assert {d for _, d, _, _, _ in rows} >= {d for d in CR.FORWARD_DEFECTS if any(CR.applies(d, S, width, m) for m in CR.MODES)}
    missed = [r for r in rows if not r[2] >= CR.MARGIN]
    assert not missed, missed


def test_fused_case_is_decided_by_the_pattern():
    """The fused renders' case: the oracle's own density stays within +-0.05, the bars are finite and the features' bar is the
    engine's own where that is larger."""
    c = CR.fused_case(16, 32, 32)
    assert c["sigma_max"] <= CR.FUSED_SIGMA and float(c["noise"][:, :, -1].abs().min()) >= 5.0
    for engine in ("f16x2", "f32"):
        for mode in CR.MODES:
            bar, base = CR.fused_bars(16, 32, 32, engine, mode), CR.bars(16, CR.ENGINE_WIDTH[engine], mode)
            assert all(math.isfinite(v) and base[q] <= v < 1e-3 for q, v in bar.items()), (engine, mode, bar)
