"""The accuracy ladder of the convolution family on the CPU (tests/_conv_arithmetic.py): the restated contractions are F.conv2d and
its autograd, the emulated weight planes are the packer's bit for bit, the defect-free emulation is as close to float64 as 16-bit
operand pairs allow, the case set reaches every path of the host's planning, and every case's bars separate a healthy kernel from
one that lost a single term in a single loop unit.  No GPU; tests/test_gpu_conv_ladder.py holds the kernels to these bars."""
import pytest
import torch

import _conv_arithmetic as A
from conftest import rel_err

conv = A.conv
CASES = [pytest.param(c, id=c.name) for c in A.CASES]
CASE_TIERS = [pytest.param(c, t, id=f"{c.name}-{t}") for c in A.CASES for t in c.tiers]


@pytest.mark.parametrize("case", CASES)
def test_restatement_is_conv2d_and_its_autograd(case):
    """The explicit-K contractions with every operand in one exact plane == F.conv2d, its data gradient and its weight gradient in
    float64 (the tap order, the zero padding, the flipped transposed weights, the padded channels)."""
    i = A.inputs_of(case)
    ref = A.exact(case, False)
    xp, wp, bp, gp = A.padded(case, i, False)
    cip, cop, k = A._up64(case.ci), A._up64(case.co), case.k
    cols, Wm = A.columns(xp, k), A.weight_matrix(wp)
    y = A._image(A.contraction(cols, Wm, {"w": (Wm, cols)}) + bp, case, cop, case.co)
    assert rel_err(y, ref["y"]) < 1e-12
    gcols, Wt = A.columns(gp, k), A.weight_matrix(conv._transposed(wp))
    dx = A._image(A.contraction(gcols, Wt, {"w": (Wt, gcols)}), case, cip, case.ci)
    assert rel_err(dx, ref["dx"]) < 1e-12
    g2 = gp.permute(0, 2, 3, 1).reshape(case.P, cop)
    dw = A.wgrad(cols, g2, {"w": (g2, cols)}).reshape(cop, k, k, cip).permute(0, 3, 1, 2)[:case.co, :case.ci]
    assert rel_err(dw, ref["dw"]) < 1e-12
    assert rel_err(g2.sum(0)[:case.co], ref["db"]) < 1e-12


@pytest.mark.parametrize("co,ci,k", sorted({(A._up64(c.co), A._up64(c.ci), c.k) for c in A.CASES}))
def test_emulated_weight_planes_are_the_packers(co, ci, k):
    """split_bf16 of the weights == the hi and lo planes of conv.pack_stream_torch's stream, decoded, bit for bit -- for the forward
    weights and for the flipped, transposed ones of the backward-data convolution."""
    w = torch.randn(co, ci, k, k, generator=torch.Generator().manual_seed(co + ci + k)) / (ci * k * k) ** 0.5
    for wt in (w, conv._transposed(w)):
        o, i = wt.shape[:2]
        NT, nblk, KSC, nch = conv.tiling(i, o)
        t = conv.pack_stream_torch(wt).view(torch.bfloat16).view(nblk, k * k, nch, KSC, NT, 2, 2, 32, 8)      # ob, tap, chunk, ks, nt, hi|lo, h, j, e
        planes = t.permute(5, 0, 4, 7, 2, 3, 6, 8, 1).reshape(2, o, i, k, k)                                    # plane, (ob, nt, j), (chunk, ks, h, e), tap
        hi, lo = A.split_bf16(wt.double())
        assert torch.equal(planes[0].double(), hi) and torch.equal(planes[1].double(), lo)
        assert float((lo != 0).double().mean()) > 0.99               # seeded fp32 weights: a lo plane that matters
    hi16, lo16 = A.split_f16(w.double())
    # f16 lo: residuals under 2^-25 (half the smallest f16 subnormal) round to zero -- a percent or two of weights of this magnitude
    assert float((lo16 != 0).double().mean()) > 0.95 and float((hi16 + lo16 - w.double()).abs().max()) <= max(2.0 ** -22 * float(w.abs().max()), 2.0 ** -25)


def test_the_cases_reach_every_path():
    """Confirmed with the library's host helpers: NT = 2, 4 and 8; more than one output block; more than one channel chunk; forward and
    backward-data launches in K-slices; the two-workgroups-per-CU 1x1 instantiation; pixel counts ragged against the 32-pixel wave
    and the 128-pixel workgroup; a weight gradient in K-slices with a ragged last k-step -- within the size limits of the suite."""
    plans = {c.name: A.ladder_of(c, "f32")["plans"] for c in A.CASES}
    fwd = [p["y"] for p in plans.values()]
    assert {p.nt for p in fwd} == {2, 4, 8}
    assert any(p.blocks > 1 for p in fwd) and any(p.chunks > 1 for p in fwd) and any(p.occ2 for p in fwd)
    assert any(p["y"].slices > 1 for p in plans.values()) and any(p["dx"].slices > 1 for p in plans.values())
    assert any(p.slices > 1 and p.n_iter % p.it_per_slice for p in fwd)                     # ... one with a short last slice
    assert any(c.P % 32 and c.P % 128 and c.P > 128 for c in A.CASES) and any(c.P < 128 and c.P % 32 for c in A.CASES)
    assert any(p["dw"].slices > 1 and c.P % 16 for c, p in zip(A.CASES, plans.values()))
    for c in A.CASES:
        K = c.k * c.k * A._up64(c.ci)
        assert K <= 4608 and (c.P <= 300 or c.P * K <= 300 * 4608), c.name                 # many pixels only at K = 64
        # at most one unit per case may be left undeclared, never the tap or the slice unit; the AMP outputs declare every unit at
        # K <= 1152 and all but the k-step at K = 4608
        assert len(c.undeclared) <= 1 and all(u in ("kstep", "chunk") for _, u in c.undeclared), c.name
        if "f16x2" not in c.tiers:
            assert not c.undeclared, c.name
        if "f16x2" in c.tiers:
            assert c.undeclared == ((("amp", "kstep"),) if K > 1152 else ()), c.name


@pytest.mark.parametrize("case", CASES)
def test_defect_free_emulation_reproduces_float64(case):
    """hi.hi + hi.lo + lo.hi summed in float64 against F.conv2d and its autograd in float64, in EVERY group (whole tensor, worst
    channel, worst row, worst tap): not exact, and at most a third of the group's bar -- that is a ninth of the smallest error any
    declared single defect leaves in that group, so a restatement that itself lost a cross term in one tap, chunk, K-slice or k-step
    cannot pass (the figures: 4-7e-6 for the whole tensors, <= 1.6e-5 for the worst channel or row; printed)."""
    L = A.ladder_of(case, "f32")
    for prim, groups in A.OUT_GROUPS.items():
        for g in groups:
            got, bar = L["x3"][g], L["bars"][g]
            print(f"{case.name} {g:7s}: x3 emulation vs float64 {got:.2e}, bar {bar:.2e}, smallest declared defect {min(L['defects'][g].values()):.2e}")
            assert 0 < got <= bar / A.MARGIN, (g, got, bar)


@pytest.mark.parametrize("case,tier", CASE_TIERS)
def test_bars_separate_a_lost_term_from_a_healthy_kernel(case, tier):
    """Every declared single defect is >= 3 x over its group's bar (by construction: the bar is the smallest of them / 3) and the healthy
    fp32-accumulated emulation is >= 3 x under it; where the bar IS 3 x the healthy emulation (f16-stored outputs: the max-norm, and
    the share of the one-plane tier) the healthy figure must be non-zero for the bar to mean anything."""
    L = A.ladder_of(case, tier)
    print(f"\n{case.name} {tier}  {L['plans']}")
    for g, bar in L["bars"].items():
        healthy, d = L["healthy"][g], L["defects"].get(g)
        assert bar > 0, g
        if d is None:
            print(f"  {g:9s} bar {bar:.2e}  healthy {healthy:.2e} ({bar / max(healthy, 1e-300):6.1f} x under)")
            assert A.MARGIN * healthy <= bar * (1 + 1e-12), (g, healthy, bar)
            continue
        worst = min(d, key=d.get)
        print(f"  {g:9s} bar {bar:.2e}  healthy {healthy:.2e} ({bar / max(healthy, 1e-300):6.1f} x under)  smallest defect {worst} {d[worst]:.2e}  "
              f"largest {max(d.values()):.2e}  ({len(d)} defects)")
        assert all(v >= A.MARGIN * bar * (1 - 1e-12) for v in d.values()), g
        assert A.MARGIN * healthy <= bar, (g, healthy, bar)
    for prim in ("y", "dx", "dw"):                                     # tap and slice units are never dropped
        kinds = {n.split("@")[1].rstrip("0123456789") for g, d in L["defects"].items() if g.startswith(prim) for n in d}
        if kinds:
            assert case.k == 1 or "tap" in kinds, prim
            assert L["plans"][prim].slices == 1 or "slice" in kinds, prim
