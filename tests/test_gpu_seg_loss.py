"""The fused segmentation loss (csrc/seg_loss.hip, lib/components/ops/seg_loss.py) on the GPU against the float64 restatement
(tests/_seg_loss_reference.py): the fixture cases of tests/golden/seg_loss_modes.npz plus logits at +-80 and an exact argmax
tie, each in three memory layouts -- contiguous NCHW, the discriminator's channel slice of a channels-last tensor (staged through
LDS), and a window with no single pixel pitch (the general path).

Bar per case and quantity: max(4 e_ref, 4 ulp of fp32 at the compared magnitude), e_ref = the error of the torch fp32 composition
(losses.segmentation_loss) on the same case.  The 4 x allows a different but fixed summation order in a reduction that finishes
in fp64; the ulp floor covers cases where torch happens to be exact.  The correct count is compared exactly.  Worst ratios to
the bar, measured on an MI355X: profiles/seg_loss_parity.json."""
import importlib

import numpy as np
import pytest
import torch

from _seg_loss_reference import LAYOUTS, MODES, hard_cases, in_layout, parity
from conftest import load_golden

pytestmark = pytest.mark.gpu

losses = importlib.import_module("3dhumangan_amd.lib.trainers.losses")
seg_ops = importlib.import_module("3dhumangan_amd.lib.components.ops.seg_loss")
_lib = importlib.import_module("3dhumangan_amd._lib")


_SHARED = {}          # (case, mode) -> the float64 results and the torch composition's, computed once for the three layouts


@pytest.fixture(scope="module")
def cases():
    out = {k: (c["logits"].float(), c["labels"].long(), c["prior"].numpy()) for k, c in load_golden("seg_loss_modes").items()}
    out.update(hard_cases())
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", MODES)
def test_parity_with_the_float64_restatement(cases, mode, layout):
    failures, worst = [], {}
    for name, (logits, labels, prior) in cases.items():
        r = parity(losses.segmentation_loss_fused, losses.segmentation_loss, logits, labels, prior, mode, layout, "cuda", grad_scale=2.5,
                   cache=_SHARED, key=name)
        print(f"{mode} {layout} {name}: " + " ".join(f"{k} err {r[k]['err']:.3e} e_ref {r[k]['e_ref']:.3e} ratio {r[k]['ratio']:.3f}"
                                                      for k in ("loss", "real_prob", "dlogits")) + f" correct {r['correct']}")
        if r["correct"][0] != r["correct"][1] or not r["accuracy_exact"]:
            failures.append((name, "correct", r["correct"]))
        for k in ("loss", "real_prob", "dlogits"):
            worst[k] = max(worst.get(k, 0.0), r[k]["ratio"])
            if not r[k]["err"] <= r[k]["bar"]:
                failures.append((name, k, r[k]))
    print(f"{mode} {layout}: worst ratio to the bar {worst}")
    assert not failures, failures


def test_tie_goes_to_the_first_index(cases):
    logits, labels, _ = cases["tie_L26"]
    _, acc, _ = losses.segmentation_loss_fused(in_layout(logits.cuda(), "sliced"), labels.cuda(), 26)
    assert float(acc) == float((labels == 1).float().mean())


@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_runs_are_bit_identical(cases, layout):
    logits, labels, prior = cases["base_L26_3x67x33"]
    for mode in MODES:
        runs = []
        for _ in range(2):
            x = in_layout(logits.cuda(), layout).detach().requires_grad_(True)
            out = losses.segmentation_loss_fused(x, labels.cuda(), 26, prior.tolist(), mode)
            out[0].backward()
            runs.append([t.detach().clone() for t in out] + [x.grad.clone()])
        for a, b in zip(*runs):
            assert torch.equal(a, b), mode


def test_gradient_layout_follows_the_logits():
    """the sliced layout's gradient comes back dense channels-last (the layout the discriminator's last convolution produces)"""
    x = in_layout(torch.randn(2, 5, 9, 6, device="cuda"), "sliced").detach().requires_grad_(True)
    gt = torch.randint(0, 5, (2, 9, 6), device="cuda")
    loss, acc, prob = seg_ops.seg_loss(x, gt, 5)
    (g,) = torch.autograd.grad(loss, x)
    assert g.permute(0, 2, 3, 1).is_contiguous()
    assert not acc.requires_grad and not prob.requires_grad


@pytest.mark.parametrize("n", [70, 6633, 300 * 257])
def test_histogram_counts_exactly(n):
    g = torch.Generator().manual_seed(n)
    labels = torch.randint(0, 26, (n,), generator=g)
    labels[labels == 7] = 0                                    # an absent class
    occ, coef = seg_ops.label_histogram(labels.cuda(), 26)
    want = torch.bincount(labels, minlength=26)
    assert torch.equal(occ.cpu(), want)
    present = (want[1:] > 0).sum()
    ref = torch.where(want > 0, n / (want.double() * present), torch.zeros(26, dtype=torch.float64))
    ref[0] = 0
    assert torch.equal(coef.cpu(), ref.float())
    _, ones = seg_ops.label_histogram(torch.zeros(n, dtype=torch.long, device="cuda"), 26)
    assert torch.equal(ones.cpu(), torch.ones(26))


def test_refusals():
    x, gt = torch.zeros(1, 2, 3, 3), torch.zeros(1, 3, 3, dtype=torch.long)
    with pytest.raises(_lib.H3DError):
        losses.segmentation_loss_fused(x, gt, 2)
    with pytest.raises(_lib.H3DError):
        losses.segmentation_loss_fused(x.cuda(), gt, 2)
    with pytest.raises(ValueError, match="label_dim >= 3"):
        losses.segmentation_loss_fused(x.cuda(), gt.cuda(), 2, mode="softplus")
    with pytest.raises(ValueError, match="fp32"):
        losses.segmentation_loss_fused(x.cuda().half(), gt.cuda(), 2)
    with pytest.raises(ValueError, match="outside"):
        losses.segmentation_loss_fused(torch.zeros(1, 65, 3, 3, device="cuda"), gt.cuda(), 65)


def test_label_dim_bounds():
    """label_dim 2 (one foreground channel) and 64 (the widest LDS tile: 256 x 65 words, above the 64 KB default limit)"""
    for L in (2, 64):
        g = torch.Generator().manual_seed(L)
        logits, labels = torch.randn(2, L, 19, 17, generator=g), torch.randint(0, L, (2, 19, 17), generator=g)
        for mode in MODES[:3] if L == 2 else MODES:
            for layout in LAYOUTS:
                r = parity(losses.segmentation_loss_fused, losses.segmentation_loss, logits, labels, None, mode, layout, "cuda")
                assert r["correct"][0] == r["correct"][1]
                for k in ("loss", "real_prob", "dlogits"):
                    assert r[k]["err"] <= r[k]["bar"], (L, mode, layout, k, r[k])
