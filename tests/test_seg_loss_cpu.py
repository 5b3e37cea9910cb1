"""Segmentation loss, CPU side: the float64 restatement and the torch modes of lib/trainers/losses.py against the fixture captured
from the reference (tests/golden/seg_loss_modes.npz, make_golden_seg_loss.py), and the default mode against the function as it
stood before the other modes were added (bit for bit: it is the training objective of every shipped config)."""
import importlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _seg_loss_reference import MODES, seg_loss_f64, seg_loss_grad_f64
from conftest import GOLDEN, load_golden

losses = importlib.import_module("3dhumangan_amd.lib.trainers.losses")
_lib = importlib.import_module("3dhumangan_amd._lib")


@pytest.fixture(scope="module")
def cases():
    return load_golden("seg_loss_modes")


def test_fixture_has_the_cases_the_kernel_is_tested_on(cases):
    names = set(cases)
    for L in (26, 3):
        assert {f"base_L{L}_2x7x5", f"base_L{L}_3x67x33", f"allbg_L{L}", f"single_L{L}", f"prior_L{L}", f"up2_L{L}"} <= names
        assert int(cases[f"allbg_L{L}"]["labels"].max()) == 0
        assert int((cases[f"single_L{L}"]["labels"] == L - 1).sum()) == 1
        assert cases[f"up2_L{L}"]["labels"].shape[1:] == (14, 10) and cases[f"up2_L{L}"]["logits"].shape[2:] == (7, 5)
        assert float(cases[f"prior_L{L}"]["prior"].std()) > 0.1
    assert os.path.getsize(os.path.join(GOLDEN, "seg_loss_modes.npz")) < 1 << 20


# fp32 results of the reference against float64: the reference's means run over <= 6633 x 26 fp32 terms (pairwise sums), its
# softmax / log are fp32: a few ulp.  8 ulp relative (9.5e-7) on loss and real_prob; accuracy is a ratio of exact counts
FP32_BAR = 8 * 2.0 ** -23


@pytest.mark.parametrize("mode", MODES)
def test_restatement_matches_the_reference(cases, mode):
    for name, c in cases.items():
        got = seg_loss_f64(c["logits"].float().numpy(), c["labels"].numpy(), c["prior"].numpy(), mode)
        for k in ("loss", "real_prob"):
            ref = float(c[mode][k])
            assert abs(got[k] - ref) <= FP32_BAR * max(abs(ref), 1e-3), (name, mode, k, got[k], ref)
        assert np.float32(got["accuracy"]) == np.float32(c[mode]["accuracy"]), (name, mode)


@pytest.mark.parametrize("mode", MODES)
def test_torch_modes_match_the_reference(cases, mode):
    """the same operations as the reference in the same order: equal to the last bits"""
    for name, c in cases.items():
        L = c["logits"].shape[1]
        loss, acc, prob = losses.segmentation_loss(c["logits"].float(), c["labels"].long(), L, c["prior"].tolist(), mode)
        assert abs(float(loss) - float(c[mode]["loss"])) <= 2 * 2.0 ** -23 * abs(float(c[mode]["loss"])), (name, mode)
        assert float(acc) == float(c[mode]["accuracy"]) and float(prob) == float(c[mode]["real_prob"]), (name, mode)


@pytest.mark.parametrize("mode", MODES)
def test_restated_gradient_is_the_torch_gradient(cases, mode):
    """the float64 gradient the GPU test compares with, against autograd of the torch composition (fp32)"""
    c = cases["prior_L26"]
    x = c["logits"].float().requires_grad_(True)
    losses.segmentation_loss(x, c["labels"].long(), 26, c["prior"].tolist(), mode)[0].backward()
    ref = seg_loss_grad_f64(c["logits"].float().numpy(), c["labels"].numpy(), c["prior"].numpy(), mode)
    assert np.abs(x.grad.numpy() - ref).max() <= 16 * 2.0 ** -23 * np.abs(ref).max()


def _segmentation_loss_before(segments, gt_segments, label_dim, prior_weights=None):
    """lib/trainers/losses.py: segmentation_loss as it stood before the other three modes were added"""
    B, _, H, W = segments.shape
    if gt_segments.shape[1] != H or gt_segments.shape[2] != W:
        gt_segments = F.interpolate(gt_segments.unsqueeze(1).float(), (H, W), mode="nearest").squeeze(1).long()
    pw = torch.ones(label_dim, dtype=segments.dtype, device=segments.device) if prior_weights is None else \
        torch.as_tensor(prior_weights, dtype=segments.dtype, device=segments.device)
    pw = pw / pw.mean()
    if torch.any(gt_segments > 0):
        one_hot = F.one_hot(gt_segments, num_classes=label_dim).permute(0, 3, 1, 2)
        occ = one_hot.sum(dim=(0, 2, 3))
        occ[0] = 0
        n_present = torch.count_nonzero(occ)
        coef = torch.reciprocal(occ.to(segments.dtype)) * one_hot.numel() / (n_present * one_hot.shape[1])
        coef[0] = 0
        coef[torch.isinf(coef)] = 0
        loss = (F.cross_entropy(segments, gt_segments, reduction="none") * (coef * pw)[gt_segments]).mean()
    else:
        loss = F.cross_entropy(segments, gt_segments)
    real_prob = (1 - torch.softmax(segments, dim=1)[:, 0]).mean()
    accuracy = ((torch.argmax(segments[:, 1:], dim=1) + 1) == gt_segments).float().mean()
    return loss, accuracy, real_prob


def test_default_mode_is_bit_identical_to_the_function_before():
    g = load_golden("disc_tiny")
    L = json.load(open(os.path.join(GOLDEN, "disc_tiny.json")))["meta"]["label_dim"]
    for seg, gt in ((g["out_real"]["segments"], g["gt_segments"]), (g["out_fake"]["segments"], torch.zeros_like(g["gt_segments"]))):
        for pw in (None, [0.5, 1.0, 3.0]):
            a, b = seg.clone().requires_grad_(True), seg.clone().requires_grad_(True)
            now, before = losses.segmentation_loss(a, gt, L, pw), _segmentation_loss_before(b, gt, L, pw)
            for u, v in zip(now, before):
                assert torch.equal(u, v)
            now[0].backward()
            before[0].backward()
            assert torch.equal(a.grad, b.grad)
    assert float(losses.segmentation_loss(g["out_real"]["segments"], g["gt_segments"], L)[0]) == float(g["loss"]["seg_real"])


def test_refusals():
    x, gt = torch.zeros(1, 2, 3, 3), torch.zeros(1, 3, 3, dtype=torch.long)
    with pytest.raises(ValueError, match="label_dim >= 3"):
        losses.segmentation_loss(x, gt, 2, mode="softplus")
    with pytest.raises(ValueError, match="unknown segmentation_loss_mode"):
        losses.segmentation_loss(x, gt, 2, mode="dice")
    with pytest.raises(_lib.H3DError):                       # the fused op has no CPU path
        losses.segmentation_loss_fused(x, gt, 2)


def test_library_exports_the_entry_points():
    lib = _lib.load()
    for name in ("h3d_seg_loss_rows", "h3d_seg_histogram", "h3d_seg_loss_fwd", "h3d_seg_loss_bwd"):
        assert hasattr(lib, name)
    assert lib.h3d_seg_loss_rows() == 256
    # bad arguments are refused before any HIP call
    assert lib.h3d_seg_loss_fwd(None, None, None, None, None, None, 1, 4, 4, 26, 0, None) == -1
    assert b"null pointer" in lib.h3d_last_error()


class _TinyD(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 4, 1)

    def forward(self, x, conditions, alpha, **kw):
        y = self.conv(x)
        return {"prediction": y[:, :1], "segments": y[:, 1:]}


class _TinyG(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(4, 3 * 4 * 2)

    def forward(self, z, conditions, **kw):
        return {"rgbs": self.lin(z).view(-1, 3, 4, 2)}


def test_steps_pass_the_mode_and_the_function_through():
    """discriminator_step / generator_step call the given seg_loss with meta's segmentation_loss_mode (a recording stand-in);
    seg_loss=None is losses.segmentation_loss, and a non-default mode changes the G step's loss accordingly"""
    tr = importlib.import_module("3dhumangan_amd.lib.trainers")
    torch.manual_seed(0)
    D, G = _TinyD(), _TinyG()
    calls = []

    def recording(segments, gt, label_dim, prior, mode):
        calls.append((tuple(segments.shape), label_dim, prior, mode))
        return losses.segmentation_loss(segments, gt, label_dim, prior, mode)

    meta = dict(gan_lambda=0, segmentation_lambda=1, r1_lambda=0.0, label_dim=3, segmentation_loss_mode="softplus",
                segmentation_weights=[1.0, 2.0, 3.0])
    gt, z = torch.randint(0, 3, (2, 4, 2)), torch.randn(2, 4)
    real, fake = torch.randn(2, 3, 4, 2), torch.randn(2, 3, 4, 2)
    d = tr.discriminator_step(D, torch.optim.SGD(D.parameters(), lr=0.0), real, fake, gt, meta, do_r1=False, seg_loss=recording)
    assert calls == [((2, 3, 4, 2), 3, [1.0, 2.0, 3.0], "softplus")] * 2
    assert torch.equal(d["segmentation"], tr.discriminator_step(D, torch.optim.SGD(D.parameters(), lr=0.0), real, fake, gt, meta,
                                                                do_r1=False)["segmentation"])
    del calls[:]
    g = tr.generator_step(G, D, torch.optim.SGD(G.parameters(), lr=0.0), z, {}, meta, gt_segments=gt, seg_loss=recording)
    assert calls == [((2, 3, 4, 2), 3, [1.0, 2.0, 3.0], "softplus")]
    plain = tr.generator_step(G, D, torch.optim.SGD(G.parameters(), lr=0.0), z, {}, meta, gt_segments=gt)
    other = tr.generator_step(G, D, torch.optim.SGD(G.parameters(), lr=0.0), z, {}, dict(meta, segmentation_loss_mode="cross_entropy"),
                              gt_segments=gt)
    assert torch.equal(g["segmentation"], plain["segmentation"]) and not torch.equal(g["segmentation"], other["segmentation"])
    with torch.no_grad():
        want = losses.segmentation_loss(D(G(z, {})["rgbs"], {}, 1.0)["segments"], gt, 3, [1.0, 2.0, 3.0], "softplus")[0]
    assert torch.equal(g["segmentation"], want)


def test_prior_length_is_checked_before_the_device_reads_it():
    seg_ops = importlib.import_module("3dhumangan_amd.lib.components.ops.seg_loss")
    for bad in ([1.0, 2.0], torch.ones(2)):
        with pytest.raises(ValueError, match="entries"):
            seg_ops._prior(bad, 3, "cpu")
