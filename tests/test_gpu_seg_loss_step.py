"""discriminator_step / generator_step with seg_loss=losses.segmentation_loss_fused against the same step on the torch loss, from
identical state, on the tiny discriminator of tests/golden/disc_tiny.npz: the logits reach the loss as the discriminator produces
them (y[:, semantic_dim:] of a channels-last tensor: the layout the kernel stages through LDS).

Bar on the step's segmentation scalar, as in tests/test_gpu_seg_loss.py: max(4 e_ref, 4 ulp of fp32 at the value), e_ref = the
error of the torch-loss step against the float64 restatement on the same logits.  Weight gradients: the two losses' dlogits differ
by a few ulp of their maximum (profiles/seg_loss_parity.json) and the backward through the discriminator is linear in them, so
the gradients agree to that relative error times the spread of the layer gains; 1e-4 of the gradient's maximum allows a spread of
~1e3 and is 10 x tighter than the 1e-3 the step is held to against the reference."""
import importlib
import json
import os

import pytest
import torch

from _seg_loss_reference import MODES, seg_loss_f64, ulp32
from conftest import GOLDEN, load_golden, rel_err

pytestmark = pytest.mark.gpu
disc = importlib.import_module("3dhumangan_amd.lib.discriminators")
losses = importlib.import_module("3dhumangan_amd.lib.trainers.losses")
trainers = importlib.import_module("3dhumangan_amd.lib.trainers")


@pytest.fixture(scope="module")
def fx():
    g = load_golden("disc_tiny")
    info = json.load(open(os.path.join(GOLDEN, "disc_tiny.json")))
    D = disc.UNetDiscriminator(**info["kwargs"]).eval()
    D.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in g["state"].items()}, strict=True)
    D = D.cuda()
    real, fake, gt = g["real"].cuda(), g["fake"].cuda(), g["gt_segments"].cuda()
    with torch.no_grad():
        seg = {"real": D(real, None, 1.0)["segments"], "fake": D(fake, None, 1.0)["segments"]}
    return dict(D=D, info=info, real=real, fake=fake, gt=gt, seg=seg, key=info["grad_key"])


def test_the_discriminator_hands_over_the_staged_layout(fx):
    s = fx["seg"]["real"]
    B, L, H, W = s.shape
    assert s.stride(1) == 1 and s.stride(3) >= L and s.stride(2) == W * s.stride(3) and s.stride(0) == H * W * s.stride(3)
    assert s.float().stride() == s.stride()


@pytest.mark.parametrize("mode", MODES)
def test_discriminator_step_fused_against_torch_loss(fx, mode):
    D, gt = fx["D"], fx["gt"]
    meta = dict(fx["info"]["meta"], gan_lambda=0.0, segmentation_loss_mode=mode)      # the shipped configs: the loss IS the objective
    L = meta["label_dim"]
    want = sum(seg_loss_f64(fx["seg"][k].cpu().numpy(), lab.cpu().numpy(), None, mode)["loss"]
               for k, lab in (("real", gt), ("fake", torch.zeros_like(gt))))
    res, grads = {}, {}
    for name, fn in (("torch", None), ("fused", losses.segmentation_loss_fused)):
        res[name] = trainers.discriminator_step(D, torch.optim.SGD(D.parameters(), lr=0.0), fx["real"], fx["fake"], gt, meta, do_r1=True,
                                                seg_loss=fn)
        grads[name] = dict(D.named_parameters())[fx["key"]].grad.clone()
    e_ref = abs(float(res["torch"]["segmentation"].double()) - want)
    err = abs(float(res["fused"]["segmentation"].double()) - want)
    print(f"{mode}: segmentation {want:.9f} err {err:.3e} e_ref {e_ref:.3e}; r1 {float(res['fused']['r1']):.6e}")
    assert err <= max(4 * e_ref, 4 * ulp32(want)), (mode, err, e_ref)
    assert rel_err(res["fused"]["r1"], res["torch"]["r1"]) < 1e-5                      # the R1 target is softmax(segments), not the loss
    assert rel_err(grads["fused"], grads["torch"]) < 1e-4


class _StubG(torch.nn.Module):
    """The stand-in generator of tests/golden/gstep_tiny.npz (tests/test_gstep_cpu.py)."""

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(16, 3 * 32 * 16)
        self.latent_pool = torch.nn.Embedding(4, 16)

    def forward(self, z, conditions, disable_synthesis=False, latent_indices=None, **kw):
        img = torch.tanh(self.lin(z)).view(z.shape[0], 3, 32, 16)
        return {"rgbs": img, "rgbs_render": img[:, :, ::4, ::4]}


def test_generator_step_fused_against_torch_loss():
    info, g = json.load(open(os.path.join(GOLDEN, "gstep_tiny.json"))), load_golden("gstep_tiny")
    G = _StubG()
    G.load_state_dict(g["stub"])
    G = G.cuda()
    D = disc.UNetDiscriminator(**info["disc_kwargs"]).eval()
    D.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in g["disc"].items()})
    D = D.cuda()
    gt = g["data"]["rasterized_segments"].cuda()
    meta = dict(info["meta"])
    with torch.no_grad():
        logits = D(G(g["z"].cuda(), {})["rgbs"], {}, 1.0)["segments"].float()
    want = meta["segmentation_lambda"] * seg_loss_f64(logits.cpu().numpy(), gt.cpu().numpy(), meta.get("segmentation_weights"))["loss"]
    res, grads = {}, {}
    for name, fn in (("torch", None), ("fused", losses.segmentation_loss_fused)):
        res[name] = trainers.generator_step(G, D, torch.optim.SGD(G.parameters(), lr=0.0), g["z"].cuda(), {}, meta, gt_segments=gt,
                                            d_step_count=info["d_step"], seg_loss=fn)
        grads[name] = G.lin.weight.grad.clone()
    e_ref = abs(float(res["torch"]["segmentation"].double()) - want)
    err = abs(float(res["fused"]["segmentation"].double()) - want)
    print(f"generator step: segmentation {want:.9f} err {err:.3e} e_ref {e_ref:.3e}")
    assert err <= max(4 * e_ref, 4 * ulp32(want))
    assert rel_err(grads["fused"], grads["torch"]) < 1e-4
