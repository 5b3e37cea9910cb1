"""Golden fixture of the segmentation loss from the real Python reference: seg_loss_modes.npz.

BUILD CONTAINER ONLY (imports /root/reference through _ref_import.py).  Stores data only: per case the logits (fp16-exact, stored
as fp16), the labels (int16), the prior weights and, for each of the four segmentation_loss_mode values, what the reference's own
PhaseTrainer._calculate_segmentation_loss (lib/trainers/phase_trainer.py:203-256) returns -- called unbound on a minimal
stand-in for `self`, as make_golden_train.py does for the discriminator's losses.
Cases: label_dim 26 and 3 at B.H.W = 2.7.5 and 3.67.33 (uniform prior), and at 2.7.5 the special ones: all-background labels, a
class present in exactly one pixel, non-uniform prior weights, labels given at twice the logits' size.
Run:  python tests/golden/make_golden_seg_loss.py
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
warnings.filterwarnings("ignore")

import _ref_import  # noqa: E402

_ref_import.install()
for name in ("tensorboardX", "torch.utils.tensorboard"):
    if name not in sys.modules:
        m = types.ModuleType(name)
        m.SummaryWriter = object
        sys.modules[name] = m

import lib.trainers.phase_trainer as pt  # noqa: E402

MODES = ("cross_entropy", "cross_entropy_balanced", "cross_entropy_multiclass", "softplus")


def reference(logits, labels, prior, mode):
    me = types.SimpleNamespace(device="cpu")
    meta = dict(label_dim=logits.shape[1], segmentation_loss_mode=mode, segmentation_weights=[float(v) for v in prior])
    loss, acc, prob = pt.PhaseTrainer._calculate_segmentation_loss(me, logits, labels, meta)
    return dict(loss=np.float32(loss), accuracy=np.float32(acc), real_prob=np.float32(prob))


def main():
    g = torch.Generator().manual_seed(2024)
    out = {}

    def case(name, L, shape, labels=None, prior=None, label_scale=1):
        B, H, W = shape
        logits = (2.0 * torch.randn(B, L, H, W, generator=g)).half().float()
        if labels is None:
            labels = torch.randint(0, L, (B, H * label_scale, W * label_scale), generator=g)
        prior = torch.ones(L) if prior is None else prior
        out[f"{name}/logits"] = logits.half().numpy()
        out[f"{name}/labels"] = labels.numpy().astype(np.int16)
        out[f"{name}/prior"] = prior.numpy().astype(np.float32)
        for mode in MODES:
            for k, v in reference(logits, labels.long(), prior, mode).items():
                out[f"{name}/{mode}/{k}"] = v

    for L in (26, 3):
        for shape in ((2, 7, 5), (3, 67, 33)):
            case(f"base_L{L}_{shape[0]}x{shape[1]}x{shape[2]}", L, shape)
        small = (2, 7, 5)
        case(f"allbg_L{L}", L, small, labels=torch.zeros(small, dtype=torch.long))
        once = torch.randint(0, 2, small, generator=g)                 # classes 0 and 1 only ...
        once[1, 3, 2] = L - 1                                          # ... and the last class in exactly one pixel
        case(f"single_L{L}", L, small, labels=once)
        case(f"prior_L{L}", L, small, prior=(0.25 + 2.0 * torch.rand(L, generator=g)).half().float())
        case(f"up2_L{L}", L, small, label_scale=2)
    path = os.path.join(HERE, "seg_loss_modes.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
