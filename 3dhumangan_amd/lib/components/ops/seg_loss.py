"""The discriminator's segmentation loss on one fused HIP op (csrc/seg_loss.hip).

Reference: PhaseTrainer._calculate_segmentation_loss (lib/trainers/phase_trainer.py:203-256), the four segmentation_loss_mode
values -> (loss, accuracy over the foreground classes, mean foreground probability).  The torch composition
(lib/trainers/losses.py: segmentation_loss, the CPU path and the parity yardstick) is ~15 operations with an int64 one_hot of
[B,H,W,L], a log_softmax, a second softmax and an argmax plus their autograd; here the logits are read once forward (per-workgroup
partials finished in fp64, no atomics: two runs are bit-identical) and once backward.

    logits  [B,L,H,W] fp32 in ANY strides: the discriminator's y[:, semantic_dim:] (a channel slice of a channels-last tensor) is
            staged through LDS, contiguous NCHW is read coalesced as it lies, everything else by its strides -- no copy.
    labels  [B,H',W'] integer; resized to the logits' size by F.interpolate(..., "nearest") in torch (tiny, and torch's index rule
            is the contract).  PRECONDITION: 0 <= label < label_dim (the reference would raise in one_hot).  Outside it the
            value is undefined (nothing is indexed out of bounds: the softmax modes give such a pixel no loss and no gradient,
            the two other modes treat it as "foreground, class unknown").
The coefficient vector of "cross_entropy_balanced" is built on the device from the label histogram, its no-foreground case
(plain cross entropy) is a device-side select: no host round trip.  The backward is once_differentiable: nothing differentiates the
loss twice (the R1 target is softmax(segments).sum(), not the loss).  accuracy and real_prob carry no gradient."""
import ctypes as C

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from .... import _lib

MODES = ("cross_entropy", "cross_entropy_balanced", "cross_entropy_multiclass", "softplus")
_KIND = {"cross_entropy": 0, "cross_entropy_balanced": 0, "cross_entropy_multiclass": 1, "softplus": 2}

_prior_cache = {}


def _prior(prior_weights, label_dim, device):
    """the prior weights normalised to mean 1 (phase_trainer.py:210-212) as a device vector, cached per (values, device); None: 1"""
    if prior_weights is None:
        return None
    if torch.is_tensor(prior_weights):
        if prior_weights.numel() != label_dim:
            raise ValueError(f"segmentation_weights has {prior_weights.numel()} entries, label_dim is {label_dim}")
        pw = prior_weights.detach().to(device=device, dtype=torch.float32).reshape(-1)
        return (pw / pw.mean()).contiguous()
    key = (tuple(float(v) for v in prior_weights), _lib.canonical_device(device))
    if len(key[0]) != label_dim:
        raise ValueError(f"segmentation_weights has {len(key[0])} entries, label_dim is {label_dim}")
    pw = _prior_cache.get(key)
    if pw is None:
        pw = torch.tensor(key[0], dtype=torch.float32, device=device)
        pw = _prior_cache[key] = pw / pw.mean()
    return pw


def _strides(t):
    return (C.c_int64 * 4)(*t.stride())


def _rows(n):
    r = _lib.load().h3d_seg_loss_rows()
    return (n + r - 1) // r


def label_histogram(labels, label_dim, prior=None, want_coef=True):
    """labels [...] int64 dense on the device -> (occ [L] int64, coef [L] fp32 or None)"""
    _lib.need_cuda(labels, prior)
    if labels.dtype != torch.int64 or not labels.is_contiguous():
        raise ValueError(f"label_histogram takes a contiguous int64 tensor (got {labels.dtype}, strides {labels.stride()})")
    if not 2 <= label_dim <= 64:
        raise ValueError(f"label_histogram: label_dim {label_dim} outside [2, 64]")
    if prior is not None and (prior.dtype != torch.float32 or prior.numel() != label_dim or not prior.is_contiguous()):
        raise ValueError(f"label_histogram: prior must be {label_dim} contiguous fp32 values")
    n = labels.numel()
    partial = torch.empty((_rows(n), label_dim), dtype=torch.int32, device=labels.device)
    occ = torch.empty(label_dim, dtype=torch.int64, device=labels.device)
    coef = torch.empty(label_dim, dtype=torch.float32, device=labels.device) if want_coef else None
    rc = _lib.load().h3d_seg_histogram(_lib.ptr(labels), _lib.ptr(partial), _lib.ptr(occ), _lib.ptr(prior), _lib.ptr(coef), n, label_dim,
                                       _lib.stream_handle())
    _lib.check(rc, "h3d_seg_histogram")
    return occ, coef


class _SegLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, coef, kind):
        B, L, H, W = logits.shape
        n = B * H * W
        need_grad = ctx.needs_input_grad[0]
        lib = _lib.load()
        partial = torch.empty((_rows(n), 4), dtype=torch.float32, device=logits.device)
        stats = torch.empty((n, 2), dtype=torch.float32, device=logits.device) if (need_grad and kind == 0) else None
        x = logits.detach()
        rc = lib.h3d_seg_loss_fwd(_lib.ptr(x), _strides(x), _lib.ptr(labels), _lib.ptr(coef), _lib.ptr(partial), _lib.ptr(stats), B, H, W, L,
                                  kind, _lib.stream_handle())
        _lib.check(rc, "h3d_seg_loss_fwd")
        sums = torch.empty(4, dtype=torch.float64, device=logits.device)
        _lib.check(lib.h3d_rows_sum_f64(_lib.ptr(partial), _lib.ptr(sums), partial.shape[0], 4, _lib.stream_handle()), "h3d_rows_sum_f64")
        count = (n, n * L, 3 * n)[kind]
        ctx.kind, ctx.scale = kind, 1.0 / count
        ctx.save_for_backward(x, labels, coef, stats)
        loss = (sums[0] / count).float()
        acc_prob = (sums[1:3] / n).float()
        accuracy, real_prob = acc_prob[0], acc_prob[1]
        ctx.mark_non_differentiable(accuracy, real_prob)
        return loss, accuracy, real_prob

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, _g_acc, _g_prob):
        x, labels, coef, stats = ctx.saved_tensors
        B, L, H, W = x.shape
        if x.stride(1) == 1 and L > 1:
            dx = torch.empty((B, H, W, L), dtype=torch.float32, device=x.device).permute(0, 3, 1, 2)     # dense channels-last
        else:
            dx = torch.empty_like(x, memory_format=torch.contiguous_format)
        g = g_loss.detach().to(torch.float32).contiguous()
        if ctx.kind == 0 and stats is None:
            raise _lib.H3DError("seg_loss backward without the forward's statistics (the logits did not require grad in forward)")
        rc = _lib.load().h3d_seg_loss_bwd(_lib.ptr(x), _strides(x), _lib.ptr(labels), _lib.ptr(coef), _lib.ptr(stats), _lib.ptr(g),
                                          float(ctx.scale), _lib.ptr(dx), _strides(dx), B, H, W, L, ctx.kind, _lib.stream_handle())
        _lib.check(rc, "h3d_seg_loss_bwd")
        return dx, None, None, None


def seg_loss(segments, gt_segments, label_dim, prior_weights=None, mode="cross_entropy_balanced"):
    """-> (loss, accuracy, real_prob), 0-dim fp32 device tensors; loss differentiable w.r.t. `segments` (once)."""
    if mode not in MODES:
        raise ValueError(f"unknown segmentation_loss_mode {mode!r} (one of {MODES})")
    _lib.need_cuda(segments, gt_segments)
    if segments.dim() != 4 or segments.shape[1] != label_dim:
        raise ValueError(f"segments must be [B, label_dim={label_dim}, H, W], got {tuple(segments.shape)}")
    if not 2 <= label_dim <= 64:
        raise ValueError(f"seg_loss: label_dim {label_dim} outside [2, 64]")
    if mode == "softplus" and label_dim < 3:
        raise ValueError("segmentation_loss_mode 'softplus' needs label_dim >= 3 (channel groups {0}, {1}, {2..})")
    if segments.dtype != torch.float32:
        raise ValueError(f"seg_loss takes fp32 logits (got {segments.dtype}): cast with .float(), which keeps the strides")
    B, _, H, W = segments.shape
    if gt_segments.shape[1] != H or gt_segments.shape[2] != W:
        gt_segments = F.interpolate(gt_segments.unsqueeze(1).float(), (H, W), mode="nearest").squeeze(1)
    labels = gt_segments.detach().long().contiguous()
    coef = None
    if mode == "cross_entropy_balanced":
        _, coef = label_histogram(labels, label_dim, _prior(prior_weights, label_dim, segments.device))
    return _SegLoss.apply(segments, labels, coef, _KIND[mode])
