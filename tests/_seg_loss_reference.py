"""The segmentation loss restated in float64 (numpy forward; torch float64 for the gradient): the yardstick of the fused HIP op
and of the torch modes of lib/trainers/losses.py.  Semantics: PhaseTrainer._calculate_segmentation_loss of the reference
(lib/trainers/phase_trainer.py:203-256); the fixture tests/golden/seg_loss_modes.npz holds the reference's own results."""
import numpy as np
import torch

MODES = ("cross_entropy", "cross_entropy_balanced", "cross_entropy_multiclass", "softplus")


def nearest_resize(labels, H, W):
    """F.interpolate(mode="nearest") of [B,h,w] labels: source index = floor(dst * (in / out)), the scale in float32 as torch."""
    h, w = labels.shape[1:]
    if (h, w) == (H, W):
        return labels
    ri = np.minimum(np.floor(np.arange(H, dtype=np.float32) * np.float32(h / H)).astype(np.int64), h - 1)
    ci = np.minimum(np.floor(np.arange(W, dtype=np.float32) * np.float32(w / W)).astype(np.int64), w - 1)
    return labels[:, ri][:, :, ci]


def _softplus(y):
    return np.maximum(y, 0) + np.log1p(np.exp(-np.abs(y)))


def coefficients(labels, L, prior):
    """[L] float64 coefficients of cross_entropy_balanced (all 1 when no label is above 0: plain cross entropy)"""
    occ = np.bincount(labels.reshape(-1), minlength=L).astype(np.float64)
    occ[0] = 0
    n_present = np.count_nonzero(occ)
    if n_present == 0:
        return np.ones(L)
    pw = np.asarray(prior, dtype=np.float64)
    pw = pw / pw.mean()
    coef = np.zeros(L)
    nz = occ > 0
    coef[nz] = labels.size / (occ[nz] * n_present)
    return coef * pw


def seg_loss_f64(logits, labels, prior=None, mode="cross_entropy_balanced"):
    """logits [B,L,H,W], labels [B,h,w] int (numpy) -> dict(loss, accuracy, real_prob, correct) in float64"""
    x = np.asarray(logits, dtype=np.float64)
    B, L, H, W = x.shape
    gt = nearest_resize(np.asarray(labels).astype(np.int64), H, W)
    prior = np.ones(L) if prior is None else prior
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    s = e.sum(axis=1, keepdims=True)
    lse = (m + np.log(s))[:, 0]
    x_gt = np.take_along_axis(x, gt[:, None], axis=1)[:, 0]
    one_hot = np.arange(L)[None, :, None, None] == gt[:, None]
    target = one_hot.copy()
    target[:, 1] |= gt > 0
    if mode == "cross_entropy":
        loss = (lse - x_gt).mean()
    elif mode == "cross_entropy_balanced":
        loss = ((lse - x_gt) * coefficients(gt, L, prior)[gt]).mean()
    elif mode == "cross_entropy_multiclass":
        loss = (np.maximum(x, 0) - x * target + np.log1p(np.exp(-np.abs(x)))).mean()
    elif mode == "softplus":
        y = np.where(target, -x, x)
        loss = (_softplus(y[:, 0]).mean() + _softplus(y[:, 1]).mean() + _softplus(y[:, 2:]).mean()) / 3
    else:
        raise ValueError(mode)
    correct = int(((np.argmax(x[:, 1:], axis=1) + 1) == gt).sum())          # np.argmax: the first maximum
    real_prob = (e[:, 1:].sum(axis=1) / s[:, 0]).mean()
    return dict(loss=float(loss), accuracy=correct / gt.size, real_prob=float(real_prob), correct=correct)


def seg_loss_grad_f64(logits, labels, prior=None, mode="cross_entropy_balanced"):
    """d loss / d logits by torch's float64 autograd of the same restatement -> numpy [B,L,H,W] float64"""
    x = torch.as_tensor(np.asarray(logits, dtype=np.float64)).clone().requires_grad_(True)
    B, L, H, W = x.shape
    gt_np = nearest_resize(np.asarray(labels).astype(np.int64), H, W)
    gt = torch.as_tensor(gt_np)
    prior = np.ones(L) if prior is None else prior
    nll = torch.logsumexp(x, dim=1) - torch.gather(x, 1, gt[:, None])[:, 0]
    target = torch.nn.functional.one_hot(gt, L).permute(0, 3, 1, 2).bool().clone()
    target[:, 1] |= gt > 0
    if mode == "cross_entropy":
        loss = nll.mean()
    elif mode == "cross_entropy_balanced":
        loss = (nll * torch.as_tensor(coefficients(gt_np, L, prior))[gt]).mean()
    elif mode == "cross_entropy_multiclass":
        loss = (x.clamp_min(0) - x * target + torch.log1p(torch.exp(-x.abs()))).mean()
    else:
        y = torch.where(target, -x, x)
        sp = y.clamp_min(0) + torch.log1p(torch.exp(-y.abs()))
        loss = (sp[:, 0].mean() + sp[:, 1].mean() + sp[:, 2:].mean()) / 3
    loss.backward()
    return x.grad.numpy()


# ------------------------------------------------------------------ the parity measurement shared by the GPU test and the tools
LAYOUTS = ("nchw", "sliced", "odd")


def in_layout(x, layout):
    """a [B,L,H,W] device tensor with x's values in one of the layouts the op distinguishes:
    nchw    contiguous
    sliced  the last L of L + 3 channels of a channels-last tensor (the discriminator's y[:, semantic_dim:])
    odd     an interior window of a [B, H+1, L, W+2] buffer: no single pixel pitch, channel stride W + 2"""
    B, L, H, W = x.shape
    if layout == "nchw":
        return x.contiguous()
    if layout == "sliced":
        buf = torch.full((B, H, W, L + 3), float("nan"), dtype=x.dtype, device=x.device)
        v = buf.permute(0, 3, 1, 2)[:, 3:]
    elif layout == "odd":
        buf = torch.full((B, H + 1, L, W + 2), float("nan"), dtype=x.dtype, device=x.device)
        v = buf.permute(0, 2, 1, 3)[:, :, :H, 1:W + 1]
    else:
        raise ValueError(layout)
    v.copy_(x)
    return v


def ulp32(magnitude):
    return float(np.spacing(np.float32(abs(magnitude))))


def parity(fused_fn, torch_fn, logits, labels, prior, mode, layout, device, grad_scale=1.0, cache=None, key=None):
    """Both functions against the float64 restatement on one case.  Errors are absolute; bar = max(4 e_ref, 4 ulp of fp32 at the
    compared magnitude) with e_ref the error of the torch fp32 composition; for dlogits the magnitude is the tensor's max.
    -> dict: per quantity (loss, real_prob, dlogits) err / e_ref / bar / ratio, and correct (got, want).
    ``cache`` (a dict) with ``key``: the float64 results and the torch composition's are computed once per (case, mode) and shared
    by the layouts."""
    L = logits.shape[1]
    pw = None if prior is None else [float(v) for v in prior]
    lab = labels.long().to(device)

    def run(fn, x):
        x = x.detach().requires_grad_(True)
        loss, acc, prob = fn(x, lab, L, pw, mode)
        (loss * grad_scale).backward()
        return float(loss.detach().double()), float(acc.double()), float(prob.double()), x.grad.double().cpu().numpy()

    got = run(fused_fn, in_layout(logits.to(device), layout))
    shared = None if cache is None else cache.get((key, mode, grad_scale))
    if shared is None:
        shared = (seg_loss_f64(logits.numpy(), labels.numpy(), prior, mode),
                  grad_scale * seg_loss_grad_f64(logits.numpy(), labels.numpy(), prior, mode), run(torch_fn, logits.to(device)))
        if cache is not None:
            cache[(key, mode, grad_scale)] = shared
    ref, ref_grad, tor = shared
    n = ref_grad[:, 0].size
    out = {"correct": (int(round(got[1] * n)), ref["correct"]), "accuracy_exact": np.float32(got[1]) == np.float32(ref["accuracy"])}
    for k, g, t, want, mag in (("loss", got[0], tor[0], ref["loss"], abs(ref["loss"])),
                               ("real_prob", got[2], tor[2], ref["real_prob"], abs(ref["real_prob"])),
                               ("dlogits", got[3], tor[3], ref_grad, float(np.abs(ref_grad).max()))):
        err, e_ref = float(np.max(np.abs(g - want))), float(np.max(np.abs(t - want)))
        bar = max(4 * e_ref, 4 * ulp32(mag))
        out[k] = dict(err=err, e_ref=e_ref, bar=bar, ratio=err / bar)
    return out


def hard_cases():
    """two inputs the fixture does not hold: logits at +-80 (the log-sum-exp must not overflow), and an exact tie of the
    maximum over the foreground channels (the first index wins) -> {name: (logits, labels, prior)}"""
    g = torch.Generator().manual_seed(7)
    out = {}
    for L in (26, 3):
        sign = torch.randint(0, 2, (2, L, 7, 5), generator=g).float() * 2 - 1
        out[f"pm80_L{L}"] = (80.0 * sign, torch.randint(0, L, (2, 7, 5), generator=g), np.ones(L, dtype=np.float32))
        x = torch.randn(2, L, 7, 5, generator=g).half().float().clamp(-2, 2)
        first, second = 1, L - 1
        x[:, first] = 3.0
        x[:, second] = 3.0                       # argmax over channels >= 1 must answer `first`
        lab = torch.where(torch.rand(2, 7, 5, generator=g) < 0.5, torch.tensor(first), torch.tensor(second))
        out[f"tie_L{L}"] = (x, lab, np.ones(L, dtype=np.float32))
    return out
