"""Decoded uint8 images -> the tensors of one training item, for a batch (the item transform of the reference's
SHHQDataset.__getitem__, lib/data/datasets.py:282-309).

    ingest(rgb, mask, seg, size, geo_only=False)        on a ROCm device: one launch of h3d_ingest (csrc/ingest.hip)
    ingest_torch(rgb, mask, seg, size, geo_only=False)  the same definition in plain torch ops, on any device: the reader's CPU
                                                        path and the baseline the kernel is timed against
both: rgb [B,Hs,Ws,3], mask [B,Hs,Ws], seg [B,Hs,Ws] uint8, size = (H, W)
      -> {"images": [B,3,H,W] fp32, "masks": [B,1,H,W] fp32, "body_segments": [B,H,W] int64}

The definition is in include/h3d.h.  Third-party boundaries, neither library installed: torchvision 0.10.1 (the reference's pin)
resizes a tensor with F.interpolate(mode="bilinear", align_corners=False) and no antialiasing; cv2.resize(INTER_NEAREST) reads
source floor(x * src / dst).  ingest_torch calls F.interpolate itself, whose fp32 scale arithmetic is exact at the data's 2:1 ratio
and within 1e-6 at the tested ratios; the kernel's integer coordinates are exact at every ratio.
"""
import torch
import torch.nn.functional as F

from ... import _lib


def _check(rgb, mask, seg, size):
    for name, t in (("rgb", rgb), ("mask", mask), ("seg", seg)):
        if not torch.is_tensor(t) or t.dtype != torch.uint8:
            raise TypeError(f"ingest: {name} must be a uint8 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if rgb.dim() != 4 or rgb.shape[-1] != 3:
        raise ValueError(f"ingest: rgb must be [B,Hs,Ws,3], got {tuple(rgb.shape)}")
    for name, t in (("mask", mask), ("seg", seg)):
        if tuple(t.shape) != tuple(rgb.shape[:3]):
            raise ValueError(f"ingest: {name} must be [B,Hs,Ws] = {tuple(rgb.shape[:3])}, got {tuple(t.shape)}")
        if t.device != rgb.device:
            raise ValueError(f"ingest: {name} is on {t.device}, rgb on {rgb.device}: all three inputs must share a device")
    H, W = (int(s) for s in size)
    if H < 1 or W < 1 or min(rgb.shape[:3]) < 1:
        raise ValueError(f"ingest: empty shape, source {tuple(rgb.shape)} size {(H, W)}")
    return H, W


def ingest(rgb, mask, seg, size, geo_only=False):
    """The fused path.  Inputs must be contiguous uint8 tensors on the current ROCm device; anything else is refused by name."""
    H, W = _check(rgb, mask, seg, size)
    for name, t in (("rgb", rgb), ("mask", mask), ("seg", seg)):
        if not t.is_cuda:
            raise ValueError(f"ingest: {name} is on {t.device}; the fused path runs on a ROCm device (ingest_torch runs anywhere)")
        if not t.is_contiguous():
            raise ValueError(f"ingest: {name} must be contiguous (strides {t.stride()} for shape {tuple(t.shape)})")
    _lib.need_cuda(rgb, mask, seg)
    B, Hs, Ws = rgb.shape[:3]
    images = torch.empty(B, 3, H, W, dtype=torch.float32, device=rgb.device)
    masks = torch.empty(B, 1, H, W, dtype=torch.float32, device=rgb.device)
    segments = torch.empty(B, H, W, dtype=torch.int64, device=rgb.device)
    lib = _lib.load()
    _lib.check(lib.h3d_ingest(_lib.ptr(rgb), _lib.ptr(mask), _lib.ptr(seg), _lib.ptr(images), _lib.ptr(masks), _lib.ptr(segments),
                              B, Hs, Ws, H, W, int(bool(geo_only)), _lib.stream_handle()), "h3d_ingest")
    return {"images": images, "masks": masks, "body_segments": segments}


def ingest_torch(rgb, mask, seg, size, geo_only=False):
    """The same definition as a composition of torch ops (any device)."""
    H, W = _check(rgb, mask, seg, size)
    Hs, Ws = rgb.shape[1:3]
    m = mask[:, None]
    if geo_only:
        u = m.expand(-1, 3, -1, -1)
    else:
        u = torch.where(m == 0, torch.full_like(m, 255), rgb.permute(0, 3, 1, 2))
    both = torch.cat([u, m], dim=1).float() * (2.0 / 255.0) - 1.0
    both = F.interpolate(both, size=(H, W), mode="bilinear", align_corners=False)
    ys = (torch.arange(H, device=seg.device) * Hs // H).clamp_(max=Hs - 1)
    xs = (torch.arange(W, device=seg.device) * Ws // W).clamp_(max=Ws - 1)
    s = seg[:, ys][:, :, xs].long()
    return {"images": both[:, :3].contiguous(), "masks": both[:, 3:].contiguous(), "body_segments": torch.where(s == 0, 1, s + 1)}
