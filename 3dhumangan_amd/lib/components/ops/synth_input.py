"""The synthesis network's block-0 input with the label map and / or the latent as extra inputs (the reference's
2d_label_input / 2d_latent_input, lib/generators/map3d_generator.py:256-265): sin(Conv2d(K, F, 1)(coords, label)) and the
latent repeated over the pixels, written channels last in ONE HIP pass (h3d_synth_input) instead of a coordinate tensor, a
GEMM, a sine and a concatenation.  The backward (h3d_synth_input_bwd) recomputes the sine's argument from the inputs, so
nothing activation-sized is kept, and reduces in two fixed-order stages: two runs give the same bits."""
import torch

from .... import _lib


def _run_fwd(w, b, seg, z, B, H, W, label_dim):
    F, K = w.shape
    L = 0 if z is None else z.shape[1]
    out = torch.empty((B, H * W, F + L), device=w.device, dtype=torch.float32)
    rc = _lib.load().h3d_synth_input(_lib.ptr(w), _lib.ptr(b), _lib.ptr(seg), _lib.ptr(z), _lib.ptr(out), B, H, W, F, L, K,
                                     int(label_dim), _lib.stream_handle())
    _lib.check(rc, "h3d_synth_input")
    return out


class _SynthInput(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, b, z, seg, B, H, W, label_dim):
        ctx.save_for_backward(w, b, seg)
        ctx.shape = (B, H, W, label_dim, None if z is None else z.shape[1])
        return _run_fwd(w, b, seg, z, B, H, W, label_dim)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dx):
        w, b, seg = ctx.saved_tensors
        B, H, W, label_dim, L = ctx.shape
        F, K = w.shape
        lib = _lib.load()
        dx = _lib.aligned16(dx.contiguous().float())
        nblk = (H * W + lib.h3d_synth_input_rows() - 1) // lib.h3d_synth_input_rows()
        partial = torch.empty((B, nblk, 4, F), device=dx.device, dtype=torch.float32)
        dw, db = torch.empty_like(w), torch.empty_like(b)
        want_z = L is not None and ctx.needs_input_grad[2]
        partial_z = torch.empty((B, nblk, L), device=dx.device, dtype=torch.float32) if want_z else None
        dz = torch.empty((B, L), device=dx.device, dtype=torch.float32) if want_z else None
        rc = lib.h3d_synth_input_bwd(_lib.ptr(w), _lib.ptr(b), _lib.ptr(seg), _lib.ptr(dx), _lib.ptr(partial), _lib.ptr(partial_z),
                                     _lib.ptr(dw), _lib.ptr(db), _lib.ptr(dz), B, H, W, F, L or 0, K, int(label_dim),
                                     _lib.stream_handle())
        _lib.check(rc, "h3d_synth_input_bwd")
        return dw, db, dz, None, None, None, None, None


def synth_input(weight, bias, hw, batch, seg=None, z=None, label_dim=1):
    """weight [F, K] (K = 3 with a label map, else 2), bias [F], hw = (H, W), seg int64 [batch, H, W] or None, z [batch, L] or
    None -> [batch, H*W, F + L] fp32:  sin(weight . (i, j, seg / label_dim * 2 - 1) + bias)  followed by z."""
    _lib.need_cuda(weight, bias, seg, z)
    H, W = hw
    F, K = weight.shape
    if K != (3 if seg is not None else 2):
        raise ValueError(f"synth_input: weight has {K} input channels, expected {3 if seg is not None else 2}")
    if seg is not None:
        if seg.dtype != torch.int64 or tuple(seg.shape) != (batch, H, W):
            raise ValueError(f"synth_input: seg must be int64 [{batch}, {H}, {W}], got {seg.dtype} {tuple(seg.shape)}")
        seg = seg.contiguous()
    if z is not None:
        if z.ndim != 2 or z.shape[0] != batch:
            raise ValueError(f"synth_input: z must be [{batch}, L], got {tuple(z.shape)}")
        z = z.contiguous().float()
    weight, bias = weight.contiguous().float(), bias.contiguous().float()
    if torch.is_grad_enabled() and (weight.requires_grad or bias.requires_grad or (z is not None and z.requires_grad)):
        return _SynthInput.apply(weight, bias, z, seg, batch, H, W, label_dim)
    return _run_fwd(weight, bias, seg, z, batch, H, W, label_dim)
