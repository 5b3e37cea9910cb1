"""Host-side preparation of the style input of the generator WITHOUT the 3D render (disable_render=True) for the fused HIP
kernel csrc/style_input.hip.

Reference forward: lib/components/map3d_layers.py:315-327 (SynthesisStyleInput), called at
lib/generators/map3d_generator.py:224-236.  Per pixel, c the condition and z the latent of the image:

    f = sin(W_c c + b_c);    h = lrelu_0.2(W_0 [f ; normalize_2nd_moment(z)] + b_0);    h = lrelu_0.2(W_k h + b_k) ...

Everything here is *exact* algebra on it:

  static, once per weight version (StyleInputPlan.__init__):
    W_c^T rows + b_c zero padded to LP, W_0[:, :L] and every further network.{2,4,...} conv packed into MFMA B-fragment
    order (include/h3d.h)
  per forward (bias_table), one small library GEMM on the device:
    the latent half of network.0 sees a per-image constant:  bias0[b] = b_0 + W_0[:, L:2L] normalize_2nd_moment(z_b)
    -- the expand / cat of the reference is never materialised.
"""
import torch

from ... import _lib
from ..._stages import stage
from .fragment_pack import _pad, pack_matrix


def normalize_2nd_moment(x, dim=1, eps=1e-8):
    return x * (x.square().mean(dim=dim, keepdim=True) + eps).rsqrt()


class StyleInputPlan:
    """Packed weights of `synthesis_style_input` + the dense matrix of the per-forward fold."""

    def __init__(self, state, prefix, device):
        g = lambda k: state[k].detach().to(device=device, dtype=torch.float32)
        wc = g(f"{prefix}.from_coords.0.weight").flatten(1)                  # [L, Cc]
        w0 = g(f"{prefix}.network.0.weight").flatten(1)                      # [F, 2L]
        L, Cc = wc.shape
        F = w0.shape[0]
        if w0.shape[1] != 2 * L:
            raise ValueError(f"{prefix}.network.0 takes {w0.shape[1]} channels, expected 2 * latent_dim = {2 * L}")
        # the convolutions as the module was built and loaded: network.0, then network.2, network.4, ...
        extra = []
        while f"{prefix}.network.{2 * (len(extra) + 1)}.weight" in state:
            extra.append(2 * (len(extra) + 1))
        if len(extra) > 1:
            raise NotImplementedError(f"h3d_style_input runs one or two GEMM layers (the module has {1 + len(extra)})")
        self.Cc, self.L, self.F, self.n_layers, self.device = Cc, L, F, 1 + len(extra), device
        LP, FP = (L + 31) // 32 * 32, (F + 31) // 32 * 32
        self.LP, self.FP = LP, FP
        self.w_coord = torch.cat([_pad(wc[:, c], LP) for c in range(Cc)] + [_pad(g(f"{prefix}.from_coords.0.bias"), LP)])
        self.w0 = pack_matrix(w0[:, :L], LP // 8, FP // 32)
        self.w0_latent_t = w0[:, L:].t().contiguous()                        # [L, F]
        self.b0 = g(f"{prefix}.network.0.bias")
        self.w1 = self.b1 = None
        if extra:
            self.w1 = pack_matrix(g(f"{prefix}.network.{extra[0]}.weight").flatten(1), FP // 8, FP // 32)
            self.b1 = _pad(g(f"{prefix}.network.{extra[0]}.bias"), FP)

    def bias_table(self, latent, latent_input=True):
        """latent [B, L] -> bias0 [B, F] = b_0 + W_0[:, L:2L] normalize_2nd_moment(latent); with ``latent_input=False`` the
        reference feeds a zero latent (map3d_generator.py:233-234): bias0 = b_0."""
        B = latent.shape[0]
        if not latent_input:
            return self.b0.unsqueeze(0).expand(B, -1).contiguous()
        return torch.addmm(self.b0, normalize_2nd_moment(latent.float()), self.w0_latent_t)

    def run(self, condition, latent, latent_input=True, owner=None):
        """condition [B, Cc, Hc, Wc] (segments already mapped to [-1, 1]), latent [B, L] -> feature map [B, Hc*Wc, F]
        channels last, the layout Map3DGenerator._synthesize takes."""
        if tuple(latent.shape) != (condition.shape[0], self.L):
            raise ValueError(f"latent {tuple(latent.shape)} does not match [{condition.shape[0]}, {self.L}]")
        _lib.need_cuda(condition, latent, self.w0)
        with stage(owner, "style_input_tables"):
            bias0 = self.bias_table(latent, latent_input)
        return self.launch(condition, bias0, owner)

    def launch(self, condition, bias0, owner=None):
        """The kernel on a given bias table: condition [B, Cc, Hc, Wc], bias0 [B, F] -> [B, Hc*Wc, F]."""
        if condition.dim() != 4 or condition.shape[1] != self.Cc:
            raise ValueError(f"condition {tuple(condition.shape)} does not match [B, {self.Cc}, Hc, Wc]")
        B, _, Hc, Wc = condition.shape
        if tuple(bias0.shape) != (B, self.F):
            raise ValueError(f"bias table {tuple(bias0.shape)} does not match [{B}, {self.F}]")
        _lib.need_cuda(condition, bias0, self.w0)
        lib = _lib.load()
        if lib.h3d_style_input_lds_bytes(self.L, self.F) < 0:
            raise _lib.H3DError(f"h3d_style_input: width {max(self.L, self.F)} exceeds what the kernel's LDS plan holds (512)")
        cond, bias0 = condition.float().contiguous(), bias0.float().contiguous()
        out = torch.empty(B, Hc * Wc, self.F, device=condition.device, dtype=torch.float32)
        with stage(owner, "style_input"):
            rc = lib.h3d_style_input(_lib.ptr(cond), _lib.ptr(bias0), _lib.ptr(self.w_coord), _lib.ptr(self.w0), _lib.ptr(self.w1),
                                     _lib.ptr(self.b1), _lib.ptr(out), B, self.Cc, Hc, Wc, self.L, self.F, self.n_layers,
                                     _lib.stream_handle())
        _lib.check(rc, "h3d_style_input")
        return out
