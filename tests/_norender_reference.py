"""Pure-torch restatement of the style input of the generator without the 3D render (disable_render=True), written from
the formulas (SynthesisStyleInput: sine features of the rasterised body condition, concatenated with the normalised
latent, through one or more leaky-ReLU 1x1 convolutions), and of the host-side fold of the latent half.

    c [B, Cc, Hc, Wc]  (segments: label / (label_dim - 1) * 2 - 1;  semantics as they are)
    f = sin(W_c c + b_c)                                             [B, P, L]   P = Hc * Wc
    h = lrelu_0.2([f ; normalize_2nd_moment(z)] W_0^T + b_0)         [B, P, F]
    h = lrelu_0.2(h W_k^T + b_k)   for every further network.{2, 4, ...} convolution in the state dict
Evaluated in float64 by default so that it can serve as the reference of the fp32 kernel.
"""
import torch
import torch.nn.functional as F


def normalize_2nd_moment(x, dim=1, eps=1e-8):
    return x * (x.square().mean(dim=dim, keepdim=True) + eps).rsqrt()


def scale_segments(segments, label_dim, dtype=torch.float32):
    """integer labels [B, Hc, Wc] -> [B, 1, Hc, Wc] in [-1, 1], the reference's expression evaluated in `dtype`."""
    return segments.unsqueeze(1).to(dtype) / (label_dim - 1) * 2 - 1


def extra_layers(state, prefix="synthesis_style_input"):
    ids = []
    while f"{prefix}.network.{2 * (len(ids) + 1)}.weight" in state:
        ids.append(2 * (len(ids) + 1))
    return ids


def bias_table(state, latent, dtype=torch.float64, prefix="synthesis_style_input", latent_input=True):
    """The fold: [B, F] = b_0 + W_0[:, L:2L] normalize_2nd_moment(z)  (zero latent with latent_input=False)."""
    w0 = state[f"{prefix}.network.0.weight"].detach().to(dtype).flatten(1)
    L = w0.shape[1] // 2
    z = latent.to(dtype) if latent_input else torch.zeros_like(latent, dtype=dtype)
    return state[f"{prefix}.network.0.bias"].detach().to(dtype) + normalize_2nd_moment(z) @ w0[:, L:].t()


def style_input(state, condition, latent, dtype=torch.float64, prefix="synthesis_style_input", latent_input=True,
                explicit_cat=False):
    """-> feature map [B, Hc*Wc, F] channels last.  `explicit_cat`: the reference's expand / cat form instead of the fold."""
    g = lambda k: state[k].detach().to(dtype)
    B, Cc, Hc, Wc = condition.shape
    c = condition.to(dtype).flatten(2).transpose(1, 2)                               # [B, P, Cc]
    f = torch.sin(c @ g(f"{prefix}.from_coords.0.weight").flatten(1).t() + g(f"{prefix}.from_coords.0.bias"))
    w0 = g(f"{prefix}.network.0.weight").flatten(1)
    L = w0.shape[1] // 2
    if explicit_cat:
        z = latent.to(dtype) if latent_input else torch.zeros_like(latent, dtype=dtype)
        x = torch.cat([f, normalize_2nd_moment(z)[:, None].expand(B, Hc * Wc, L)], dim=-1)
        h = x @ w0.t() + g(f"{prefix}.network.0.bias")
    else:
        h = f @ w0[:, :L].t() + bias_table(state, latent, dtype, prefix, latent_input)[:, None]
    h = F.leaky_relu(h, 0.2)
    for k in extra_layers(state, prefix):
        h = F.leaky_relu(h @ g(f"{prefix}.network.{k}.weight").flatten(1).t() + g(f"{prefix}.network.{k}.bias"), 0.2)
    return h


def to_nchw(fmap, hw):
    B, P, Fd = fmap.shape
    return fmap.transpose(1, 2).reshape(B, Fd, hw[0], hw[1])
