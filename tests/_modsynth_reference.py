"""Pure-torch restatement of the synthesis network without spatial normalisation (spatial_normalization="none"), written
from the formulas -- the committed oracle covers the SPADE variant only.

    feature maps [B, R, F] --bilinear (align_corners=False)--> style [B, H*W, F]
    x0 = sin(conv1x1((i, j)))                 (i, j) = linspace(-1, 1) pixel coordinates, channels last [B, H*W, C]
    per block k, layers mod1 / mod2:
        s  = style + fixed ("all"; "mixed" for k in mod_blocks) | style ("isolated", k in mod_blocks) | fixed (otherwise)
        m  = s A^T + b_A + 1
        y  = ((x * m) W) * rsqrt((m^2) (W^2) + 1e-8) + b;   x = leaky_relu(y, 0.2)
      x += block input for k >= num_blocks // 2;   rgb += x Wrgb^T + brgb for k >= num_blocks // 2 - 1
Evaluated in float64 by default so that it can serve as the reference of fp32 engines.
"""
import torch
import torch.nn.functional as F

EPS = 1e-8


def upsample(feature_maps, render_hw, out_hw):
    """[B, R, F] channels last at render resolution -> [B, H*W, F]."""
    B, R, Fd = feature_maps.shape
    g = feature_maps.transpose(1, 2).reshape(B, Fd, render_hw[0], render_hw[1])
    g = F.interpolate(g, out_hw, mode="bilinear", align_corners=False)
    return g.flatten(2).transpose(1, 2)


def coord_input(state, out_hw, dtype, input_prefix="synthesis_input"):
    H, W = out_hw
    i = torch.linspace(-1, 1, H, dtype=dtype).view(H, 1).expand(H, W)
    j = torch.linspace(-1, 1, W, dtype=dtype).view(1, W).expand(H, W)
    w = state[f"{input_prefix}.network.0.weight"].to(dtype).flatten(1)          # [C, 2]
    b = state[f"{input_prefix}.network.0.bias"].to(dtype)
    return torch.sin(torch.stack([i, j], dim=-1).reshape(H * W, 2) @ w.t() + b)  # [H*W, C]


def layer_style(mode, k, mod_blocks, style, fixed):
    """style [B, P, F] per pixel, fixed [B, F] -> the style block k sees, [B, P, F] or [B, 1, F]."""
    if mode == "all" or (mode == "mixed" and k in mod_blocks):
        return style + fixed[:, None]
    if mode == "mixed":
        return fixed[:, None]                       # zeros + fixed
    if mode == "isolated":
        return style if k in mod_blocks else fixed[:, None]
    raise ValueError("invalid map3d_mode")


def mod_layer(x, s, weight, bias, a_w, a_b, internal=None):
    m = s @ a_w.t() + a_b + 1
    w = weight.reshape(weight.shape[-2], weight.shape[-1])
    d = torch.rsqrt((m * m) @ (w * w) + EPS)
    if internal is not None:
        internal.append((m, d))
    return ((x * m) @ w) * d + bias.reshape(-1)


def synthesis(state, feature_maps, fixed_style, render_hw, out_hw, num_blocks, mod_blocks, mode, dtype=torch.float64,
              prefix="synthesis_network", input_prefix="synthesis_input", internal=None):
    """-> rgb [B, 3, H, W].  `internal` (a dict) receives '<block>_feature_map' [B, H*W, C], '<block>_rgb' [B, H*W, 3] and
    'layers': the (m, d) pair of every layer in order (m, d [B, P or 1, C])."""
    g = lambda k: state[k].detach().to(dtype)
    B = feature_maps.shape[0]
    H, W = out_hw
    style = upsample(feature_maps.to(dtype), render_hw, out_hw)
    fixed = fixed_style.to(dtype).reshape(B, -1)
    x = coord_input(state, out_hw, dtype, input_prefix).unsqueeze(0).expand(B, -1, -1)
    layers = [] if internal is not None else None
    rgb = None
    for k in range(num_blocks):
        s = layer_style(mode, k, mod_blocks, style, fixed)
        x_in = x
        for name in ("mod1", "mod2"):
            p = f"{prefix}.network.m3d_{k}.{name}"
            x = F.leaky_relu(mod_layer(x, s, g(p + ".weight"), g(p + ".bias"), g(p + ".affine.weight"),
                                       g(p + ".affine.bias"), layers), 0.2)
        if k >= num_blocks // 2 and x.shape[-1] == x_in.shape[-1]:
            x = x + x_in
        if k >= num_blocks // 2 - 1:
            t = f"{prefix}.to_rgbs.m3d_{k}.linear"
            out = x @ g(t + ".weight").t() + g(t + ".bias")
            rgb = out if rgb is None else out + rgb
        if internal is not None:
            internal[f"m3d_{k}_feature_map"] = x
            internal[f"m3d_{k}_rgb"] = rgb
    if internal is not None:
        internal["layers"] = layers
    return rgb.transpose(1, 2).reshape(B, 3, H, W)
