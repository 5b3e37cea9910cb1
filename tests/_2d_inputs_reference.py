"""Pure-torch restatement, float64 by default, of what the synthesis input variants add to the generator, written from the
formulas:

  block 0's input     coords = (i, j [, label / label_dim * 2 - 1])      i = linspace(-1, 1, H)[y], j = linspace(-1, 1, W)[x]
                      x = sin(W_in coords + b_in)                         [B, F, H, W]
                      x = cat([x, latent repeated over the pixels])       [B, F + L, H, W]      (2d_latent_input)
                      (the divisor of the label is label_dim, not label_dim - 1 as in the style input)
  whole generator     the oracle's stages (mapping networks, render, SPADE network -- its blocks take any input width) around that
                      input; staged_forward hands block 0 the TRUNCATED latent
  padded pack         feature_dim < hidden_dim: block 0's input side zero-padded to hidden_dim is the same function
                      (padded_state: the algebra of SynthesisPlan's fold, on a state dict)
"""
import torch
import torch.nn.functional as F

import _norender_reference as NR
import h3d_oracle as O


def pixel_coords(H, W, dtype=torch.float64):
    """-> [2, H, W]: row coordinate i, column coordinate j."""
    ii = torch.linspace(-1, 1, H, dtype=dtype)[:, None].expand(H, W)
    jj = torch.linspace(-1, 1, W, dtype=dtype)[None, :].expand(H, W)
    return torch.stack([ii, jj], dim=0)


def label_channel(seg, label_dim, dtype=torch.float64):
    """integer labels [B, H, W] -> [B, 1, H, W]; the reference's expression, evaluated in `dtype`."""
    return seg.unsqueeze(1).to(dtype) / label_dim * 2 - 1


def block0_input(weight, bias, H, W, batch, seg=None, label_dim=None, latent=None, dtype=torch.float64):
    """weight [F, K(, 1, 1)], bias [F] -> [B, H*W, F (+ L)] channels last."""
    w = weight.to(dtype).flatten(1)
    c = pixel_coords(H, W, dtype)[None].expand(batch, 2, H, W)
    if seg is not None:
        c = torch.cat([c, label_channel(seg, label_dim, dtype)], dim=1)
    assert c.shape[1] == w.shape[1], (c.shape, w.shape)
    x = torch.sin(c.flatten(2).transpose(1, 2) @ w.t() + bias.to(dtype))
    if latent is not None:
        x = torch.cat([x, latent.to(dtype)[:, None].expand(batch, H * W, latent.shape[1])], dim=-1)
    return x


def to_nchw(x, hw):
    B, P, C = x.shape
    return x.transpose(1, 2).reshape(B, C, hw[0], hw[1])


def cast(tree, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in tree.items()}


def generator_forward(state, cfg, z, cond, jitter, noise=None, truncation=None, dtype=torch.float64, training=False,
                      buffers_out=None):
    """Map3DGenerator.forward (truncation None) / staged_forward (truncation = (psi, avg z, avg freq, avg phase, avg styles)) with
    the flags of cfg: 2d_label_input, 2d_latent_input, disable_render, any feature_dim.  -> dict(rgbs, rgbs_render, depths, x0)"""
    state, cond = cast(state, dtype), cast(cond, dtype)
    z = z.to(dtype)
    B, H, W = z.shape[0], cfg["gen_height"], cfg["gen_width"]
    zin = z if cfg.get("neural_field_latent_input", True) else torch.zeros_like(z)
    freq, phase = O.film_mapping(state, zin)
    _, styles = O.style_mapping(state, z)
    latent = z
    if truncation is not None:
        psi, az, af, ap, ast = (t.to(dtype) if torch.is_tensor(t) else t for t in truncation)
        freq, phase = af + psi * (freq - af), ap + psi * (phase - ap)
        latent, styles = az + psi * (z - az), ast + psi * (styles - ast)
    hr, wr = cfg["render_height"], cfg["render_width"]
    if cfg.get("disable_render", False):
        modal = cfg["condition_modal_gen"]
        c = cond[modal]
        c = NR.scale_segments(c, cfg["label_dim"], dtype) if "segments" in modal else c
        fmap = NR.to_nchw(NR.style_input(state, c, latent, dtype=dtype), tuple(c.shape[2:]))
        rgb_render = torch.zeros(B, 3, hr, wr, dtype=dtype)
        depth = torch.zeros(B, hr * wr, 1, dtype=dtype)
    else:
        rgb_render, fmap, depth, _, _ = O.render(state, cfg, freq, phase, cond, jitter.to(dtype), None if noise is None else noise.to(dtype))
    fmap_up = F.interpolate(fmap, (H, W), mode="bilinear")
    seg = cond["rasterized_segments"] if cfg.get("2d_label_input", False) else None
    x0 = block0_input(state["synthesis_input.network.0.weight"], state["synthesis_input.network.0.bias"], H, W, B, seg,
                      cfg["label_dim"], latent if cfg.get("2d_latent_input", False) else None, dtype)
    syn = O.synthesis_network(state, to_nchw(x0, (H, W)), fmap_up, styles, cfg.get("map3d_mode", "isolated"),
                              tuple(cfg["mod_blocks"]), cfg["synthesis_blocks"], training=training, buffers_out=buffers_out)
    zc = cond["intrinsics"][:, 0, 0] / cond["scales"]
    dm = ((depth - zc.view(B, 1, 1)) / (cfg["depth_length"] / 2.0)).clamp(-1, 1)
    return dict(rgbs=syn["final"], rgbs_render=rgb_render, depths=dm.reshape(B, hr, wr).unsqueeze(1), x0=x0, styles=styles,
                feature_maps=fmap)


def padded_state(state, prefix="synthesis_network", input_prefix="synthesis_input"):
    """The state dict of the SAME function with block 0's input side zero-padded from input_dim to hidden_dim channels:
    the coordinate convolution gets zero rows (sin(0) = 0 on the new channels), the first SPADE's BatchNorm maps them to zero
    (weight 0, bias 0; mean 0, variance 1), its gamma / beta convolutions get zero rows and zero biases, conv_0 zero columns."""
    sd = dict(state)
    b0 = f"{prefix}.network.m3d_0"
    w = state[b0 + ".conv_0.weight_orig"]
    C, cin = w.shape[:2]
    n = C - cin
    assert n >= 0

    def grow(key, dim=0, fill=0.0):
        t = state[key]
        shape = list(t.shape)
        shape[dim] = n
        sd[key] = torch.cat([t, t.new_full(shape, fill)], dim=dim)

    grow(input_prefix + ".network.0.weight")
    grow(input_prefix + ".network.0.bias")
    for k in ("weight", "bias", "running_mean"):
        grow(f"{b0}.spade_0.first_norm.{k}")
    grow(f"{b0}.spade_0.first_norm.running_var", fill=1.0)
    for m in ("mlp_gamma", "mlp_beta"):
        grow(f"{b0}.spade_0.{m}.weight")
        grow(f"{b0}.spade_0.{m}.bias")
    grow(b0 + ".conv_0.weight_orig", dim=1)
    # sigma = u . (W v) of the spectral norm: zero columns with zero entries of v leave it as it is
    grow(b0 + ".conv_0.weight_v")
    return sd
