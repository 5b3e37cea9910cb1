"""Host-side preparation of the synthesis network WITHOUT spatial normalisation (spatial_normalization="none") for the
fused HIP kernel csrc/synthesis_mod.hip.

Reference forward: lib/generators/map3d_generator.py:58-97 over SynthesisBlock / SpatialStyleModLayer
(lib/components/map3d_layers.py:25-112).  One layer is

    m = A style + (b_A + 1);    y = lrelu_0.2( ((x * m) W) * rsqrt((m^2) (W^2) + eps) + b )

Everything here is *exact* algebra on it:

  static, once per weight version (ModSynthesisPlan.__init__):
    W^T and (W^2)^T of every layer packed into MFMA B-fragment order (include/h3d.h), vectors zero padded to HdP
  per forward (layer_tables), a handful of small library GEMMs on the device:
    a layer whose style is the per-image fixed style (blocks outside mod_blocks; "mixed": zeros + fixed, "isolated": fixed)
        m[b] = A fixed[b] + b_A + 1            [B, Cin]
        d[b] = rsqrt(m[b]^2 (W^2) + eps)        [B, Cout]      -> the layer is ONE per-pixel GEMM with a pre- and a post-scale
    a layer whose style is the rendered feature map G ("all": every layer; otherwise the blocks in mod_blocks)
        M = G A^T + c[b],  c[b] = b_A + 1  (+ A fixed[b] in "all" / "mixed" mode: style = G + fixed, never added per pixel)
      at RENDER resolution: A is linear and the bilinear weights sum to one, so A bilinear(G) + c = bilinear(M).  The kernel
      samples M per output pixel -> TWO per-pixel GEMMs per such layer instead of three.
  With the shipped mod_blocks = [0, 1, 2] that is 6 * 2 + 12 = 24 per-pixel GEMMs instead of the 54 of the layer-by-layer form.
"""
import ctypes

import torch

from ... import _lib
from ..._stages import stage
from .fragment_pack import _pad, pack_matrix

EPS = 1e-8          # SpatialStyleModLayer's eps (map3d_layers.py:29)


class ModLayerDesc(ctypes.Structure):
    _fields_ = [("pixel_style", ctypes.c_int32), ("map_offset", ctypes.c_int32), ("vec_index", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("w", ctypes.c_int64), ("w2", ctypes.c_int64), ("bias", ctypes.c_int64)]


class ModBlockDesc(ctypes.Structure):
    _fields_ = [("layer", ModLayerDesc * 2), ("skip", ctypes.c_int32), ("to_rgb", ctypes.c_int32), ("w_rgb", ctypes.c_int64)]


class ModSynthDesc(ctypes.Structure):
    _fields_ = [("n_blocks", ctypes.c_int32), ("C", ctypes.c_int32), ("eps", ctypes.c_float), ("reserved", ctypes.c_int32),
                ("w_in", ctypes.c_int64), ("b_in", ctypes.c_int64), ("block", ModBlockDesc * 16)]


class ModSynthesisPlan:
    """Packed weights + launch descriptor + the dense matrices of the per-forward folding."""

    def __init__(self, state, prefix, input_prefix, n_blocks, mod_blocks, map3d_mode, device):
        g = lambda k: state[k].detach().to(device=device, dtype=torch.float32)
        if map3d_mode not in ("all", "mixed", "isolated"):
            raise ValueError("invalid map3d_mode")
        if not 1 <= n_blocks <= 16:
            raise NotImplementedError(f"the synthesis kernel holds 1..16 blocks (got {n_blocks})")
        self.mode, self.n_blocks, self.device = map3d_mode, n_blocks, device
        w0 = g(f"{prefix}.network.m3d_0.mod1.weight")
        cin0, C = w0.shape[2], w0.shape[3]
        F = g(f"{prefix}.network.m3d_0.mod1.affine.weight").shape[1]
        if cin0 != C:
            raise NotImplementedError(f"the synthesis kernel needs input_dim == hidden_dim (got {cin0} and {C}; equal in every shipped config)")
        self.C, self.F = C, F
        HdP = (C + 31) // 32 * 32
        self.HdP = HdP
        NT, KBH = HdP // 32, HdP // 8
        chunks, off = [], [0]

        def add(t):
            o = off[0]
            chunks.append(t)
            off[0] += t.numel()
            return o

        desc = ModSynthDesc()
        desc.n_blocks, desc.C, desc.eps = n_blocks, C, EPS
        w_in = g(f"{input_prefix}.network.0.weight").reshape(C, 2)
        desc.w_in = add(torch.cat([_pad(w_in[:, 0], HdP), _pad(w_in[:, 1], HdP)]))
        desc.b_in = add(_pad(g(f"{input_prefix}.network.0.bias"), HdP))
        self.pixel_ids, self.vec_ids = [], []          # layer ids 2 * block + layer, in launch order
        a_pix, ba_pix, a_vec, ba_vec, w2_vec = [], [], [], [], []
        for k in range(n_blocks):
            pixel = map3d_mode == "all" or k in mod_blocks
            bd = desc.block[k]
            bd.skip = int(k >= n_blocks // 2)
            bd.to_rgb = int(k >= n_blocks // 2 - 1)
            for s in range(2):
                name = f"{prefix}.network.m3d_{k}.mod{s + 1}"
                w = g(name + ".weight").reshape(C, C)              # [Cin, Cout]
                A, bA = g(name + ".affine.weight"), g(name + ".affine.bias")          # [Cin, F], [Cin]
                d = bd.layer[s]
                d.w = add(pack_matrix(w.t(), KBH, NT))
                d.bias = add(_pad(g(name + ".bias"), HdP))
                if pixel:
                    d.pixel_style = 1
                    d.map_offset = HdP * len(self.pixel_ids)
                    self.pixel_ids.append(2 * k + s)
                    d.w2 = add(pack_matrix((w * w).t(), KBH, NT))
                    At = torch.zeros(F, HdP, dtype=torch.float32, device=device)
                    At[:, :C] = A.t()
                    a_pix.append(At)
                    ba_pix.append(_pad(bA + 1.0, HdP))
                else:
                    d.pixel_style = 0
                    d.vec_index = len(self.vec_ids)
                    self.vec_ids.append(2 * k + s)
                    a_vec.append(A)
                    ba_vec.append(bA + 1.0)
                    w2_vec.append(w * w)
            if bd.to_rgb:
                tr = f"{prefix}.to_rgbs.m3d_{k}.linear"
                wr = g(tr + ".weight").reshape(3, C)
                bd.w_rgb = add(torch.cat([_pad(wr[0], HdP), _pad(wr[1], HdP), _pad(wr[2], HdP), _pad(g(tr + ".bias"), 4)]))
        self.desc = desc
        self.blob = torch.cat(chunks).contiguous()
        self.m_channels = HdP * len(self.pixel_ids)
        if self.pixel_ids:
            self.a_pix_t = torch.cat(a_pix, dim=1).contiguous()          # [F, HdP * n_pixel]: every modulation map in one GEMM
            self.ba_pix = torch.cat(ba_pix)                               # [HdP * n_pixel]  b_A + 1, zero in the padding
        if self.vec_ids:
            self.a_vec, self.ba_vec = torch.stack(a_vec), torch.stack(ba_vec)      # [nv, C, F], [nv, C]
            self.w2_vec = torch.stack(w2_vec)                                       # [nv, Cin, Cout]
        self.engine = "f32"

    def layer_tables(self, feature_maps, fixed_style):
        """feature_maps [B, R, F] (rendered, channels last), fixed_style [B, F] ->
        (M [B, R, HdP * n_pixel] low-resolution modulation maps or None, md [B, n_vec, 2, HdP] per-image (m, d) or None)."""
        B = fixed_style.shape[0]
        M = md = None
        if self.pixel_ids:
            c = self.ba_pix.unsqueeze(0)
            if self.mode in ("all", "mixed"):           # style = feature map + fixed style: the fixed term joins the bias
                c = c + fixed_style @ self.a_pix_t
            M = torch.matmul(feature_maps, self.a_pix_t)
            M += c.unsqueeze(1)
            M = M.contiguous()
        if self.vec_ids:
            m = torch.einsum("bf,vcf->bvc", fixed_style, self.a_vec) + self.ba_vec
            d = torch.rsqrt(torch.einsum("bvc,vco->bvo", m * m, self.w2_vec) + EPS)
            md = torch.zeros(B, len(self.vec_ids), 2, self.HdP, device=fixed_style.device, dtype=torch.float32)
            md[:, :, 0, : self.C] = m
            md[:, :, 1, : self.C] = d
        return M, md

    def run(self, feature_maps, fixed_style, render_hw, out_hw, owner=None):
        """-> rgb [B,3,H,W]."""
        B = fixed_style.shape[0]
        Hr, Wr = render_hw
        H, W = out_hw
        lib = _lib.load()
        if lib.h3d_synthesis_mod_lds_bytes(self.C) < 0:
            raise _lib.H3DError(f"h3d_synthesis_mod: width {self.C} exceeds what the kernel's LDS plan holds (512)")
        if tuple(feature_maps.shape) != (B, Hr * Wr, self.F) or tuple(fixed_style.shape) != (B, self.F):
            raise ValueError(f"feature maps {tuple(feature_maps.shape)} / style {tuple(fixed_style.shape)} do not match "
                             f"[{B}, {Hr}*{Wr}, {self.F}] / [{B}, {self.F}]")
        _lib.need_cuda(feature_maps, fixed_style, self.blob)
        with stage(owner, "synthesis_tables"):
            M, md = self.layer_tables(feature_maps.float(), fixed_style.float())
        rgb = torch.empty(B, 3, H, W, device=fixed_style.device, dtype=torch.float32)
        with stage(owner, "synthesis"):
            rc = lib.h3d_synthesis_mod(_lib.ptr(self.blob), ctypes.byref(self.desc), _lib.ptr(M), self.m_channels, Hr, Wr,
                                       _lib.ptr(md), len(self.vec_ids), _lib.ptr(rgb), B, H, W, _lib.stream_handle())
        _lib.check(rc, "h3d_synthesis_mod")
        return rgb


class LayerwiseModSynthesis:
    """The same network layer by layer from the stand-alone entry points: h3d_bilinear_resize_cl for the style,
    h3d_modconv1x1 per layer (components/map3d_layers.py: SpatialStyleModLayer), torch for the coordinate input, the
    activations, the skip additions and ToRGB.  Every [B, H*W, C] activation goes through HBM: this is the cross-check of the
    fused engine and the baseline of tools/modsynth_bench.py, not an inference path.  Widths up to 256 (h3d_modconv1x1)."""

    def __init__(self, state, prefix, input_prefix, n_blocks, mod_blocks, map3d_mode, device):
        from ..components.map3d_layers import SpatialStyleModLayer
        g = lambda k: state[k].detach().to(device=device, dtype=torch.float32)
        self.n_blocks, self.mod_blocks, self.mode = n_blocks, list(mod_blocks), map3d_mode
        self.w_in = g(f"{input_prefix}.network.0.weight").flatten(1)            # [C, 2]
        self.b_in = g(f"{input_prefix}.network.0.bias")
        self.layers, self.rgb = [], {}
        for k in range(n_blocks):
            for s in (1, 2):
                name = f"{prefix}.network.m3d_{k}.mod{s}"
                w = g(name + ".weight")
                layer = SpatialStyleModLayer(w.shape[2], w.shape[3], style_dim=g(name + ".affine.weight").shape[1])
                layer.load_state_dict({"weight": w, "bias": g(name + ".bias"), "affine.weight": g(name + ".affine.weight"),
                                       "affine.bias": g(name + ".affine.bias")})
                self.layers.append(layer.to(device).requires_grad_(False))
            if k >= n_blocks // 2 - 1:
                self.rgb[k] = (g(f"{prefix}.to_rgbs.m3d_{k}.linear.weight"), g(f"{prefix}.to_rgbs.m3d_{k}.linear.bias"))

    @torch.no_grad()
    def __call__(self, feature_maps, fixed_style, render_hw, out_hw):
        from ..components.resample import bilinear_resize_cl
        B, (H, W) = fixed_style.shape[0], out_hw
        dev = fixed_style.device
        style = bilinear_resize_cl(feature_maps.float(), render_hw, out_hw)                  # [B, H*W, F]
        fixed = fixed_style.float()[:, None].expand_as(style)
        i = torch.linspace(-1, 1, H, device=dev).view(H, 1).expand(H, W)
        j = torch.linspace(-1, 1, W, device=dev).view(1, W).expand(H, W)
        x = torch.sin(torch.stack([i, j], dim=-1).reshape(H * W, 2) @ self.w_in.t() + self.b_in)
        x = x.unsqueeze(0).expand(B, -1, -1).contiguous()
        both = style + fixed if self.mode in ("all", "mixed") else None
        fixed = fixed.contiguous()
        rgb = None
        for k in range(self.n_blocks):
            pixel = self.mode == "all" or k in self.mod_blocks
            s = fixed if not pixel else style if self.mode == "isolated" else both
            x_in = x
            for layer in self.layers[2 * k: 2 * k + 2]:
                x = torch.nn.functional.leaky_relu(layer(x, s), 0.2)
            if k >= self.n_blocks // 2:
                x = x + x_in
            if k in self.rgb:
                out = torch.addmm(self.rgb[k][1], x.flatten(0, 1), self.rgb[k][0].t())
                rgb = out if rgb is None else out + rgb
        return rgb.view(B, H * W, 3).transpose(1, 2).reshape(B, 3, H, W).contiguous()
