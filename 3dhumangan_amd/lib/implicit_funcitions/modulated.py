"""COORDCONCATSIREN -- the pluggable pose-conditioned implicit function (reference:
lib/implicit_funcitions/modulated.py:6-75), evaluated by the fp32-MFMA HIP kernel behind
h3d_neural_field / h3d_render_fused.

Same constructor arguments, same parameter names (so reference state_dicts load unchanged), same forward
signature and output channel order [rgb(3), feat(F), sigma(1)].  `.eval()`: the fused inference kernels (no autograd
through them).  `.train()` (or ``differentiable=True``): the differentiable evaluation of lib/generators/differentiable.py --
library GEMMs + the HIP film_sin kernels with hand-written adjoints.
"""
import ctypes
import math
import os
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from ... import _lib
from ..generators.volume_rendering import _CLAMP


class _Engine(NamedTuple):
    """One arithmetic engine of the field: its entry points of the C ABI (include/h3d.h) and what a launch needs to know."""
    name: str
    pack_size: str
    pack: str
    device_pack: Optional[str]     # the packer's device-side twin (csrc/field_x3.hip: field_pack_kernel)
    field: str
    render: str                    # fused field + integration
    render_geo: Optional[str]      # ... that builds the geometry features itself (A4 inside the render, csrc/field_x3.hip GEOIN)
    tile: int                      # sample tile of the fused kernels
    tier: tuple                    # extra trailing arguments (before the stream) of the field / render entry points


_ENGINES = {e.name: e for e in (
    _Engine("f16x3", "h3d_field_pack_x3_size", "h3d_field_pack_x3", "h3d_field_pack_x3_device", "h3d_neural_field_x3",
            "h3d_render_fused_x3", "h3d_render_fused_x3_geo", 32, ()),
    _Engine("f16x2", "h3d_field_pack_x2_size", "h3d_field_pack_x2", "h3d_field_pack_x2_device", "h3d_neural_field_x2",
            "h3d_render_fused_x2", "h3d_render_fused_x2_geo", 32, ()),
    _Engine("f16x3t", "h3d_field_pack_x3t_size", "h3d_field_pack_x3t", None, "h3d_neural_field_x3t", "h3d_render_fused_x3t", None, 64, ()),
    _Engine("f16x1t", "h3d_field_pack_x3t_size", "h3d_field_pack_x3t", None, "h3d_neural_field_x3t_tier", "h3d_render_fused_x3t_tier",
            None, 64, (1,)),
    _Engine("f16x2t", "h3d_field_pack_x3t_size", "h3d_field_pack_x2t", None, "h3d_neural_field_x3t_tier", "h3d_render_fused_x3t_tier",
            None, 64, (4,)),
    _Engine("f32", "h3d_field_pack_size", "h3d_field_pack", None, "h3d_neural_field", "h3d_render_fused", None, 64, ()),
)}


class _Dense(nn.Module):
    """Holder that reproduces the reference's `<name>.layer.{weight,bias}` parameter paths."""

    def __init__(self, n_in, n_out):
        super().__init__()
        self.layer = nn.Linear(n_in, n_out)


def _uniform_(linear, bound):
    with torch.no_grad():
        linear.weight.uniform_(-bound, bound)


class COORDCONCATSIREN(nn.Module):

    def __init__(self, input_dim=2, latent_dim=100, hidden_dim=256, geo_feature_dim=88, output_dim=1, feature_dim=32,
                 num_blocks=9, device=None):
        super().__init__()
        if input_dim != 3 or geo_feature_dim != 31 or num_blocks != 4:
            raise NotImplementedError("the HIP field kernel is built for input_dim=3, geo_feature_dim=31, 4 FiLM blocks "
                                      "(every shipped config); got "
                                      f"{input_dim}/{geo_feature_dim}/{num_blocks}")
        self.device = device
        self.input_dim, self.latent_dim, self.hidden_dim = input_dim, latent_dim, hidden_dim
        self.geo_feature_dim, self.output_dim, self.feature_dim = geo_feature_dim, output_dim, feature_dim
        H = hidden_dim
        self.first_layer_coord = _Dense(input_dim, H)
        self.first_layer_mod = _Dense(geo_feature_dim, H)
        self.network = nn.ModuleList([_Dense(2 * H, H)] + [_Dense(H, H) for _ in range(num_blocks - 1)])
        self.sigma_layer = nn.Linear(H, 1)
        self.color_layer_sine = _Dense(H + 3, H)
        self.color_layer_linear = nn.Linear(H, 3)
        self.feature_layer_linear = nn.Linear(H, feature_dim)
        # SIREN initialisation (reference pigan_layers.py:26-53): U(+-sqrt(6/fan_in)/25), first layers U(+-1/fan_in)
        for lin in [d.layer for d in self.network] + [self.sigma_layer, self.color_layer_sine.layer,
                                                      self.color_layer_linear, self.feature_layer_linear]:
            _uniform_(lin, math.sqrt(6.0 / lin.weight.shape[1]) / 25.0)
        for lin in (self.first_layer_coord.layer, self.first_layer_mod.layer):
            _uniform_(lin, 1.0 / lin.weight.shape[1])
        self._packed = {}
        # Arithmetic engine (all meet the 1e-3 parity budget):
        #   "f16x2"   as f16x3 with the two cross products of a contraction in one block-scaled fp6 instruction (widths <= 256)
        #   "f16x3"   split-operand f16 matrix cores, activations register-resident (widths <= 256)
        #   "f16x2t"  the x2 arithmetic on the LDS-resident engine, any width <= 448
        #   "f16x3t"  split-operand f16 matrix cores, activations LDS-resident, any width <= 448 (MAP3DBN 384, MAP3DBN512L 420)
        #   "f32"     fp32 matrix cores (any width <= 512)
        # and, NOT within the 1e-3 budget (the "fp16 MFMA path" tier of BASELINE config 5, ~1e-2 on the render; opt-in):
        #   "f16x1t"  plain f16 matrix-core products on the f16x3t engine (one product instead of three)
        widest = max(hidden_dim, feature_dim)
        default = "f16x2" if widest <= 256 else "f16x2t" if widest <= 448 else "f32"
        self.precision = os.environ.get("H3D_FIELD_PRECISION", default)
        # x2 render: refinement of ill-conditioned last samples on the three-product engine (render_geo; round 6)
        self.refine_last_sample = os.environ.get("H3D_FIELD_REFINE", "1") != "0"
        # weights packed on the device they live on (round 6); False: D2H copy + host packer + H2D copy -- the same bytes
        self.device_pack = True
        self.refine_eps = float(os.environ.get("H3D_FIELD_REFINE_EPS", "1e-3"))
        self.refine_capacity = int(os.environ.get("H3D_FIELD_REFINE_CAP", "128"))       # listed units per batch item
        self._refine_buf = None
        self._sigma_scale_cache = None

    # ---- weight packing (host, once per weight version)
    def _params_for_pack(self):
        return [self.first_layer_coord.layer, self.first_layer_mod.layer] + [d.layer for d in self.network] + \
               [self.sigma_layer, self.color_layer_sine.layer, self.color_layer_linear, self.feature_layer_linear]

    def _engine(self, precision=None):
        name = self.precision if precision is None else precision
        if name not in _ENGINES:
            raise ValueError(f"unknown precision {name!r}")
        return _ENGINES[name]

    def fused_supported(self, num_steps, precision=None):
        """Sample counts the fused field+integration kernel of the engine (None: the module's own) accepts."""
        S, tile = int(num_steps), self._engine(precision).tile
        return (8 <= S <= tile and S & (S - 1) == 0) or (S > tile and S % tile == 0)

    def render_geo_supported(self, num_steps, precision=None):
        return self._engine(precision).render_geo is not None and self.fused_supported(num_steps, precision)

    def packed_weights(self, device, precision=None):
        """Device blob in MFMA fragment order (csrc/field_common.hpp, csrc/field_x3.hip) for the engine (None: the module's own);
        cached until a parameter changes."""
        device = _lib.canonical_device(device)
        lins = self._params_for_pack()
        eng = self._engine(precision)
        key = (str(device), eng.pack) + tuple((p.data_ptr(), p._version) for l in lins for p in (l.weight, l.bias))
        hit = self._packed.get(eng.pack)                 # engines that share a packer share the blob
        if hit is not None and hit[0] == key:
            return hit[1]
        lib = _lib.load()
        H, F = self.hidden_dim, self.feature_dim
        on_device = (self.device_pack and eng.device_pack is not None and device.type == "cuda"
                     and all(p.device == device for l in lins for p in (l.weight, l.bias)))
        if on_device:
            # round 6: packed where the parameters live (one memset + one launch, no synchronisation, bit-identical blob) -- what lets
            # a weight that changes every optimiser step use the fused render (the D step's no-grad generator forward)
            host = [(l.weight.detach().float().contiguous(), l.bias.detach().float().contiguous()) for l in lins]
        else:
            host = [(l.weight.detach().float().cpu().contiguous(), l.bias.detach().float().cpu().contiguous()) for l in lins]
        P = _lib.FieldParams()
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        P.w_coord, P.b_coord = vp(host[0][0]), vp(host[0][1])
        P.w_geo, P.b_geo = vp(host[1][0]), vp(host[1][1])
        for k in range(4):
            P.w_film[k], P.b_film[k] = host[2 + k][0].data_ptr(), host[2 + k][1].data_ptr()
        P.w_sigma, P.b_sigma = vp(host[6][0]), vp(host[6][1])
        P.w_color, P.b_color = vp(host[7][0]), vp(host[7][1])
        P.w_rgb, P.b_rgb = vp(host[8][0]), vp(host[8][1])
        P.w_feat, P.b_feat = vp(host[9][0]), vp(host[9][1])
        nbytes = getattr(lib, eng.pack_size)(H, F)
        if nbytes <= 0:
            raise _lib.H3DError(f"field engine {eng.name} does not support widths {H}/{F}")
        if on_device:
            with torch.cuda.device(device):
                dev_blob = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
                rc = getattr(lib, eng.device_pack)(ctypes.byref(P), H, F, _lib.ptr(dev_blob), _lib.stream_handle())
            _lib.check(rc, eng.device_pack)
        else:
            blob = torch.empty((nbytes + 3) // 4, dtype=torch.float32)
            _lib.check(getattr(lib, eng.pack)(ctypes.byref(P), H, F, ctypes.c_void_p(blob.data_ptr())), "h3d_field_pack")
            dev_blob = blob.to(device)
        self._packed[eng.pack] = (key, dev_blob)
        return dev_blob

    def forward(self, input, frequencies, phase_shifts, geo_feature, ray_directions, input_scaler=1.,
                geo_feature_scaler=1., differentiable=None, precision=None, **kwargs):
        """input [B,N,3], frequencies/phase_shifts [B,4H], geo_feature [B,N,31], ray_directions [B,N,3] or None
        (None == the lock_view_dependence direction (0,0,-1))  ->  [B,N,F+4].  `precision`: the engine of the fused kernel for
        this call (None: the module's own; the differentiable evaluation has one arithmetic)."""
        if self.training if differentiable is None else differentiable:
            from ..generators.differentiable import field_forward
            _lib.need_cuda(input, frequencies, phase_shifts, geo_feature, ray_directions)
            if input.dim() < 3:
                out = field_forward(self, input.unsqueeze(1), frequencies, phase_shifts, geo_feature.unsqueeze(1),
                                    None if ray_directions is None else ray_directions.unsqueeze(1), input_scaler,
                                    geo_feature_scaler)
                return out.squeeze(1)
            return field_forward(self, input, frequencies, phase_shifts, geo_feature, ray_directions, input_scaler,
                                 geo_feature_scaler)
        with torch.no_grad():
            return self._forward_fused(input, frequencies, phase_shifts, geo_feature, ray_directions, input_scaler,
                                       geo_feature_scaler, precision)

    def _prepare(self, input, ray_directions, frequencies, phase_shifts, z_vals=None, num_steps=None, noise=None,
                 clamp_mode="relu"):
        """The operands every launch shares as contiguous fp32 -> (points, directions or None, frequencies, phases, render), where
        `render` is None without z_vals and else (z_vals [B,R,S], noise [B,R,S] or None, the outputs features [B,R,F+3], depth
        [B,R,1] and weights [B,R,S,1], the clamp code).  The caller binds all of it to locals until after its launch: _lib.ptr
        keeps only the address, a temporary would be freed before the kernel runs (components/smpl.py: get_geo_features)."""
        f32 = lambda t: None if t is None else t.contiguous().float()
        pts, dirs, fr, ph = f32(input), f32(ray_directions), f32(frequencies), f32(phase_shifts)
        if z_vals is None:
            return pts, dirs, fr, ph, None
        B, S = pts.shape[0], int(num_steps)
        R = pts.shape[1] // S
        z, nz = f32(z_vals.reshape(B, R, S)), None if noise is None else f32(noise.reshape(B, R, S))
        feats = torch.empty((B, R, self.feature_dim + 3), device=pts.device, dtype=torch.float32)
        depth = torch.empty((B, R, 1), device=pts.device, dtype=torch.float32)
        weights = torch.empty((B, R, S, 1), device=pts.device, dtype=torch.float32)
        return pts, dirs, fr, ph, (z, nz, feats, depth, weights, _CLAMP[clamp_mode])

    def _forward_fused(self, input, frequencies, phase_shifts, geo_feature, ray_directions, input_scaler=1.,
                       geo_feature_scaler=1., precision=None):
        unsq = input.dim() < 3
        if unsq:
            input, geo_feature = input.unsqueeze(1), geo_feature.unsqueeze(1)
            ray_directions = None if ray_directions is None else ray_directions.unsqueeze(1)
        _lib.need_cuda(input, frequencies, phase_shifts, geo_feature, ray_directions)
        B, N, _ = input.shape
        H, F = self.hidden_dim, self.feature_dim
        eng = self._engine(precision)
        pts, dirs, fr, ph, _ = self._prepare(input, ray_directions, frequencies, phase_shifts)
        geo = geo_feature if geo_feature_scaler == 1. else geo_feature * geo_feature_scaler
        geo = geo.contiguous().float()
        assert fr.shape == (B, 4 * H) and ph.shape == (B, 4 * H)
        out = torch.empty((B, N, F + 4), device=pts.device, dtype=torch.float32)
        blob = self.packed_weights(pts.device, precision)
        rc = getattr(_lib.load(), eng.field)(_lib.ptr(blob), _lib.ptr(pts), _lib.ptr(geo), _lib.ptr(dirs), _lib.ptr(fr), _lib.ptr(ph),
                                             _lib.ptr(out), B, N, H, F, geo.shape[-1], float(input_scaler), *eng.tier,
                                             _lib.stream_handle())
        _lib.check(rc, "h3d_neural_field")
        return out.squeeze(1) if unsq else out

    @torch.no_grad()
    def render(self, input, frequencies, phase_shifts, geo_feature, ray_directions, z_vals, num_steps, input_scaler=1.,
               noise=None, clamp_mode="relu", last_back=False, white_back=False, precision=None):
        """Fused field evaluation + volume integration (reference: COORDCONCATSIREN.forward followed by
        volume_rendering.ray_integration) on the engine `precision` (None: the module's own).  input [B,R*S,3] with the S
        samples of a ray contiguous.  -> (features [B,R,F+3], depth [B,R,1], weights [B,R,S,1])."""
        _lib.need_cuda(input, frequencies, phase_shifts, geo_feature, ray_directions, z_vals, noise)
        eng = self._engine(precision)
        pts, dirs, fr, ph, (z, nz, feats, depth, weights, mode) = self._prepare(input, ray_directions, frequencies, phase_shifts,
                                                                                 z_vals, num_steps, noise, clamp_mode)
        geo = geo_feature.contiguous().float()
        B, R, S = z.shape
        blob = self.packed_weights(pts.device, precision)
        rc = getattr(_lib.load(), eng.render)(_lib.ptr(blob), _lib.ptr(pts), _lib.ptr(geo), _lib.ptr(dirs), _lib.ptr(fr), _lib.ptr(ph),
                                              _lib.ptr(z), _lib.ptr(nz), _lib.ptr(feats), _lib.ptr(depth), _lib.ptr(weights), B, R, S,
                                              self.hidden_dim, self.feature_dim, geo.shape[-1], float(input_scaler), mode,
                                              int(bool(last_back)), int(bool(white_back)), *eng.tier, _lib.stream_handle())
        _lib.check(rc, "h3d_render_fused")
        return feats, depth, weights

    @torch.no_grad()
    def render_geo(self, input, frequencies, phase_shifts, nn_index, skeletons, vertices, tpose_vertices, vertex_ik,
                   ray_directions, z_vals, num_steps, legacy_mode=False, input_scaler=1., noise=None, clamp_mode="relu",
                   last_back=False, white_back=False, precision=None):
        """`render` with the geometry features built inside the kernel (reference: get_geo_features,
        lib/components/smpl.py:210-249, then COORDCONCATSIREN.forward and ray_integration): instead of geo_feature [B,N,31] it
        takes nn_index [B,N] int32 (smpl.nearest_vertex), skeletons [B,24,3], vertices / tpose_vertices [B,V,3] and
        vertex_ik [B,V,16] (smpl.vertex_inverse_transforms).  -> (features [B,R,F+3], depth [B,R,1], weights [B,R,S,1])."""
        _lib.need_cuda(input, frequencies, phase_shifts, nn_index, skeletons, vertices, tpose_vertices, vertex_ik,
                       ray_directions, z_vals, noise)
        eng = self._engine(precision)
        if eng.render_geo is None:
            raise ValueError(f"field engine {eng.name} has no fused render with in-kernel geometry")
        B, N, _ = input.shape
        idx = nn_index.contiguous()
        if idx.dtype != torch.int32 or tuple(idx.shape) != (B, N):
            raise ValueError("nn_index must be int32 [B, N]")
        sk, vt = skeletons.contiguous().float(), vertices.contiguous().float()
        tv, vik = tpose_vertices.contiguous().float(), vertex_ik.contiguous().float()
        if sk.shape[1:] != (24, 3) or vik.shape[1:] != (vt.shape[1], 16) or tv.shape != vt.shape:
            raise ValueError("skeletons [B,24,3], vertices / tpose_vertices [B,V,3], vertex_ik [B,V,16] expected")
        pts, dirs, fr, ph, (z, nz, feats, depth, weights, mode) = self._prepare(input, ray_directions, frequencies, phase_shifts,
                                                                                 z_vals, num_steps, noise, clamp_mode)
        _, R, S = z.shape
        blob = self.packed_weights(pts.device, precision)
        lib = _lib.load()
        common = lambda b: (_lib.ptr(b), _lib.ptr(pts), _lib.ptr(idx), _lib.ptr(sk), _lib.ptr(vt), _lib.ptr(tv), _lib.ptr(vik),
                            vt.shape[1], int(bool(legacy_mode)), _lib.ptr(dirs), _lib.ptr(fr), _lib.ptr(ph), _lib.ptr(z), _lib.ptr(nz),
                            _lib.ptr(feats), _lib.ptr(depth), _lib.ptr(weights), B, R, S, self.hidden_dim, self.feature_dim,
                            float(input_scaler), mode, int(bool(last_back)), int(bool(white_back)))
        if eng.name == "f16x2" and self.refine_last_sample:
            # Round 6: rays whose LAST sample's density lies within `refine_eps` of zero (relative to the ray's largest density, floored
            # by the density head's weight norm) are listed by the x2 launch and redone by the three-product engine right behind it:
            # the reference's delta = 1e9 on the last sample (lib/generators/volume_rendering.py:21) turns the SIGN of that density
            # into an alpha of 0 or 1, and the x2 arithmetic's ~1e-4 density error must not decide it.  No host synchronisation.
            cap = self.refine_capacity
            buf = self._refine_buf
            if buf is None or buf[0].device != pts.device or buf[0].shape != (B, cap):
                buf = (torch.zeros(B, cap, dtype=torch.int32, device=pts.device), torch.zeros(B, dtype=torch.int32, device=pts.device))
                self._refine_buf = buf
            blob3 = self.packed_weights(pts.device, "f16x3")      # the same weights in the x3 format (cached per weight version)
            scale = self._sigma_scale(pts.device)
            rc = lib.h3d_render_fused_x2_geo_ref(*common(blob), float(self.refine_eps), scale, _lib.ptr(buf[0]), _lib.ptr(buf[1]), cap,
                                                 _lib.stream_handle())
            rc = rc or lib.h3d_render_fused_x3_geo_units(*common(blob3), _lib.ptr(buf[0]), _lib.ptr(buf[1]), cap, _lib.stream_handle())
        else:
            rc = getattr(lib, eng.render_geo)(*common(blob), _lib.stream_handle())
        _lib.check(rc, "h3d_render_fused_geo")
        return feats, depth, weights

    def _sigma_scale(self, device):
        """Euclidean norm of the density head's weights (the scale of a density whose inputs are sines), cached per weight version:
        the floor of the refinement threshold's scale."""
        w = self.sigma_layer.weight
        key = (w.data_ptr(), w._version, str(device))
        if self._sigma_scale_cache is None or self._sigma_scale_cache[0] != key:
            self._sigma_scale_cache = (key, float(w.detach().float().norm()))
        return self._sigma_scale_cache[1]

    def refined_units(self):
        """Per-item number of wave units the LAST render_geo call listed for the three-product refinement (device tensor [B]; reading
        it synchronises), or None."""
        return None if self._refine_buf is None else self._refine_buf[1]
