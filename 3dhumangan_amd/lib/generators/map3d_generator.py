"""Map3DGenerator -- drop-in for the reference class of the same name
(lib/generators/map3d_generator.py:101-523): same constructor kwargs (the whole config dict is splatted in), same
state_dict key schema, same ``forward`` / ``staged_forward`` / ``set_device`` / ``generate_avg_latent`` surface and
output dict keys.  In `.eval()` mode every hot stage is a fused HIP kernel behind libh3d.so (in `.train()` mode the
differentiable path of lib/generators/differentiable.py runs instead, see Map3DGenerator.wants_autograd):

    mapping networks (B x L GEMVs)      torch GEMMs on the device + h3d_bias_act        (A1, A2)
    ray set-up                          h3d_ray_setup                                     (A3)
    SMPL geometry features              h3d_geo_features                                  (A4)
    FiLM-SIREN + volume integration     h3d_render_fused  (or h3d_neural_field + h3d_ray_integrate)   (A5, A6)
    resize + synthesis input + 9 SPADE blocks + ToRGB      h3d_synthesis                  (A7, A8, A9)
    (spatial_normalization="none": 9 modulated-conv blocks + ToRGB      h3d_synthesis_mod)
    (disable_render=True: the rasterised body condition -> style feature map, no field / rays      h3d_style_input)
    (2d_label_input / 2d_latent_input: label map / latent as inputs of block 0      h3d_synth_input + the layer-wise path)

The reference forward is stochastic.  The draws happen here at the same places with torch's device
RNG; ``jitter=`` / ``noise=`` kwargs inject explicit tensors instead (used by the parity tests).
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn

from ... import _lib
from ..._stages import stage
from ..components import smpl
from ..components.ops.bias_act import bias_act
from . import geometry_export
from . import volume_rendering as vr
from .differentiable import synthesis_forward
from .modsynth_pack import ModSynthesisPlan
from .style_input_pack import StyleInputPlan, normalize_2nd_moment
from .synthesis_pack import SynthesisPlan


def _consume_camera_rng(sample_dist, batch, device):
    """The reference samples a camera position inside transform_sampled_points and throws it away (the camera comes
    from the conditions): volume_rendering.py:141-143 -> sample_camera_positions (:182-221).  Only the RNG draws
    survive, and they depend on ``sample_dist``; they are mirrored here so that the integration noise drawn afterwards
    comes from the same place of the device RNG stream for every mode:
      'uniform', 'spherical_uniform'   two rand  [B,1]
      'normal', 'gaussian'             two randn [B,1]
      'truncated_gaussian'             two normal_ [B,1,4]   (truncated_normal_, :173-180)
      'hybrid'                         python's random.random() picks the rand or the randn pair
      anything else (None)             no draw"""
    if sample_dist in ("uniform", "spherical_uniform"):
        torch.rand((batch, 1), device=device), torch.rand((batch, 1), device=device)
    elif sample_dist in ("normal", "gaussian"):
        torch.randn((batch, 1), device=device), torch.randn((batch, 1), device=device)
    elif sample_dist == "hybrid":
        import random
        draw = torch.rand if random.random() < 0.5 else torch.randn
        draw((batch, 1), device=device), draw((batch, 1), device=device)
    elif sample_dist == "truncated_gaussian":
        torch.empty((batch, 1, 4), device=device).normal_(), torch.empty((batch, 1, 4), device=device).normal_()


def _integration_noise(given, shape, nerf_noise, device):
    """The noise ray integration adds to the densities: `given` when it is injected, else drawn where the reference draws it
    (volume_rendering.py:24) -- also when nerf_noise == 0 scales it away, which leaves None."""
    if given is not None:
        return given
    drawn = torch.randn(shape, device=device)
    return drawn * nerf_noise if nerf_noise != 0 else None


def _render_route(differentiable, recording, hierarchical_sample, fused, train_field, fuse_geo, device_pack, precision, S,
                  fused_supported, render_geo_supported):
    """Which kernels a render call takes -> (route, field engine, differentiable).  Plain values only: `recording` is
    torch.is_grad_enabled(), `device_pack` / `precision` are the field module's own settings and the two predicates its
    fused_supported(S, engine) / render_geo_supported(S, engine).  First match:

      hierarchical_sample, differentiable                      NotImplementedError
      hierarchical_sample                                      "hierarchical"  coarse + fine pass on the unfused kernels
      differentiable, nothing recording, fused, train_field x3 | x2, device_pack, precision f16x2 | f16x3 that fuses S
                                                               promoted: engine f16x3 | f16x2 by train_field, not differentiable
      fused, not differentiable, engine fuses S, fuse_geo, engine builds the geometry features
                                                               "fused_geo"     nearest-vertex search + render_geo
      fused, not differentiable, engine fuses S                "fused"         geometry features + render
      otherwise                                                "unfused"       geometry features + field tensor + ray integration

    Promotion: a train-mode forward that nothing records (the D step's no-grad generator forward, reference
    lib/trainers/phase_trainer.py:355-362) runs the fused render on device-packed weights; whether S fuses is asked of the
    module's own engine, the call then runs on train_field's."""
    if hierarchical_sample:
        if differentiable:
            raise NotImplementedError("hierarchical_sample=True has no differentiable path (no shipped config trains with it)")
        return "hierarchical", precision, False
    engine = precision
    if (differentiable and not recording and fused and train_field in ("x3", "x2") and device_pack
            and precision in ("f16x2", "f16x3") and fused_supported(S, precision)):
        engine, differentiable = "f16x3" if train_field == "x3" else "f16x2", False
    can_fuse = fused and not differentiable and fused_supported(S, engine)
    if can_fuse and fuse_geo and render_geo_supported(S, engine):
        return "fused_geo", engine, differentiable
    return "fused" if can_fuse else "unfused", engine, differentiable


class LatentPool(nn.Module):
    """reference lib/components/util.py:16-29."""

    def __init__(self, pool_size, latent_dim):
        super().__init__()
        self.latents = nn.Parameter(torch.zeros([pool_size, latent_dim]), requires_grad=True)

    def init(self, latents):
        with torch.no_grad():
            self.latents.copy_(latents)

    def forward(self, indices):
        return self.latents[indices]


class MappingNetwork(nn.Module):
    """FiLM frequency/phase mapping (reference lib/components/mapping_networks.py:13-41)."""

    def __init__(self, latent_dim, map_hidden_dim, map_output_dim):
        super().__init__()
        self.network = nn.Sequential(nn.Linear(latent_dim, map_hidden_dim), nn.LeakyReLU(0.2, inplace=True),
                                     nn.Linear(map_hidden_dim, map_hidden_dim), nn.LeakyReLU(0.2, inplace=True),
                                     nn.Linear(map_hidden_dim, map_hidden_dim), nn.LeakyReLU(0.2, inplace=True),
                                     nn.Linear(map_hidden_dim, map_output_dim))
        for m in self.network:
            if isinstance(m, nn.Linear):
                nn.init.kaiming_normal_(m.weight, a=0.2, mode="fan_in", nonlinearity="leaky_relu")
        with torch.no_grad():
            self.network[-1].weight *= 0.25

    def forward(self, z):
        out = self.network(normalize_2nd_moment(z.to(torch.float32)))
        half = out.shape[-1] // 2
        return out[..., :half], out[..., half:]


class FullyConnectedLayer(nn.Module):
    """Equalised-learning-rate dense layer holding the parameters of the reference's FullyConnectedLayer
    (mapping_networks.py:92-121: weight stored divided by lr_multiplier, raw bias; same state_dict keys).  Inference
    form: the runtime gains are folded into an effective (W^T, b) pair once per weight version, the product is one
    library GEMM and bias + activation go through the HIP bias_act op."""

    def __init__(self, in_features, out_features, bias=True, activation="linear", lr_multiplier=1, bias_init=0):
        super().__init__()
        self.activation = activation
        self.weight = nn.Parameter(torch.randn(out_features, in_features) * (1.0 / lr_multiplier))
        self.bias = nn.Parameter(torch.full((out_features,), float(bias_init))) if bias else None
        self.weight_gain = lr_multiplier / math.sqrt(in_features)      # callers may rescale it (implicit branch: x0.2)
        self.bias_gain = lr_multiplier
        self._folded = (None, None, None)

    def folded(self):
        """(W^T * weight_gain [in, out], b * bias_gain or None), rebuilt when a parameter or a gain changes."""
        key = (self.weight.data_ptr(), self.weight._version, self.weight_gain, self.bias_gain,
               None if self.bias is None else (self.bias.data_ptr(), self.bias._version))
        if self._folded[0] != key:
            wt = (self.weight.detach().float() * self.weight_gain).t().contiguous()
            b = None if self.bias is None else self.bias.detach().float() * self.bias_gain
            self._folded = (key, wt, b)
        return self._folded[1], self._folded[2]

    def forward(self, x):
        if torch.is_grad_enabled() and (self.weight.requires_grad or x.requires_grad):
            # training form: the gains stay in the graph (equalised learning rate), bias_act is differentiable
            wt = (self.weight.float() * self.weight_gain).t()
            b = None if self.bias is None else self.bias.float() * self.bias_gain
        else:
            wt, b = self.folded()
        # [B, 512] x [512, 512] products: under float16 autocast they stay in fp32 (round 6) -- autocast would convert the activation
        # and both parameters of every layer and call (the folded weight is a non-leaf, so its conversion is never cached) for a
        # product that costs nothing: 3 launches + 3 in the backward per layer, ~100 launches per iteration
        with torch.autocast("cuda", enabled=False):
            y = x.float() @ wt
            if self.activation == "linear":
                return y if b is None else y + b
            return bias_act(y, b, act=self.activation)


class TwoPartMappingNetwork(nn.Module):
    """reference mapping_networks.py:124-216 with c_dim == 0 (the only use)."""

    def __init__(self, z_dim, c_dim, implicit_dim, w_dim, num_ws, trunk_layers=6, branch_layers=2, activation="lrelu",
                 lr_multiplier=0.01, **_):
        super().__init__()
        if c_dim != 0:
            raise NotImplementedError("label conditioning (c_dim > 0) is not used by any config")
        self.z_dim, self.w_dim, self.num_ws = z_dim, w_dim, num_ws
        self.trunk_layers, self.branch_layers = trunk_layers, branch_layers
        dims = [z_dim] + [w_dim] * trunk_layers
        for i in range(trunk_layers):
            setattr(self, f"trunk{i}", FullyConnectedLayer(dims[i], dims[i + 1], activation=activation, lr_multiplier=lr_multiplier))
        ich = [w_dim] * branch_layers + [implicit_dim]
        sch = [w_dim] * branch_layers + [w_dim]
        for i in range(branch_layers):
            setattr(self, f"implicit{i}", FullyConnectedLayer(ich[i], ich[i + 1], lr_multiplier=lr_multiplier,
                                                             activation="linear" if i == branch_layers - 1 else activation))
            setattr(self, f"superres{i}", FullyConnectedLayer(sch[i], sch[i + 1], activation=activation, lr_multiplier=lr_multiplier))
        getattr(self, f"implicit{branch_layers - 1}").weight_gain *= 0.2

    def forward(self, z, c=None, **_):
        assert z.shape[1] == self.z_dim
        x = normalize_2nd_moment(z.to(torch.float32))
        for i in range(self.trunk_layers):
            x = getattr(self, f"trunk{i}")(x)
        xi, xs = x, x
        for i in range(self.branch_layers):
            xi = getattr(self, f"implicit{i}")(xi)
            xs = getattr(self, f"superres{i}")(xs)
        if self.num_ws is not None:
            xs = xs.unsqueeze(1).repeat([1, self.num_ws, 1])
        return xi, xs


# ---- parameter holders that reproduce the reference's state_dict paths for the synthesis side ---------------

class _SpectralConv(nn.Module):
    """nn.utils.spectral_norm(nn.Conv2d(cin, cout, 1)) as stored: bias, weight_orig, weight_u, weight_v."""

    def __init__(self, cin, cout):
        super().__init__()
        w = torch.empty(cout, cin, 1, 1)
        nn.init.kaiming_normal_(w, a=0.2, mode="fan_in", nonlinearity="leaky_relu")
        self.bias = nn.Parameter(torch.zeros(cout))
        self.weight_orig = nn.Parameter(w)
        u, s, vh = torch.linalg.svd(w.flatten(1), full_matrices=False)
        self.register_buffer("weight_u", u[:, 0].clone())
        self.register_buffer("weight_v", vh[0].clone())


class _BatchNormStats(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


def _conv1x1(cin, cout):
    m = nn.Conv2d(cin, cout, kernel_size=1)
    nn.init.kaiming_normal_(m.weight, a=0.2, mode="fan_in", nonlinearity="leaky_relu")
    return m


class _Spade(nn.Module):
    def __init__(self, c, style_dim):
        super().__init__()
        self.first_norm = _BatchNormStats(c)
        self.mlp_shared = nn.Sequential(_conv1x1(style_dim, 128), nn.ReLU())
        self.mlp_gamma = _conv1x1(128, c)
        self.mlp_beta = _conv1x1(128, c)


class _SpadeBlock(nn.Module):
    def __init__(self, cin, cout, style_dim):
        super().__init__()
        self.conv_0 = _SpectralConv(cin, cout)
        self.conv_1 = _SpectralConv(cout, cout)
        self.spade_0 = _Spade(cin, style_dim)
        self.spade_1 = _Spade(cout, style_dim)


class _ToRGB(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.linear = nn.Conv2d(c, 3, 1)
        with torch.no_grad():
            self.linear.weight *= 0.25


class _ModLayer(nn.Module):
    """SpatialStyleModLayer parameters (reference map3d_layers.py:50-55): weight [1,1,Cin,Cout], bias [1,1,Cout], affine."""

    def __init__(self, cin, cout, style_dim):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(1, 1, cin, cout) * math.sqrt(2 / (1 + 0.2 ** 2)) / math.sqrt(cin))
        self.bias = nn.Parameter(torch.zeros(1, 1, cout))
        self.affine = nn.Linear(style_dim, cin)
        nn.init.kaiming_normal_(self.affine.weight, mode="fan_in", nonlinearity="linear")


class _ModBlock(nn.Module):
    """SynthesisBlock parameters (reference map3d_layers.py:92-95)."""

    def __init__(self, cin, cout, style_dim):
        super().__init__()
        self.mod1 = _ModLayer(cin, cout, style_dim)
        self.mod2 = _ModLayer(cout, cout, style_dim)


class _ToRGBLinear(nn.Module):
    """ToRGB(use_conv=False) (reference map3d_layers.py:340-344)."""

    def __init__(self, c):
        super().__init__()
        self.linear = nn.Linear(c, 3)
        with torch.no_grad():
            self.linear.weight *= 0.25


class SynthesisNetwork(nn.Module):
    """Parameters of reference map3d_generator.py:14-55; evaluation goes through SynthesisPlan / h3d_synthesis
    (spatial_normalization="batch_norm": SPADE blocks) or ModSynthesisPlan / h3d_synthesis_mod ("none": modulated blocks)."""

    def __init__(self, input_dim, style_dim, hidden_dim=256, num_blocks=8, mod_blocks=list(range(8)), name_prefix="m3d",
                 spatial_normalization="instance_norm", map3d_mode="isolated", **_):
        super().__init__()
        if spatial_normalization not in ("batch_norm", "none"):
            raise NotImplementedError("only spatial_normalization='batch_norm' (all shipped configs) and 'none' have a HIP kernel")
        self.normalization = spatial_normalization
        self.style_dim, self.num_blocks, self.mod_blocks, self.map3d_mode = style_dim, num_blocks, list(mod_blocks), map3d_mode
        net, rgbs = {}, {}
        cin = input_dim
        for i in range(num_blocks):
            if spatial_normalization == "none":
                net[f"{name_prefix}_{i}"] = _ModBlock(cin, hidden_dim, style_dim)
                rgbs[f"{name_prefix}_{i}"] = _ToRGBLinear(hidden_dim)
            else:
                net[f"{name_prefix}_{i}"] = _SpadeBlock(cin, hidden_dim, style_dim)
                rgbs[f"{name_prefix}_{i}"] = _ToRGB(hidden_dim)
            cin = hidden_dim
        self.network = nn.ModuleDict(net)
        self.to_rgbs = nn.ModuleDict(rgbs)


class _CoordInput(nn.Module):
    """SynthesisInput parameters (reference map3d_layers.py:241-258): network.0 = Conv2d(2, F, 1)."""

    def __init__(self, input_dim, output_dim):
        super().__init__()
        conv = nn.Conv2d(input_dim, output_dim, kernel_size=1)
        nn.init.uniform_(conv.weight, -math.sqrt(9 / input_dim), math.sqrt(9 / input_dim))
        self.network = nn.Sequential(conv)


class _StyleInput(nn.Module):
    """SynthesisStyleInput parameters (reference map3d_layers.py:278-300, built with num_layers=3: two convolutions);
    evaluated through StyleInputPlan / h3d_style_input when a forward passes disable_render=True."""

    def __init__(self, input_dim, latent_dim, output_dim):
        super().__init__()
        self.from_coords = nn.Sequential(nn.Conv2d(input_dim, latent_dim, 1))
        self.network = nn.Sequential(nn.Conv2d(latent_dim * 2, output_dim, 1), nn.LeakyReLU(0.2),
                                     nn.Conv2d(output_dim, output_dim, 1), nn.LeakyReLU(0.2))


class Map3DGenerator(nn.Module):

    def __init__(self, neural_field_cls, **kwargs):
        super().__init__()
        k = kwargs
        self.latent_dim, self.hidden_dim, self.feature_dim = k["latent_dim"], k["hidden_dim"], k["feature_dim"]
        self.geo_feature_dim, self.label_dim = k["geo_feature_dim"], k["label_dim"]
        self.gen_height, self.gen_width = k["gen_height"], k["gen_width"]
        self.disable_modulation = k.get("disable_modulation", False)
        self.legacy_mode = k.get("legacy_mode", False)
        # eval-mode render: nearest-vertex search + fused field kernel that builds the geometry features itself (default), or
        # h3d_geo_features + fused field kernel (H3D_FUSE_GEO=0 / .fuse_geo = False)
        self.fuse_geo = os.environ.get("H3D_FUSE_GEO", "1") != "0"
        # Train-mode forward that nothing records (the D step's no-grad generator forward, reference
        # lib/trainers/phase_trainer.py:355-362): the field + integration run on the fused render with device-packed weights (round 6).
        # "x3" (default): three f16 products, the differentiable path's own error class (~1e-5); "x2": the inference default's tier;
        # "off": lib/generators/differentiable.py as in rounds 2-5.  The field has no batch statistics: train and eval mode coincide.
        self.train_field = os.environ.get("H3D_TRAIN_FIELD", "x3")
        # Block 0's input beyond "sine of the pixel coordinates" (reference :127-131, :140-141, :256-265): the label map as a third
        # coordinate of synthesis_input, the latent as extra channels behind it.  2d_semantic_input widens synthesis_input by
        # semantic_dim but the reference never concatenates the semantics: a no-op with semantic_dim == 0, a failing forward otherwise.
        self.label_input, self.latent_input = bool(k.get("2d_label_input", False)), bool(k.get("2d_latent_input", False))
        if k.get("2d_semantic_input", False) and k.get("semantic_dim", 0) > 0:
            raise NotImplementedError("2d_semantic_input=True with semantic_dim > 0: the reference's own forward fails there (its "
                                      "synthesis_input expects the semantics as channels but they are never concatenated)")
        if k.get("spatial_normalization", "instance_norm") == "none":
            for flag in ("2d_label_input", "2d_latent_input"):
                if k.get(flag, False):
                    raise NotImplementedError(f"{flag}=True with spatial_normalization='none': the modulated-conv engine takes "
                                              "the coordinate input alone")
        self.neural_field = neural_field_cls(output_dim=k["feature_dim"] + 4, latent_dim=k["latent_dim"],
                                             input_dim=k["input_dim"], hidden_dim=k["hidden_dim"],
                                             geo_feature_dim=k["geo_feature_dim"], feature_dim=k["feature_dim"],
                                             num_blocks=k["neural_field_blocks"], device=None)
        self.synthesis_input = _CoordInput(2 + int(self.label_input), k["feature_dim"])
        self.synthesis_style_input = _StyleInput(1 if "segments" in k["condition_modal_gen"] else 3, k["latent_dim"],
                                                 k["feature_dim"])
        self.synthesis_network = SynthesisNetwork(input_dim=k["feature_dim"] + (k["latent_dim"] if self.latent_input else 0),
                                                  style_dim=k["feature_dim"],
                                                  hidden_dim=k["hidden_dim"], num_blocks=k["synthesis_blocks"],
                                                  mod_blocks=k["mod_blocks"], map3d_mode=k.get("map3d_mode", "isolated"),
                                                  spatial_normalization=k.get("spatial_normalization", "instance_norm"))
        self.neural_field_mapping_network = MappingNetwork(latent_dim=k["latent_dim"], map_hidden_dim=k["hidden_dim"],
                                                           map_output_dim=2 * k["neural_field_blocks"] * k["hidden_dim"])
        self.synthesis_mapping_network = TwoPartMappingNetwork(z_dim=k["latent_dim"], c_dim=0, implicit_dim=1,
                                                               w_dim=k["feature_dim"], num_ws=1, trunk_layers=7,
                                                               branch_layers=1, lr_multiplier=0.01)
        self.epoch = 0
        self.step = 0
        self.side_length = k["side_length"]
        self.latent_pool = LatentPool(k["dataset_length"], k["latent_dim"])
        self.device = None
        self.avg_latent = None
        self._avg_latent_key = None
        self._plan = None
        self._plan_key = None
        self._style_plan = None
        self._style_plan_key = None
        self.stage_timer = None          # set to _stages.StageTimer() to collect per-stage HIP-event timings

    # ------------------------------------------------------------------ reference surface
    def set_device(self, device):
        self.device = device
        self.neural_field.device = device

    def _mapping_key(self):
        """Identity + version of every mapping-network tensor: a cached avg_latent is only valid for these weights."""
        return tuple((p.data_ptr(), p._version) for net in (self.neural_field_mapping_network, self.synthesis_mapping_network)
                     for p in net.parameters())

    def generate_avg_latent(self):
        """Mean freq / phase / styles over 10 000 random latents (reference :182-194)."""
        z = torch.randn((10000, self.latent_dim), device=self.neural_field.device)
        fr, ph = self.neural_field_mapping_network(z)
        _, st = self.synthesis_mapping_network(z)
        self.avg_latent = (z.mean(dim=0, keepdim=True), fr.mean(dim=0, keepdim=True), ph.mean(dim=0, keepdim=True),
                           st.mean(dim=0, keepdim=True))
        self._avg_latent_key = self._mapping_key()
        return self.avg_latent

    def cached_avg_latent(self):
        """The cached avg_latent if it was computed from the CURRENT mapping-network weights (load_state_dict, .to() or an
        optimizer step invalidate it), else None."""
        if self.avg_latent is not None and getattr(self, "_avg_latent_key", None) == self._mapping_key():
            return self.avg_latent
        return None

    @torch.no_grad()
    def get_geo_features(self, points, skeletons, vertices, tpose_vertices, fk_matrices, lbs_weights, **kw):
        if self.disable_modulation:
            return torch.zeros(list(points.shape)[:2] + [self.geo_feature_dim], dtype=points.dtype, device=points.device)
        return smpl.get_geo_features(points, skeletons, vertices, tpose_vertices, fk_matrices, lbs_weights,
                                     self.legacy_mode, **kw)

    # ------------------------------------------------------------------ synthesis plan (static packing)
    def synthesis_plan(self, device):
        """Packed synthesis weights for `device` ("cuda", "cuda:0" and torch.device("cuda", 0) name the same plan: an
        engine override set through one spelling must be seen by forward(), which asks with the tensors' device)."""
        device = _lib.canonical_device(device)
        sd = self.state_dict()
        key = (str(device),) + tuple((v.data_ptr(), v._version) for n, v in sd.items()
                                     if n.startswith(("synthesis_network", "synthesis_input")))
        if self._plan is None or self._plan_key != key:
            sn = self.synthesis_network
            plan_cls = ModSynthesisPlan if sn.normalization == "none" else SynthesisPlan
            self._plan = plan_cls(sd, "synthesis_network", "synthesis_input", sn.num_blocks, sn.mod_blocks, sn.map3d_mode, device)
            self._plan_key = key
        return self._plan

    def style_input_plan(self, device):
        """Packed `synthesis_style_input` weights for `device` (the disable_render=True path), cached per weight version."""
        device = _lib.canonical_device(device)
        sd = {"synthesis_style_input." + n: v for n, v in self.synthesis_style_input.state_dict().items()}
        key = (str(device),) + tuple((v.data_ptr(), v._version) for v in sd.values())
        if self._style_plan is None or self._style_plan_key != key:
            self._style_plan = StyleInputPlan(sd, "synthesis_style_input", device)
            self._style_plan_key = key
        return self._style_plan

    # ------------------------------------------------------------------ stages
    def _mapping(self, latent, kwargs):
        with stage(self, "mapping"):
            return self._mapping_impl(latent, kwargs)

    def _mapping_impl(self, latent, kwargs):
        if kwargs.get("neural_field_latent_input", True):
            fr, ph = self.neural_field_mapping_network(latent)
        else:
            fr, ph = self.neural_field_mapping_network(torch.zeros_like(latent))
        _, styles = self.synthesis_mapping_network(latent)
        return fr, ph, styles

    def render(self, *args, differentiable=False, **kwargs):
        """reference :381-523.  -> rgb_render [B,3,Hr,Wr], feature_maps [B,R,F] (channels LAST: it feeds the
        synthesis kernel directly; use .transpose for NCHW), depths [B,R,1], weights [B,R,S,1], None.

        ``staged``/``max_points`` chunking is a memory work-around of the reference and is not needed: the field
        tensor never materialises in the fused path.  ``differentiable=True`` evaluates the field as library GEMMs + HIP
        activation / integration kernels with hand-written adjoints (lib/generators/differentiable.py) instead of the fused
        inference kernel."""
        if differentiable:
            return self._render(*args, differentiable=True, **kwargs)
        with torch.no_grad():
            return self._render(*args, **kwargs)

    def _render(self, freq, phase, conditions, render_width, render_height, ray_start, ray_end, coarse_steps, fine_steps=None,
                h_stddev=0, v_stddev=0, h_mean=0, v_mean=0, hierarchical_sample=False, sample_dist=None,
                lock_view_dependence=False, staged=False, max_points=50000, jitter=None, noise=None, fused=True,
                differentiable=False, noise_coarse=None, fine_u=None, **kwargs):
        nf, c, dev = self.neural_field, conditions, freq.device
        B, S, R, res = freq.shape[0], int(coarse_steps), render_width * render_height, (render_width, render_height)
        route, engine, differentiable = _render_route(differentiable, torch.is_grad_enabled(), hierarchical_sample, fused,
                                                      self.train_field, self.fuse_geo, nf.device_pack, nf.precision, S,
                                                      nf.fused_supported, nf.render_geo_supported)
        focals, scales = c["intrinsics"][:, 0, 0], c["scales"].float()
        mesh = (c["skeletons_xyz"], c["vertices"], c["tpose_vertices"], c["fk_matrices"], c["lbs_weights"])
        nerf_noise, scaler = kwargs.get("nerf_noise", 0), 2.0 / self.side_length
        integ = dict(clamp_mode=kwargs["clamp_mode"], last_back=kwargs.get("last_back", False), white_back=kwargs.get("white_back", False))
        # RNG order of the reference: jitter U(0,1) [B,R,S,1]; the discarded camera sample; integration noise randn
        with stage(self, "ray_setup"):
            pts, z_vals = vr.sample_rays(focals, scales, c["cam2world_matrices"], S, res, ray_start, ray_end, jitter=jitter, perturb=True)
            frame = vr.ray_frame_world(focals, c["cam2world_matrices"], res) if route == "hierarchical" else None
        _consume_camera_rng(sample_dist, B, dev)
        if route == "hierarchical":
            feats, depths, weights = self._render_hierarchical(freq, phase, mesh, pts, z_vals, frame, S if fine_steps is None else int(fine_steps),
                                                               engine, lock_view_dependence, scaler, integ, nerf_noise, noise_coarse, fine_u, noise)
        else:
            noise = _integration_noise(noise, (B, R, S, 1), nerf_noise, dev)
            # "fused_geo": A4 inside the fused render (round 4) -- only the nearest-vertex search runs as its own kernel, the features
            # are built in the field kernel's prologue, the [B, N, 31] tensor is never written (H3D_FUSE_GEO=0: the two-kernel path)
            with stage(self, "geo_features"):
                if route == "fused_geo":
                    vik = smpl.vertex_inverse_transforms(c["fk_matrices"], c["lbs_weights"])
                    nn_index = smpl.nearest_vertex(pts, c["vertices"], ray_shape=(render_height, render_width, S))
                else:
                    geo = self.get_geo_features(pts, *mesh)
            dirs = None if lock_view_dependence else vr.ray_directions_world(focals, c["cam2world_matrices"], res, S)
            if route == "fused_geo":
                with stage(self, "render_fused"):
                    feats, depths, weights = nf.render_geo(pts, freq, phase, nn_index, *mesh[:3], vik, dirs, z_vals, S,
                                                           legacy_mode=self.legacy_mode, input_scaler=scaler, noise=noise,
                                                           precision=engine, **integ)
            elif route == "fused":
                with stage(self, "render_fused"):
                    feats, depths, weights = nf.render(pts, freq, phase, geo, dirs, z_vals, S, input_scaler=scaler, noise=noise,
                                                       precision=engine, **integ)
            else:
                with stage(self, "neural_field"):
                    field = nf(pts, freq, phase, geo, dirs, input_scaler=scaler, differentiable=differentiable, precision=engine)
                with stage(self, "ray_integrate"):
                    feats, depths, weights = vr.ray_integration(field.reshape(B, R, S, -1), z_vals, noise_std=0, noise=noise,
                                                                consume_rng=False, **integ)
        rgb_render = (feats[..., :3] * 2 - 1).reshape(B, render_height, render_width, 3).permute(0, 3, 1, 2)
        return rgb_render, feats[..., 3:], depths, weights, None

    def _render_hierarchical(self, freq, phase, mesh, pts, z_vals, frame, Sf, engine, lock_view_dependence, scaler, integ, nerf_noise,
                             noise_coarse, fine_u, noise):
        """reference :449-516, behind _render's ray set-up: coarse pass -> compositing weights -> importance samples -> fine pass ->
        merge by depth -> integration over all samples -> (features, depths, weights).  The field tensors materialise here (unfused
        kernels); random tensors can be injected (noise_coarse [B,R,S,1], fine_u [B*R,Sf], noise [B,R,S+Sf,1]) or are drawn where
        the reference draws them."""
        (B, R, S), dev = z_vals.shape[:3], freq.device
        origins, ray_dirs = frame

        def field(points, n_steps):
            with stage(self, "geo_features"):
                geo = self.get_geo_features(points, *mesh)
            with stage(self, "neural_field"):
                dirs = None
                if not lock_view_dependence:
                    dirs = ray_dirs.unsqueeze(2).expand(B, R, n_steps, 3).reshape(B, R * n_steps, 3).contiguous()
                return self.neural_field(points, freq, phase, geo, dirs, input_scaler=scaler, differentiable=False,
                                         precision=engine).reshape(B, R, n_steps, -1)

        coarse = field(pts, S)
        noise_coarse = _integration_noise(noise_coarse, (B, R, S, 1), nerf_noise, dev)        # first ray_integration call
        with stage(self, "ray_integrate"):
            _, _, w = vr.ray_integration(coarse, z_vals, noise_std=0, noise=noise_coarse, clamp_mode=integ["clamp_mode"],
                                         consume_rng=False)
        with stage(self, "resample"):
            w = w.reshape(B * R, S) + 1e-5
            zv = z_vals.reshape(B * R, S)
            z_mid = 0.5 * (zv[:, :-1] + zv[:, 1:])
            fine_z = vr.sample_pdf(z_mid, w[:, 1:-1], Sf, det=False, u=fine_u).reshape(B, R, Sf, 1)
            fine_pts = vr.ray_points(origins, ray_dirs, fine_z)
        fine = field(fine_pts, Sf)
        with stage(self, "resample"):
            all_out, all_z = vr.merge_samples(fine, coarse, fine_z, z_vals)
        noise = _integration_noise(noise, (B, R, S + Sf, 1), nerf_noise, dev)                 # second call
        with stage(self, "ray_integrate"):
            return vr.ray_integration(all_out, all_z, noise_std=0, noise=noise, consume_rng=False, **integ)

    def _block0_inputs(self, latent, conditions, kwargs):
        """What block 0 reads besides the pixel coordinates (reference :256-265 / :344-352) -> (label map int64 [B, H, W] or None,
        latent [B, L] or None).  The flags are read from the call as in the reference and must be the ones the modules were built
        with (the reference's convolutions would fail on the channel count)."""
        for flag, built in (("2d_label_input", self.label_input), ("2d_latent_input", self.latent_input)):
            if bool(kwargs.get(flag, False)) != built:
                raise ValueError(f"{flag}={bool(kwargs.get(flag, False))} in the call, but the generator was built with {flag}={built}")
        seg = None
        if self.label_input:
            seg = conditions["rasterized_segments"]
            want = (latent.shape[0], self.gen_height, self.gen_width)
            if tuple(seg.shape) != want:
                raise ValueError(f"2d_label_input: rasterized_segments must be [batch, gen_height, gen_width] = {list(want)}, "
                                 f"got {list(seg.shape)}")
            seg = seg.long()
        return seg, (latent if self.latent_input else None)

    def _layerwise_synthesis(self):
        """Input variants the fused engines do not take run layer by layer (differentiable.synthesis_forward) in inference too."""
        return self.label_input or self.latent_input or self.feature_dim > self.hidden_dim

    def _synthesize(self, feature_maps, styles, render_hw, differentiable=False, block0=(None, None)):
        if differentiable or (self._layerwise_synthesis() and self.synthesis_network.normalization != "none"):
            if self.synthesis_network.normalization == "none":
                raise NotImplementedError("spatial_normalization='none' has no differentiable synthesis path")
            with stage(self, "synthesis"):
                if differentiable:
                    return synthesis_forward(self, feature_maps, styles, render_hw, (self.gen_height, self.gen_width),
                                             training=self.training, group=getattr(self, "process_group", None), block0=block0)
                with torch.no_grad():          # inference: running statistics, stored spectral-norm u / v, nothing recorded
                    return synthesis_forward(self, feature_maps, styles, render_hw, (self.gen_height, self.gen_width),
                                             training=False, block0=block0)
        plan = self.synthesis_plan(feature_maps.device)
        return plan.run(feature_maps, styles.reshape(styles.shape[0], -1), render_hw, (self.gen_height, self.gen_width),
                        owner=self)

    @staticmethod
    def _norender_checks(kwargs, differentiable):
        """What the disable_render=True path does not cover, refused before anything runs."""
        if differentiable:
            raise NotImplementedError("disable_render=True has the fused inference kernel only: the training / differentiable "
                                      "path is not implemented (call .eval() and leave differentiable unset)")
        mode = kwargs.get("feature_map_interpolation", "bilinear")
        if mode != "bilinear":
            raise NotImplementedError(f"disable_render=True: feature_map_interpolation={mode!r} has no HIP path (the synthesis "
                                      "engines resize bilinearly)")

    def _style_features(self, latent, conditions, kwargs):
        """reference :224-236 / :303-318: the style feature map straight from the rasterised body condition.
        -> feature_maps [B, Hc*Wc, F] (channels last, as render() returns them), (Hc, Wc)"""
        modal = kwargs["condition_modal_gen"]
        condition = conditions[modal]
        if "segments" in modal:
            condition = condition.unsqueeze(1).to(latent.dtype) / (kwargs["label_dim"] - 1) * 2 - 1
        plan = self.style_input_plan(latent.device)
        fmap = plan.run(condition, latent, latent_input=kwargs.get("spade_latent_input", True), owner=self)
        return fmap, tuple(condition.shape[2:])

    def wants_autograd(self, kwargs):
        """Which evaluation a forward call gets.  ``.train()`` mode -> the differentiable path with the reference's train-mode
        semantics (batch-statistics BatchNorm, spectral-norm power iteration), whether or not autograd is recording;
        ``.eval()`` mode -> the fused inference engines, never recorded.  ``differentiable=True / False`` overrides the
        choice (True in eval mode: gradients through the running-statistics network, e.g. latent optimisation)."""
        d = kwargs.get("differentiable")
        return self.training if d is None else bool(d)

    def forward(self, latent, conditions, render_height, render_width, latent_indices=None, **kwargs):
        """reference :208-280 -> {"rgbs", "rgbs_render"}"""
        if not latent.is_cuda:
            _lib.need_cuda(latent)
        diff = self.wants_autograd(kwargs)
        kwargs.pop("differentiable", None)
        with torch.cuda.device(latent.device):          # kernels launch on the current device's stream
            if diff:
                return self._forward(latent, conditions, render_height, render_width, latent_indices, differentiable=True,
                                     **kwargs)
            with torch.no_grad():
                return self._forward(latent, conditions, render_height, render_width, latent_indices, **kwargs)

    def _forward(self, latent, conditions, render_height, render_width, latent_indices=None, differentiable=False, **kwargs):
        if kwargs.get("disable_render", False):
            self._norender_checks(kwargs, differentiable)
            if latent_indices is not None:
                latent = self.latent_pool(latent_indices)
            rgb_render = torch.zeros([latent.shape[0], 3, render_height, render_width], dtype=latent.dtype, device=latent.device)
            if kwargs.get("disable_synthesis", False):
                return {"rgbs": rgb_render, "rgbs_render": rgb_render}
            with stage(self, "mapping"):
                _, styles = self.synthesis_mapping_network(latent)
            block0 = self._block0_inputs(latent, conditions, kwargs)
            fmap, cond_hw = self._style_features(latent, conditions, kwargs)
            return {"rgbs": self._synthesize(fmap, styles, cond_hw, block0=block0), "rgbs_render": rgb_render}
        if differentiable and self.synthesis_network.normalization == "none":
            raise NotImplementedError("spatial_normalization='none' has the fused inference engine only: the training / "
                                      "differentiable path is not implemented (call .eval() and leave differentiable unset)")
        num_steps = kwargs.get("num_steps", 24)
        if latent_indices is not None:
            latent = self.latent_pool(latent_indices)
        fr, ph, styles = self._mapping(latent, kwargs)
        rk = {k: v for k, v in kwargs.items() if k not in ("coarse_steps", "fine_steps", "render_width", "render_height")}
        rgb_render, fmap, _, _, _ = self.render(fr, ph, conditions, render_width, render_height,
                                                coarse_steps=num_steps, fine_steps=num_steps, differentiable=differentiable,
                                                **rk)
        if kwargs.get("disable_synthesis", False):
            return {"rgbs": rgb_render, "rgbs_render": rgb_render}
        rgb = self._synthesize(fmap, styles, (render_height, render_width), differentiable,
                               block0=self._block0_inputs(latent, conditions, kwargs))
        return {"rgbs": rgb, "rgbs_render": rgb_render}

    @torch.no_grad()
    def staged_forward(self, latent, conditions, render_height, render_width, truncation_psi, **kwargs):
        """reference :282-378 -> {"rgbs", "rgbs_render", "depths" (CPU, as the reference), "skeletons"}.
        ``avg_latent=`` kwarg (or a cached self.avg_latent with cache_avg_latent=True) skips the 10 000-sample pass."""
        if not latent.is_cuda:
            _lib.need_cuda(latent)
        with torch.cuda.device(latent.device):
            return self._staged_forward(latent, conditions, render_height, render_width, truncation_psi, **kwargs)

    def _truncated_mapping(self, latent, truncation_psi, kwargs):
        """reference :289-301: the mapping networks, then the truncation trick towards the mean of 10 000 latents (``avg_latent=`` in
        kwargs, or the cached one with cache_avg_latent=True, else drawn here) -> (latent, frequencies, phases, styles)."""
        fr, ph, styles = self._mapping(latent, kwargs)
        if truncation_psi < 1.0:
            avg = kwargs.get("avg_latent")
            if avg is None:
                avg = self.cached_avg_latent() if kwargs.get("cache_avg_latent", False) else None
                if avg is None:
                    avg = self.generate_avg_latent()
            az, af, ap, ast = avg
            fr = af + truncation_psi * (fr - af)
            ph = ap + truncation_psi * (ph - ap)
            latent = az + truncation_psi * (latent - az)
            styles = ast + truncation_psi * (styles - ast)
        return latent, fr, ph, styles

    def _staged_forward(self, latent, conditions, render_height, render_width, truncation_psi, **kwargs):
        no_render = kwargs.get("disable_render", False)
        if no_render:
            self._norender_checks(kwargs, False)
        num_steps = kwargs.get("num_steps", 24)
        B = latent.shape[0]
        latent, fr, ph, styles = self._truncated_mapping(latent, truncation_psi, kwargs)
        rk = {k: v for k, v in kwargs.items() if k not in ("coarse_steps", "fine_steps", "render_width", "render_height",
                                                           "staged", "avg_latent", "cache_avg_latent")}
        feature_hw = (render_height, render_width)
        if no_render:
            # reference :303-316: the (truncated) latent feeds the style input; the render image and the depths are zeros
            rgb_render = torch.zeros([B, 3, render_height, render_width], dtype=latent.dtype, device=latent.device)
            depths = torch.zeros([B, render_height * render_width, 1], dtype=latent.dtype, device=latent.device)
            if not kwargs.get("disable_synthesis", False):
                fmap, feature_hw = self._style_features(latent, conditions, kwargs)
        else:
            rgb_render, fmap, depths, _, _ = self.render(fr, ph, conditions, render_width, render_height,
                                                         coarse_steps=num_steps, fine_steps=num_steps, staged=True, **rk)
        if kwargs.get("disable_synthesis", False):
            from ..components.resample import bilinear_resize
            out = {"rgbs": bilinear_resize(rgb_render.contiguous(), (self.gen_height, self.gen_width)),
                   "rgbs_render": rgb_render}
        else:
            # reference :300, :349-352: the TRUNCATED latent is the one block 0 reads
            out = {"rgbs": self._synthesize(fmap, styles, feature_hw, block0=self._block0_inputs(latent, conditions, kwargs)),
                   "rgbs_render": rgb_render}
        zc = conditions["intrinsics"][:, 0, 0] / conditions["scales"].float()
        depth = ((depths - zc.view(B, 1, 1)) / (kwargs["depth_length"] / 2.0)).clamp(-1.0, 1.0)
        depth_map = depth.reshape(B, render_height, render_width).unsqueeze(1).contiguous()
        out.update({"depths": depth_map if kwargs.get("keep_depth_on_device", False) else depth_map.cpu(),
                    "skeletons": conditions["skeletons_xyz"]})
        return out

    # ------------------------------------------------------------------ geometry export
    MESH_CONDITIONS = ("skeletons_xyz", "vertices", "tpose_vertices", "fk_matrices", "lbs_weights")

    @torch.no_grad()
    def density_grid(self, latent, conditions, resolution=256, margin=0.1, truncation_psi=1.0, max_points=2 ** 21, precision=None,
                     **config):
        """The density of the field on a regular grid around each body -> (sigma fp32 [B,Nx,Ny,Nz], origin [B,3], spacing [B,3]);
        node (i, j, k) of item b lies at origin[b] + spacing[b] * (i, j, k), in the world frame of conditions["vertices"].

        Mapping and truncation are staged_forward's own (avg_latent= / cache_avg_latent= honoured), so the grid belongs to the image
        the same latent gives.  Per item the axis-aligned box of the SMPL vertices is grown on every side by `margin` x its longest
        edge; the voxels are cubic, `resolution` nodes span the longest axis of the grown box and the other axes take as many nodes
        as cover it at that spacing; all items share (Nx, Ny, Nz), the largest count over the batch per axis.  The field runs on
        chunks of at most `max_points` points (over the batch) through get_geo_features and the engine `precision` (None: the
        field's own) and only its density channel is kept: the [N, F+4] tensor never exists for the grid.  The density head does
        not read the view direction.  Of `conditions` only MESH_CONDITIONS are read -- no camera."""
        if not latent.is_cuda:
            _lib.need_cuda(latent)
        if int(resolution) < 2:
            raise ValueError(f"density_grid: resolution={resolution} (nodes along the longest axis) must be at least 2")
        with torch.cuda.device(latent.device):
            _, fr, ph, _ = self._truncated_mapping(latent, truncation_psi, config)
            mesh = tuple(conditions[k] for k in self.MESH_CONDITIONS)
            verts = conditions["vertices"].float()
            B, dev = verts.shape[0], verts.device
            # the grid's frame, on the host in float64 (the node counts are shapes: one read of 6 B numbers)
            lo, hi = (t.double().cpu().numpy() for t in (verts.amin(dim=1), verts.amax(dim=1)))
            grow = margin * (hi - lo).max(axis=1, keepdims=True)
            lo, extent = lo - grow, (hi - lo) + 2 * grow
            step = extent.max(axis=1) / (int(resolution) - 1)                                  # [B]
            counts = np.ceil(extent / step[:, None] - 1e-6).astype(np.int64) + 1               # nodes that cover the box
            Nx, Ny, Nz = (max(2, int(n)) for n in counts.max(axis=0))
            origin = torch.as_tensor(lo, dtype=torch.float32).to(dev)
            spacing = torch.as_tensor(np.repeat(step[:, None], 3, axis=1), dtype=torch.float32).to(dev)
            N = Nx * Ny * Nz
            sigma = torch.empty(B, N, dtype=torch.float32, device=dev)
            chunk = max(1, int(max_points) // B)
            scaler = 2.0 / self.side_length
            for start in range(0, N, chunk):
                n = torch.arange(start, min(start + chunk, N), device=dev)
                ijk = torch.stack([n // (Ny * Nz), (n // Nz) % Ny, n % Nz], dim=-1).float()    # node id = (ix Ny + iy) Nz + iz
                pts = (origin[:, None] + spacing[:, None] * ijk[None]).contiguous()
                geo = self.get_geo_features(pts, *mesh)
                out = self.neural_field(pts, fr, ph, geo, None, input_scaler=scaler, differentiable=False, precision=precision)
                sigma[:, start:start + n.shape[0]] = out[..., -1]
            return sigma.reshape(B, Nx, Ny, Nz), origin, spacing

    @torch.no_grad()
    def extract_mesh(self, latent, conditions, level=None, simplify=None, **config):
        """The iso-surface of density_grid(latent, conditions, **config) at `level` as one (vertices fp32 [V,3], faces int32 [T,3])
        per item, in the world frame of conditions["vertices"], normals pointing out of the body (marching tetrahedra on the
        device, lib/components/isosurface.py).  level=None: ln 2 * num_steps / (ray_end - ray_start), the density at which one
        coarse integration step of the render is half opaque (1 - exp(-sigma * delta) = 1/2).
        simplify=K (a positive number, None: off): the surface is reduced by quadric vertex clustering (lib/components/
        mesh_simplify.py) on cells of K voxels of the density grid, laid over the grid's own box: 12 / 27 / 49 times fewer triangles
        at K = 2 / 3 / 4 on a sphere, with the shape the fine grid saw."""
        s = geometry_export.settings("extract_mesh", config, level=level, simplify=simplify)
        sigma, origin, spacing = self.density_grid(latent, conditions, **config)
        with torch.cuda.device(sigma.device):
            return [(m["vertices"], m["faces"]) for m in geometry_export.surfaces(sigma, origin, spacing, s.level, s.simplify, False)]

    @torch.no_grad()
    def extract_textured_mesh(self, latent, conditions, views, level=None, depth_tolerance=None, normal_power=2, texture_size=None,
                              simplify=None, **config):
        """extract_mesh with per-vertex attributes -> one dict(vertices, faces, normals, colors, coverage) per item.

        vertices and faces are extract_mesh's; normals are vertex_normals of the same density grid (one density_grid call serves
        both).  The colour does not live in the field -- the synthesis network makes the appearance -- so it is carried over from
        images: for every entry of `views` (a conditions dict batched like `conditions`, what CameraPreprocessor.forward_with_rotation
        returns) staged_forward(latent, view, keep_depth_on_device=True, **config) runs, in list order, and nothing else here draws
        random numbers: the same seed in front of this call gives the frames the app gives.  Each view's depth map is taken back to
        the distance along the ray (depth_map * depth_length / 2 + focal / scale) and project_colors (lib/components/mesh_color.py)
        weighs the views at every vertex: colors fp32 [V,3] in the images' [-1, 1], coverage fp32 [V] = how much the vertex was seen
        (a vertex no view sees has coverage 0 and colour 0).  views=[] gives colors = coverage = None.
        depth_tolerance=None: 2 * (ray_end - ray_start) / num_steps, two coarse steps of the render -- the resolution to which its
        expected depth and the iso-surface can agree.
        texture_size=S (needs at least one view): every dict gains uvs fp32 [T,3,2] (per face corner, v = 0 at the top row), texture
        fp32 [S,S,3] and texture_coverage fp32 [S,S] -- the same frames baked into a texture atlas (lib/components/mesh_texture.py),
        so the appearance has the resolution of the texture, not of the density grid.  Nothing else is rendered or drawn for it, and
        colors / coverage are what they are without it.
        simplify=K: as in extract_mesh; the normals, colours and texture are evaluated at the simplified mesh's own vertices and
        faces (nothing is carried across), so every triangle's cell of the atlas grows with the reduction."""
        views = list(views)
        s = geometry_export.settings("extract_textured_mesh", config, len(views), level, depth_tolerance, normal_power, texture_size, simplify)
        return self._textured_meshes(latent, conditions, views, s, config)

    def _textured_meshes(self, latent, conditions, views, s, config):
        """behind the settings `s`: the geometry of every item, then the frames in the order of `views`, then the colours"""
        sigma, origin, spacing = self.density_grid(latent, conditions, **config)
        with torch.cuda.device(sigma.device):
            meshes = geometry_export.surfaces(sigma, origin, spacing, s.level, s.simplify, True)
            if not views:
                return meshes
            frames = [geometry_export.view_frame(self, latent, view, config) for view in views]
            return geometry_export.colour(meshes, views, frames, s.depth_tolerance, s.normal_power, s.texture_size)

    @torch.no_grad()
    def extract_avatar(self, latent, conditions, k=4, level=None, views=(), texture_size=None, simplify=None, **config):
        """extract_textured_mesh made re-posable -> its list of dicts, each with the rig entries of mesh_rig.bind added:
        rest_vertices, rest_normals, joints int32 [V,4], weights [V,4], det [V].

        The generator's own notion of space is "nearest SMPL vertex, then undo that vertex's blended bone transform"
        (get_geo_features), so the body of `conditions` is the rig: every mesh vertex takes the skin weights of its `k` nearest posed
        SMPL vertices (conditions["vertices"], ["lbs_weights"]: [B,V,J] or [V,J]), cut to four joints, and goes to the rest pose by
        the inverse of its blend of conditions["fk_matrices"].  mesh_rig.pose(rest_vertices, joints, weights, fk) puts it into any
        other pose of the skeleton; with this item's fk_matrices it gives back `vertices`.  `views`, `level` and the config: as in
        extract_textured_mesh (views=() gives no colours).  texture_size: as there; the UVs belong to the faces, so the texture baked
        in the posed space serves the rest mesh unchanged.  simplify=K: as there; the simplified vertices are the ones bound."""
        views = list(views)
        s = geometry_export.settings("extract_avatar", config, len(views), level, texture_size=texture_size, simplify=simplify)
        meshes = self._textured_meshes(latent, conditions, views, s, config)
        with torch.cuda.device(latent.device):
            return geometry_export.rig(meshes, conditions, k)

    default_depth_tolerance = staticmethod(geometry_export.default_depth_tolerance)
