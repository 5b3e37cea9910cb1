"""One statement of the field engines' arithmetic on the CPU, and the accuracy bars derived from it ("accuracy
ladder").  No GPU, no kernel: float64 everywhere except the six hidden contractions (FiLM 0-3, the hidden part of the colour
layer, the feature head), which go through an `mm` hook -- exact, three-product f16 ("x3"), f16 + block-scaled fp6 ("x2",
tests/x2_emulation.py), a single f16 product, or one of those with ONE term missing in ONE contraction:

    D1  x3 without hi(W).lo(x)          D2  x3 without lo(W).hi(x)          D3  x2 without its fp6 cross-term product

The bars (ladder_of) come from these emulations and the float64 oracle alone:
    x3 class (f32, f16x3, f16x3t), against float64:  min over the single-defect variants D1, D2 that touch the group / 3
    x2 class (f16x2, f16x2t),      against float64:  3 x the healthy x2 emulation's error
                                   against the x2 emulation's output:  min over D3 of its distance to the healthy emulation / 3
A defect counts for a group only if its contraction touches the group (TOUCHED_BY).  tests/test_field_ladder_cpu.py
checks that each case separates (every defect >= 3 x its bar by construction, the healthy reference arithmetic >= 3 x under it);
tests/test_gpu_field_ladder.py holds the kernels to the bars."""
import importlib
from typing import NamedTuple

import numpy as np
import torch

import h3d_oracle as O
from conftest import rel_err, rel_err_channels
from x2_emulation import f16, q_e2m3, slot_groups, weight_alpha, x2_matmul, x3_matmul

N_CONTRACTIONS = 6            # FiLM 0-3, the hidden part of the colour layer, the feature head
HEAD = 5
MARGIN = 3.0
X3_CLASS, X2_CLASS = ("f32", "f16x3", "f16x3t"), ("f16x2", "f16x2t")


def engine_class(engine):
    return "x2" if engine in X2_CLASS else "x3"


# ---- contractions: x [..., K], W [N, K] -> x @ W.T

def exact_matmul(x, W):
    return x.double() @ W.double().t()


def _matrix_scale(W, w_target=8192.0):
    mx = float(W.abs().max())
    return 2.0 ** np.floor(np.log2(w_target / mx)) if mx > 0 else 1.0


def f16_matmul(x, W):
    """A single f16 product (the f16x1 tier): hi(W).hi(x)."""
    x, W = x.double(), W.double()
    sc = _matrix_scale(W)
    return f16(x) @ f16(W * sc).t() / sc


def x3_terms(x, W, hi_lo=True, lo_hi=True):
    """x3_matmul with its cross terms optional: hi_lo = hi(W).lo(x), lo_hi = lo(W).hi(x)."""
    x, W = x.double(), W.double()
    sc = _matrix_scale(W)
    Ws = W * sc
    Wh = f16(Ws)
    Wl = f16(Ws - Wh)
    xh = f16(x)
    xl = f16(x - xh)
    y = xh @ Wh.t()
    if hi_lo:
        y = y + xl @ Wh.t()
    if lo_hi:
        y = y + xh @ Wl.t()
    return y / sc


def x2_terms(x, W, fp6=True, acc=torch.float64, per_ray_head=False, x_scale_hi=4.0, rho=4096.0):
    """x2_matmul with its fp6 product optional and the accumulation type selectable (fp32: the matrix cores' own).
    per_ray_head: the operand split of the fused render's per-ray feature head (csrc/field_x3.hip, RAYHEAD flush) -- hi(W).lo(x)
    is a full f16 product there and the fp6 instruction carries lo(W).hi(x) alone."""
    x, W = x.double(), W.double()
    K = W.shape[1]
    sc = _matrix_scale(W)
    Ws = W * sc
    Wh = f16(Ws)
    Wl = Ws - Wh
    xh = f16(x)
    xl = x - xh
    y = xh.to(acc) @ Wh.to(acc).t()
    if per_ray_head:
        y = y + f16(xl).to(acc) @ Wh.to(acc).t()
    if fp6:
        Bh = q_e2m3(xh * x_scale_hi)
        Bl = torch.zeros_like(Bh) if per_ray_head else q_e2m3(f16(xl * rho) * x_scale_hi)
        for g in slot_groups(K):
            alpha = weight_alpha(Wh[:, g], Wl[:, g], rho)
            Ah = q_e2m3(Wh[:, g] * alpha[:, None])
            Al = q_e2m3(Wl[:, g] * rho * alpha[:, None])
            cross = Bl[..., g].to(acc) @ Ah.to(acc).t() + Bh[..., g].to(acc) @ Al.to(acc).t()     # exact fp6 products, accumulated
            y = y + cross * (1.0 / (alpha * x_scale_hi * rho)).to(acc)                             # power-of-two block scale
    return y.double() / sc


def single_defect(healthy, broken, layer):
    """-> the mm table of _field: `broken` in contraction `layer`, `healthy` in the five others."""
    return [broken if l == layer else healthy for l in range(N_CONTRACTIONS)]


def d1(x, W):
    return x3_terms(x, W, hi_lo=False)


def d2(x, W):
    return x3_terms(x, W, lo_hi=False)


def d3(x, W):
    return x2_terms(x, W, fp6=False)


# ---- the field

def _field(state, points, freq, phase, geo, dirs, input_scaler, mm, head=True):
    """lib/implicit_funcitions/modulated.py:41-75 with the hidden-layer contractions routed through `mm` (float64 elsewhere).
    mm: one contraction for all six, or a table of six (single_defect).  FiLM 0 is contracted as the engines do it: the coordinate
    half and the geometry half of its input are two operands of their own (each padded to whole K-tiles, so the fp6 slot groups
    never straddle the halves).  head=False: -> (rgb, colour activations, sigma) without the feature head (field_render)."""
    p = "neural_field."
    st = {k: v.double() for k, v in state.items()}
    hd = st[p + "sigma_layer.weight"].shape[1]
    mms = list(mm) if isinstance(mm, (list, tuple)) else [mm] * N_CONTRACTIONS

    def lin(name, x):
        return x @ st[p + name + ".weight"].t() + st[p + name + ".bias"]

    f = (freq.double() * 15 + 30).unsqueeze(1)
    ph = phase.double().unsqueeze(1)
    a = torch.sin(30.0 * lin("first_layer_coord.layer", points.double() * input_scaler))
    g = torch.sin(30.0 * lin("first_layer_mod.layer", geo.double()))
    W0, b0 = st[p + "network.0.layer.weight"], st[p + "network.0.layer.bias"]
    x = torch.sin(f[..., :hd] * (mms[0](a, W0[:, :hd]) + mms[0](g, W0[:, hd:]) + b0) + ph[..., :hd])
    for k in range(1, 4):
        sl = slice(k * hd, (k + 1) * hd)
        y = mms[k](x, st[p + f"network.{k}.layer.weight"]) + st[p + f"network.{k}.layer.bias"]
        x = torch.sin(f[..., sl] * y + ph[..., sl])
    sigma = lin("sigma_layer", x)
    Wc, bc = st[p + "color_layer_sine.layer.weight"], st[p + "color_layer_sine.layer.bias"]
    c = mms[4](x, Wc[:, 3:]) + dirs.double() @ Wc[:, :3].t() + bc
    c = torch.sin(f[..., -hd:] * c + ph[..., -hd:])
    rgb = torch.sigmoid(lin("color_layer_linear", c))
    if not head:
        return rgb, c, sigma
    feat = mms[HEAD](c, st[p + "feature_layer_linear.weight"]) + st[p + "feature_layer_linear.bias"]
    return torch.cat([rgb, feat, sigma], dim=-1)


def field_render(state, points, freq, phase, geo, dirs, input_scaler, mm, z, noise, S, clamp, last_back, white_back,
                 per_ray_head=False, head_mm=None):
    """_field, then O.ray_integration in float64 -> (features [B,R,F+3], depth [B,R,1], weights [B,R,S,1]).
    per_ray_head: the feature head applied once per ray to the composited colour activations, as the RAYHEAD kernels do:
    head(sum_s w_s c_s) + b_f sum_s w_s (+ the white background), the head contraction through head_mm (default: mm's sixth)."""
    B, R = z.shape[:2]
    zd, nd = z.double(), None if noise is None else noise.double()
    if not per_ray_head:
        out = _field(state, points, freq, phase, geo, dirs, input_scaler, mm)
        return O.ray_integration(out.reshape(B, R, S, -1), zd, nd, clamp, last_back, white_back)
    mms = list(mm) if isinstance(mm, (list, tuple)) else [mm] * N_CONTRACTIONS
    rgb, c, sigma = _field(state, points, freq, phase, geo, dirs, input_scaler, mms, head=False)
    parts = torch.cat([rgb, c, sigma], dim=-1).reshape(B, R, S, -1)
    comp, depth, w = O.ray_integration(parts, zd, nd, clamp, last_back, False)
    Wf = state["neural_field.feature_layer_linear.weight"].double()
    bf = state["neural_field.feature_layer_linear.bias"].double()
    feat = (head_mm or mms[HEAD])(comp[..., 3:], Wf) + bf * w.sum(2)
    feats = torch.cat([comp[..., :3], feat], dim=-1)
    if white_back:
        feats = feats + 1 - O.ray_integration(parts, zd, nd, clamp, False, False)[2].sum(2)
    return feats, depth, w


# ---- error metrics, one number per output group

FIELD_GROUPS = ("rgb", "feat", "feat_ch", "sigma")
RENDER_GROUPS = ("rgb", "feats", "feats_ch", "weights", "depth")
# The contractions that touch a group: the density leaves the chain after FiLM 3 (contractions 0-3: sigma, and the weights and
# depth composited from it), the colours after the colour layer (0-4), only the features see the feature head (0-5).
TOUCHED_BY = {"sigma": 4, "weights": 4, "depth": 4, "rgb": 5}


def field_errors(out, ref, feature):
    """out, ref [B, N, F + 4] -> max-norm relative error of the colours, the features (whole tensor and worst channel), the density."""
    out, ref = out.detach().cpu().double(), ref.double()
    f = slice(3, 3 + feature)
    return {"rgb": rel_err(out[..., :3], ref[..., :3]), "feat": rel_err(out[..., f], ref[..., f]),
            "feat_ch": rel_err_channels(out[..., f], ref[..., f], dim=2), "sigma": rel_err(out[..., -1:], ref[..., -1:])}


def render_errors(got, ref, z_span, white=False):
    """got, ref = (features [B,R,F+3], depth, weights); the depth error is normalised by the case's z-span (max z - min z), not by
    |depth|: the depths sit at |z| ~ 11 with a span of ~1, and a relative error would hide the compositing error 11-fold.
    white: a render with white_back and without last_back -- every colour and feature channel carries the background term
    1 - sum(w), which each side's own weights give back exactly.  It is taken off both sides first: with it every channel has the
    same O(1) term, so the per-channel metric collapses onto the whole-tensor one, and the term's own error (the weights', which
    have their group) drowns what the colour layer and the head contribute.  A kernel that composes the term wrongly still shows:
    what is taken off is the term its weights imply, not what it added."""
    (gf, gd, gw), (rf, rd, rw) = ([t.detach().cpu().double() for t in got], [t.double() for t in ref])
    if white:
        gf, rf = gf - (1 - gw.sum(2)), rf - (1 - rw.sum(2))
    return {"rgb": rel_err(gf[..., :3], rf[..., :3]), "feats": rel_err(gf[..., 3:], rf[..., 3:]),
            "feats_ch": rel_err_channels(gf[..., 3:], rf[..., 3:], dim=2), "weights": rel_err(gw, rw),
            "depth": float((gd - rd).abs().max() / z_span)}


# ---- cases

class Case(NamedTuple):
    name: str
    kind: str                  # "field" | "render" | "render_geo"
    hidden: int
    feature: int
    seed: int                  # of the weights (random_state of tests/test_gpu_field.py)
    gseed: int                 # of the inputs
    N: int = 0                 # field: samples per item
    S: int = 0                 # render: samples per ray
    R: int = 0                 # render: rays per item
    dirs: bool = False         # field: explicit view directions (False: None = the locked direction (0, 0, -1))
    mode: tuple = ()           # render: (clamp, last_back, white_back)
    engines: tuple = ()
    refine: bool = False       # render_geo: the x2 render's last-sample refinement on (the shipped default)
    no_dist: tuple = ()        # groups whose x2 distance bar does not separate on the CPU: measured and recorded, not asserted

    @property
    def per_ray_head(self):
        """The calls the register engines' fused render takes with the head once per ray (csrc/field_x3.hip: RAYHEAD)."""
        return self.kind != "field" and self.S >= 32 and self.feature == self.hidden

    @property
    def input_key(self):
        """Cases with the same key share weights, inputs and every field evaluation."""
        return (self.kind != "field", self.kind == "render_geo", self.hidden, self.feature, self.seed, self.gseed, self.N, self.S, self.R,
                self.dirs)


B = 2
REGISTER, WIDE = ("f32", "f16x3", "f16x2"), ("f32", "f16x3t", "f16x2t")
MODES = (("relu", False, True), ("softplus", True, False))


def _cases():
    out = []
    # unfused field: N = 77 is ragged against the 32-sample wave unit; NT = 4, padded channels, NT = 8, the wide engines,
    # feature_dim != hidden_dim; with the locked direction and with explicit ones
    for hidden, feature, engines in ((64, 64, REGISTER), (200, 200, REGISTER), (256, 256, REGISTER), (384, 384, WIDE),
                                     (420, 420, WIDE), (128, 96, REGISTER)):
        for dirs in (False, True):
            out.append(Case(f"field-h{hidden}-f{feature}-{'dirs' if dirs else 'locked'}", "field", hidden, feature, seed=hidden, gseed=77,
                            N=77, dirs=dirs, engines=engines))
    # fused render: per-sample head with two rays per wave step (S = 16), the per-ray head with a carry across tiles (S = 64, 128),
    # a narrow head that stays per sample
    for S, R, hidden, feature, seed, gseed, no_dist_relu in RENDER_SHAPES:
        for mode in MODES:
            tag = f"render-S{S}-R{R}-h{hidden}-f{feature}-{mode[0]}"
            out.append(Case(tag, "render", hidden, feature, seed=seed, gseed=gseed, S=S, R=R, mode=mode, engines=REGISTER,
                            no_dist=no_dist_relu if mode[0] == "relu" else ()))
    # in-kernel geometry features (geo_setup of tests/test_gpu_ray_head.py): one case per engine of field_x3.hip, and the x2 render
    # with its last-sample refinement on.  NOT coverage of the refinement itself: every ray is conditioned 10 x outside the 1e-3
    # listing band, so no unit is listed and the x3 relaunch redoes nothing (its tests: tests/test_gpu_refine.py); the case shows
    # that the shipped default path, list launch included, meets the x2 bars.
    out.append(Case("geo-S64-R7-h64", "render_geo", 64, 64, seed=128, gseed=7, S=64, R=7, mode=("relu", True, False),
                    engines=("f16x3", "f16x2")))
    out.append(Case("geo-S64-R7-h64-refined", "render_geo", 64, 64, seed=128, gseed=7, S=64, R=7, mode=("relu", True, False),
                    engines=("f16x2",), refine=True))
    return out


# (S, R, hidden, feature, weight seed, input seed, groups without an x2 distance assertion in the relu / white-background mode):
# weight seed S + hidden as tests/test_gpu_field.py::test_fused_render_vs_oracle; input seeds chosen on the CPU so that every ray
# is well conditioned and the case separates (tests/test_field_ladder_cpu.py).  Every shape runs in both modes with every bar but
# one: in the (relu, white background) mode of three shapes the x2 DISTANCE of the colours does not separate.  A dead fp6 product
# in the colour layer alone (D3@4) moves the composited colours by ~5e-6 through the 3-row sigmoid head, the healthy emulation's
# own fp32-accumulation noise in the weights moves them by 1-4e-6 (under 9 x apart for 30 input seeds of each shape, background
# term removed or not).  That one assertion is left out there, the figure is still measured and recorded; the colours keep their
# x3 and x2-vs-float64 bars, and the layers a dead colour-layer product would hide behind keep the distance bars of the features.
RENDER_SHAPES = ((16, 30, 48, 48, 64, 31, ("rgb",)), (64, 40, 64, 64, 128, 40, ("rgb",)), (64, 5, 256, 256, 320, 5, ("rgb",)),
                 (128, 3, 64, 64, 192, 3, ()), (64, 5, 64, 32, 128, 7, ()))
CASES = _cases()
CASE = {c.name: c for c in CASES}


def make_state(hidden, feature, seed, sigma_gain=1.0):
    """random_state of tests/test_gpu_field.py on the CPU: -> (state dict, module).  Seeded fp32 initialisation, never float16."""
    impl = importlib.import_module("3dhumangan_amd.lib.implicit_funcitions")
    torch.manual_seed(seed)
    net = impl.COORDCONCATSIREN(input_dim=3, latent_dim=hidden, hidden_dim=hidden, geo_feature_dim=31, output_dim=feature + 4,
                                feature_dim=feature, num_blocks=4)
    with torch.no_grad():
        for p in net.parameters():
            if p.ndim == 1:
                p.add_(0.05 * torch.randn_like(p))
        net.sigma_layer.weight.mul_(sigma_gain)          # renders: make the densities matter
    return {"neural_field." + k: v.detach().clone() for k, v in net.state_dict().items()}, net


_INPUTS, _OUTPUTS, _LADDER = {}, {}, {}


def inputs_of(case):
    """-> dict of the case's CPU inputs (shared, never modified): state, net, pts, geo, dirs (tensor), freq, phase, scaler and, for
    renders, z, noise, z_span (and cond for render_geo)."""
    key = case.input_key
    if key in _INPUTS:
        return _INPUTS[key]
    hidden = case.hidden
    g = torch.Generator().manual_seed(case.gseed)
    if case.kind == "field":
        state, net = make_state(hidden, case.feature, case.seed)
        N = case.N
        pts = torch.rand(B, N, 3, generator=g) * 2 - 1
        geo = torch.rand(B, N, 31, generator=g) * 2 - 1
        dirs = torch.nn.functional.normalize(torch.randn(B, N, 3, generator=g), dim=-1)
        freq = torch.randn(B, 4 * hidden, generator=g) * 0.5
        phase = torch.randn(B, 4 * hidden, generator=g)
        if not case.dirs:
            dirs = torch.zeros(B, N, 3)
            dirs[..., 2] = -1
        inp = dict(state=state, net=net, pts=pts, geo=geo, dirs=dirs, freq=freq, phase=phase, scaler=2.0 / 2.85)
    else:
        state, net = make_state(hidden, case.feature, case.seed, sigma_gain=40.0)
        S, R = case.S, case.R
        N = R * S
        cond = None
        if case.kind == "render_geo":
            synthetic = importlib.import_module("3dhumangan_amd.synthetic")
            cond = synthetic.make_conditions(B, n_vertices=500, seed=R)
        pts = torch.rand(B, N, 3, generator=g) * 2 - 1
        if cond is None:
            geo = torch.rand(B, N, 31, generator=g) * 2 - 1
        else:
            geo = O.geo_features(pts, cond["skeletons_xyz"], cond["vertices"], cond["tpose_vertices"], cond["fk_matrices"],
                                 cond["lbs_weights"], False)
        freq = torch.randn(B, 4 * hidden, generator=g) * 0.5
        phase = torch.randn(B, 4 * hidden, generator=g)
        z = torch.sort(torch.rand(B, R, S, 1, generator=g) + 11, dim=2).values
        noise = torch.randn(B, R, S, 1, generator=g) * 0.3
        dirs = torch.zeros(B, N, 3)
        dirs[..., 2] = -1
        inp = dict(state=state, net=net, pts=pts, geo=geo, dirs=dirs, freq=freq, phase=phase, scaler=0.7, z=z, noise=noise,
                   z_span=float(z.max() - z.min()), cond=cond)
    _INPUTS[key] = inp
    return inp


def hidden_matrices(state):
    """The weight operands of the six hidden contractions."""
    p = "neural_field."
    return {**{f"network.{k}": state[p + f"network.{k}.layer.weight"] for k in range(4)},
            "color": state[p + "color_layer_sine.layer.weight"][:, 3:], "feat": state[p + "feature_layer_linear.weight"]}


def variants(per_ray_head=False):
    """name -> (mm table, head contraction of the per-ray head or None).  The reference arithmetics and every single defect."""
    x2_f32 = lambda x, W: x2_terms(x, W, acc=torch.float32)
    v = {"exact": (exact_matmul, None), "x3": (x3_matmul, None), "x2": (x2_matmul, None), "x2_f32acc": (x2_f32, None),
         "f16x1": (f16_matmul, None)}
    if per_ray_head:
        v["x2"] = (x2_matmul, lambda x, W: x2_terms(x, W, per_ray_head=True))
        v["x2_f32acc"] = (x2_f32, lambda x, W: x2_terms(x, W, acc=torch.float32, per_ray_head=True))
    for l in range(N_CONTRACTIONS):
        v[f"D1@{l}"] = (single_defect(x3_matmul, d1, l), None)
        v[f"D2@{l}"] = (single_defect(x3_matmul, d2, l), None)
        v[f"D3@{l}"] = (single_defect(x2_matmul, d3, l), v["x2"][1])
    if per_ray_head:
        v[f"D3@{HEAD}"] = (single_defect(x2_matmul, d3, HEAD), lambda x, W: x2_terms(x, W, fp6=False, per_ray_head=True))
    return v


def _evaluate(case, name, mm, head_mm=None):
    i = inputs_of(case)
    args = (i["state"], i["pts"], i["freq"], i["phase"], i["geo"], i["dirs"], i["scaler"])
    if case.kind == "field":
        return _field(*args, mm=mm)
    clamp, last_back, white_back = case.mode
    return field_render(*args, mm, i["z"], i["noise"], case.S, clamp, last_back, white_back,
                        per_ray_head=case.per_ray_head and name != "exact", head_mm=head_mm)


def fp32_oracle(case):
    """The oracle in float32 throughout: the healthy reference arithmetic of the x3 class."""
    i = inputs_of(case)
    sd = {k: v.float() for k, v in i["state"].items()}
    out = O.neural_field(sd, i["pts"], i["freq"], i["phase"], i["geo"].float(), i["dirs"], i["scaler"])
    if case.kind == "field":
        return out
    clamp, last_back, white_back = case.mode
    return O.ray_integration(out.reshape(B, case.R, case.S, -1), i["z"], i["noise"], clamp, last_back, white_back)


def outputs_of(case):
    """name -> output of every variant (and "fp32") of the case, computed once."""
    if case.name not in _OUTPUTS:
        res = {n: _evaluate(case, n, mm, head_mm) for n, (mm, head_mm) in variants(case.per_ray_head).items()}
        res["fp32"] = fp32_oracle(case)
        _OUTPUTS[case.name] = res
    return _OUTPUTS[case.name]


def errors(case, got, ref):
    if case.kind == "field":
        return field_errors(got, ref, case.feature)
    _, last_back, white_back = case.mode
    return render_errors(got, ref, inputs_of(case)["z_span"], white=white_back and not last_back)


def ladder_of(case):
    """-> dict: groups; vs_exact[variant][group]; vs_x2[variant][group] (distance to the healthy x2 emulation); bars[assertion][group]
    with the assertions "x3" (x3 class vs float64), "x2" (x2 class vs float64), "x2_dist" (x2 class vs the x2 emulation); healthy
    [assertion][group]: the healthy reference arithmetic's own figure for that assertion."""
    if case.name in _LADDER:
        return _LADDER[case.name]
    out = outputs_of(case)
    groups = FIELD_GROUPS if case.kind == "field" else RENDER_GROUPS
    vs_exact = {n: errors(case, o, out["exact"]) for n, o in out.items() if n != "exact"}
    vs_x2 = {n: errors(case, o, out["x2"]) for n, o in out.items() if n == "x2_f32acc" or n.startswith("D3")}

    def defect(table, kinds, group):
        layers = range(TOUCHED_BY.get(group, N_CONTRACTIONS))
        return min(table[f"{k}@{l}"][group] for k in kinds for l in layers)

    bars = {"x3": {g: defect(vs_exact, ("D1", "D2"), g) / MARGIN for g in groups},
            "x2": {g: MARGIN * vs_exact["x2"][g] for g in groups},
            "x2_dist": {g: defect(vs_x2, ("D3",), g) / MARGIN for g in groups}}
    healthy = {"x3": vs_exact["fp32"], "x2": vs_exact["x2"], "x2_dist": vs_x2["x2_f32acc"]}
    _LADDER[case.name] = dict(groups=groups, vs_exact=vs_exact, vs_x2=vs_x2, bars=bars, healthy=healthy)
    return _LADDER[case.name]


def asserted(case, assertion, group):
    return not (assertion == "x2_dist" and group in case.no_dist)


def assertions_for(engine):
    """-> the (assertion name, reference output name) pairs an engine is held to."""
    return (("x2", "exact"), ("x2_dist", "x2")) if engine_class(engine) == "x2" else (("x3", "exact"),)


def sigma_conditioning(case):
    """Render cases: min over the rays of |sigma_last + noise| / max_s |sigma_s| in the float64 oracle.  The last sample's delta
    is 1e9, so the sign of that density decides the ray's background term."""
    i = inputs_of(case)
    sd = {k: v.double() for k, v in i["state"].items()}
    field = O.neural_field(sd, i["pts"].double(), i["freq"].double(), i["phase"].double(), i["geo"].double(), i["dirs"].double(), i["scaler"])
    sigma = field[..., -1].reshape(B, case.R, case.S)
    last = (sigma[..., -1] + i["noise"].double()[..., -1, 0]).abs()
    return float((last / sigma.abs().amax(-1)).min())
