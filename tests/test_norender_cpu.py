"""Host side of the generator without the 3D render (disable_render=True): the pure-torch restatement of the style input
against the reference-written goldens, the fold of the latent half into a per-image bias, the plan's packing, the
parameter schema and the refusals.

staged_forward: the reference's own staged_forward runs in this mode (its depth bookkeeping works on a zero depth tensor), so
both entry points are implemented; the fixtures carry its outputs ('staged/...') and its keys are rgbs, rgbs_render,
depths, skeletons."""
import importlib

import pytest
import torch

import _norender_reference as NR
from conftest import load_golden, rel_err

gens = importlib.import_module("3dhumangan_amd.lib.generators")
impl = importlib.import_module("3dhumangan_amd.lib.implicit_funcitions")
pack = importlib.import_module("3dhumangan_amd.lib.generators.style_input_pack")
spack = importlib.import_module("3dhumangan_amd.lib.generators.fragment_pack")

GOLDENS = ["gen_tiny_norender_segments", "gen_tiny_norender_semantics", "gen_tiny_norender_none"]
TOL = 5e-5          # the bar of the oracle-vs-golden tests: the goldens are fp32 results of the reference


def build(meta, state=None):
    cfg = dict(meta)
    cfg["neural_field_cls"] = impl.COORDCONCATSIREN
    G = gens.Map3DGenerator(**cfg)
    if state is not None:
        G.load_state_dict(state, strict=True)
    return G.eval(), cfg


def condition_of(g):
    """The condition map as the generator hands it to the style input: [B, Cc, Hc, Wc] fp32."""
    modal = g["meta"]["condition_modal_gen"]
    c = g["cond"][modal]
    return NR.scale_segments(c, g["meta"]["label_dim"]) if "segments" in modal else c


def test_fixtures_cover_both_conditions_and_both_normalisations():
    metas = [load_golden(n)["meta"] for n in GOLDENS]
    assert [m["condition_modal_gen"] for m in metas] == ["rasterized_segments", "rasterized_semantics", "rasterized_segments"]
    assert [m["spatial_normalization"] for m in metas] == ["batch_norm", "batch_norm", "none"]
    assert [m["map3d_mode"] for m in metas] == ["mixed", "isolated", "mixed"]
    for n in GOLDENS:
        g = load_golden(n)
        m = g["meta"]
        seg, sem = g["cond"]["rasterized_segments"], g["cond"]["rasterized_semantics"]
        assert seg.dtype == torch.int64 and int(seg.min()) == 0 and int(seg.max()) == m["label_dim"] - 1
        assert sem.shape[1] == 3 and float(sem.abs().max()) == 1.0
        # the condition map has its own resolution: neither the image's nor the render's
        assert tuple(seg.shape[1:]) not in ((m["gen_height"], m["gen_width"]), (m["render_height"], m["render_width"]))
        assert g["stage"]["feature_maps"].shape == (2, m["feature_dim"]) + tuple(seg.shape[1:])
        for k in ("from_coords.0.bias", "network.0.bias", "network.2.bias"):
            assert float(g["state"]["synthesis_style_input." + k].abs().max()) > 0, k
        assert float(g["out"]["rgbs_render"].abs().max()) == 0.0 and float(g["staged"]["rgbs_render"].abs().max()) == 0.0


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_reproduces_the_golden(name):
    g = load_golden(name)
    c = condition_of(g)
    hw = tuple(c.shape[2:])
    for explicit in (False, True):
        fmap = NR.style_input(g["state"], c, g["z"], explicit_cat=explicit)
        assert rel_err(NR.to_nchw(fmap, hw), g["stage"]["feature_maps"]) < TOL
    # staged run: the truncated latent (0.7 with the stored average) feeds the style input
    z = g["avg"]["z"] + 0.7 * (g["z"] - g["avg"]["z"])
    assert rel_err(NR.to_nchw(NR.style_input(g["state"], c, z), hw), g["staged"]["feature_maps"]) < TOL


@pytest.mark.parametrize("name", GOLDENS)
def test_fold_identity_and_plan_tables(name):
    """The [B, F] bias table against the explicit cat / expand form, and the plan's table and packing against both."""
    g = load_golden(name)
    c, z, sd = condition_of(g), g["z"], g["state"]
    folded, explicit = NR.style_input(sd, c, z), NR.style_input(sd, c, z, explicit_cat=True)
    assert rel_err(folded, explicit) < 1e-12                       # float64: the same sums in another order
    G, _ = build(g["meta"], sd)
    plan = G.style_input_plan("cpu")
    assert isinstance(plan, pack.StyleInputPlan) and G.style_input_plan("cpu") is plan       # cached per weight version
    L, F = g["meta"]["latent_dim"], g["meta"]["feature_dim"]
    assert (plan.Cc, plan.L, plan.F, plan.n_layers) == (c.shape[1], L, F, 2)
    table = plan.bias_table(z)
    assert table.shape == (2, F) and rel_err(table, NR.bias_table(sd, z)) < 1e-5
    # the explicit form through network.0 alone, at one pixel: W_0 [f ; zn] + b_0 == W_0[:, :L] f + table
    w0 = sd["synthesis_style_input.network.0.weight"].flatten(1).double()
    f = torch.randn(2, L, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    zn = NR.normalize_2nd_moment(z.double())
    want = torch.cat([f, zn], dim=1) @ w0.t() + sd["synthesis_style_input.network.0.bias"].double()
    assert rel_err(f @ w0[:, :L].t() + table.double(), want) < 1e-5
    # packing: the same bytes as the shared packer on the [F, L] / [F, F] matrices, vectors zero padded
    assert torch.equal(plan.w0, spack.pack_matrix(w0[:, :L].float(), plan.LP // 8, plan.FP // 32))
    assert torch.equal(plan.w1, spack.pack_matrix(sd["synthesis_style_input.network.2.weight"].flatten(1), plan.FP // 8, plan.FP // 32))
    wc = sd["synthesis_style_input.from_coords.0.weight"].flatten(1)
    assert plan.w_coord.shape == ((plan.Cc + 1) * plan.LP,)
    assert torch.equal(plan.w_coord[: L], wc[:, 0]) and torch.equal(plan.w_coord[plan.Cc * plan.LP: plan.Cc * plan.LP + L],
                                                                    sd["synthesis_style_input.from_coords.0.bias"])
    with torch.no_grad():
        G.synthesis_style_input.network[0].bias.add_(1.0)
    assert G.style_input_plan("cpu") is not plan


@pytest.mark.parametrize("name", GOLDENS[:2])
def test_no_latent_input_equals_a_zero_latent(name):
    g = load_golden(name)
    c, z, sd = condition_of(g), g["z"], g["state"]
    off = NR.style_input(sd, c, z, latent_input=False)
    assert torch.equal(off, NR.style_input(sd, c, torch.zeros_like(z)))
    assert torch.equal(off, NR.style_input(sd, c, torch.zeros_like(z), explicit_cat=True, latent_input=False))
    assert rel_err(off, NR.style_input(sd, c, z)) > 1e-3           # the latent matters in these fixtures
    G, _ = build(g["meta"], sd)
    plan = G.style_input_plan("cpu")
    b0 = sd["synthesis_style_input.network.0.bias"]
    assert torch.equal(plan.bias_table(z, latent_input=False), b0.expand(2, -1))
    # normalize_2nd_moment(0) = 0: the table of a zero latent is b_0 too
    assert torch.equal(plan.bias_table(torch.zeros_like(z)), b0.expand(2, -1))


@pytest.mark.parametrize("name", GOLDENS)
def test_generator_loads_the_reference_state_dict(name):
    g = load_golden(name)
    G, _ = build(g["meta"], g["state"])
    sd = G.state_dict()
    assert set(sd) == set(g["state"])
    for k, v in g["state"].items():
        assert sd[k].shape == v.shape, k
    cc = 1 if "segments" in g["meta"]["condition_modal_gen"] else 3
    assert sd["synthesis_style_input.from_coords.0.weight"].shape == (32, cc, 1, 1)
    assert sd["synthesis_style_input.network.0.weight"].shape == (32, 64, 1, 1)
    assert sd["synthesis_style_input.network.2.weight"].shape == (32, 32, 1, 1)


def test_plan_takes_the_layer_count_from_the_module():
    g = load_golden(GOLDENS[0])
    sd = {k: v for k, v in g["state"].items() if k.startswith("synthesis_style_input.")}
    one = {k: v for k, v in sd.items() if ".network.2." not in k}
    assert pack.StyleInputPlan(one, "synthesis_style_input", "cpu").n_layers == 1
    three = dict(sd)
    three["synthesis_style_input.network.4.weight"] = sd["synthesis_style_input.network.2.weight"]
    three["synthesis_style_input.network.4.bias"] = sd["synthesis_style_input.network.2.bias"]
    with pytest.raises(NotImplementedError, match="one or two"):
        pack.StyleInputPlan(three, "synthesis_style_input", "cpu")


def test_training_and_interpolation_refusals_carry_their_messages():
    g = load_golden(GOLDENS[0])
    G, cfg = build(g["meta"], g["state"])
    run = dict(cfg, disable_render=True)
    with pytest.raises(NotImplementedError, match="disable_render"):
        G._forward(g["z"], g["cond"], differentiable=True, **run)
    for mode in ("nearest", "bicubic"):
        with pytest.raises(NotImplementedError, match=f"disable_render.*feature_map_interpolation='{mode}'"):
            G._forward(g["z"], g["cond"], **dict(run, feature_map_interpolation=mode))
        with pytest.raises(NotImplementedError, match=f"disable_render.*feature_map_interpolation='{mode}'"):
            G._staged_forward(g["z"], g["cond"], truncation_psi=1.0, **dict(run, feature_map_interpolation=mode))
    # train() selects the differentiable path: refused by name as well (wants_autograd is what forward() asks)
    G.train()
    assert G.wants_autograd({}) is True
    with pytest.raises(NotImplementedError, match="disable_render"):
        G._forward(g["z"], g["cond"], differentiable=G.wants_autograd({}), **run)


def test_disable_synthesis_returns_the_zero_image_without_a_kernel():
    g = load_golden(GOLDENS[0])
    G, cfg = build(g["meta"], g["state"])
    out = G._forward(g["z"], g["cond"], **dict(cfg, disable_render=True, disable_synthesis=True))
    assert out["rgbs"].shape == (2, 3, cfg["render_height"], cfg["render_width"])
    assert float(out["rgbs"].abs().max()) == 0.0 and out["rgbs_render"] is out["rgbs"]
