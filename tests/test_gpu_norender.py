"""GPU parity of the generator without the 3D render (disable_render=True): the fused style-input kernel
(h3d_style_input) against the reference-written goldens and the float64 restatement (tests/_norender_reference.py), the
whole forward / staged_forward in that mode, the resize ratios that make the synthesis plan change engines, batch
independence, determinism, the entry point's argument errors, and the rasteriser feeding the generator end to end.

staged_forward: the reference's own staged_forward runs in this mode (zero render image, zero depths), so it is implemented
and checked against the 'staged/...' entries of the fixtures."""
import ctypes
import importlib
import math

import pytest
import torch

import _norender_reference as NR
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
gens = importlib.import_module("3dhumangan_amd.lib.generators")
impl = importlib.import_module("3dhumangan_amd.lib.implicit_funcitions")
pack = importlib.import_module("3dhumangan_amd.lib.generators.style_input_pack")
synthetic = importlib.import_module("3dhumangan_amd.synthetic")
conditions = importlib.import_module("3dhumangan_amd.lib.data.conditions")
L = importlib.import_module("3dhumangan_amd._lib")
DEV = "cuda"
TOL = 1e-3          # north_star: generator outputs within 1e-3 relative of the reference CPU path
LAYER_BAR = 1e-5    # the bar of test_gpu_modsynth.py's h3d_modconv1x1 check: the same engine, the same fp32 arithmetic
GOLDENS = ["gen_tiny_norender_segments", "gen_tiny_norender_semantics", "gen_tiny_norender_none"]
PREFIX = "synthesis_style_input"


def build(meta, state=None, **over):
    cfg = dict(meta)
    cfg.update(over)
    cfg["neural_field_cls"] = impl.COORDCONCATSIREN
    G = gens.Map3DGenerator(**cfg)
    if state is not None:
        G.load_state_dict(state, strict=True)
    G = G.to(DEV).eval()
    G.set_device(DEV)
    return G, cfg


def cond_to(cond):
    return {k: v.to(DEV) for k, v in cond.items()}


def condition_of(g):
    modal = g["meta"]["condition_modal_gen"]
    c = g["cond"][modal]
    return NR.scale_segments(c, g["meta"]["label_dim"]) if "segments" in modal else c


def random_state(L_, F_, Cc, layers, seed):
    """A style-input state dict with the reference's initialisation scales and non-zero biases."""
    g = torch.Generator().manual_seed(seed)
    sd = {f"{PREFIX}.from_coords.0.weight": (torch.rand(L_, Cc, 1, 1, generator=g) * 2 - 1) * math.sqrt(9 / Cc),
          f"{PREFIX}.from_coords.0.bias": 0.3 * torch.randn(L_, generator=g),
          f"{PREFIX}.network.0.weight": torch.randn(F_, 2 * L_, 1, 1, generator=g) * math.sqrt(2 / 1.04 / (2 * L_)),
          f"{PREFIX}.network.0.bias": 0.1 * torch.randn(F_, generator=g)}
    if layers == 2:
        sd[f"{PREFIX}.network.2.weight"] = torch.randn(F_, F_, 1, 1, generator=g) * math.sqrt(2 / 1.04 / F_)
        sd[f"{PREFIX}.network.2.bias"] = 0.1 * torch.randn(F_, generator=g)
    return sd


def random_condition(B, Cc, hw, seed, label_dim=26):
    g = torch.Generator().manual_seed(seed)
    if Cc == 1:
        return NR.scale_segments(torch.randint(0, label_dim, (B,) + tuple(hw), generator=g), label_dim)
    return torch.rand(B, 3, *hw, generator=g) * 2 - 1


@pytest.mark.parametrize("name", GOLDENS)
def test_kernel_golden(name):
    g = load_golden(name)
    c = condition_of(g)
    plan = pack.StyleInputPlan(g["state"], PREFIX, DEV)
    out = plan.run(c.to(DEV), g["z"].to(DEV))
    assert out.shape == (2, c.shape[2] * c.shape[3], g["meta"]["feature_dim"])
    e = rel_err(NR.to_nchw(out.cpu(), tuple(c.shape[2:])), g["stage"]["feature_maps"])
    e64 = rel_err(out.cpu(), NR.style_input(g["state"], c, g["z"]))
    print(f"{name}: h3d_style_input vs golden {e:.3e}, vs float64 restatement {e64:.3e}")
    assert e < TOL
    assert e64 < LAYER_BAR
    # spade_latent_input=False: the zero latent of the reference
    off = plan.run(c.to(DEV), g["z"].to(DEV), latent_input=False)
    assert rel_err(off.cpu(), NR.style_input(g["state"], c, g["z"], latent_input=False)) < LAYER_BAR
    assert torch.equal(off, plan.run(c.to(DEV), torch.zeros_like(g["z"]).to(DEV)))


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("Cc", [1, 3])
@pytest.mark.parametrize("hw", [(7, 6), (9, 18), (33, 31)])
@pytest.mark.parametrize("width", [64, 130, 256, 420])
def test_kernel_vs_restatement(width, hw, Cc, layers):
    """Every register tiling (1..4 column tiles per wave), a width that is not a multiple of 32, one ragged tile, several
    tiles, a last tile that is 63/64 full; the reference is the restatement in float64 on the CPU."""
    sd = random_state(width, width, Cc, layers, seed=width + hw[0])
    c = random_condition(2, Cc, hw, seed=width + Cc)
    z = torch.randn(2, width, generator=torch.Generator().manual_seed(hw[1]))
    plan = pack.StyleInputPlan(sd, PREFIX, DEV)
    assert plan.n_layers == layers
    out = plan.run(c.to(DEV), z.to(DEV)).cpu()
    ref = NR.style_input(sd, c, z)
    e = rel_err(out, ref)
    print(f"width {width} map {hw[0]}x{hw[1]} Cc={Cc} layers={layers}: rel_err {e:.3e} (bar {LAYER_BAR:.0e})")
    assert out.shape == ref.shape and torch.isfinite(out).all()
    assert e < LAYER_BAR


@pytest.mark.parametrize("L_,F_", [(96, 40), (40, 160)])
def test_kernel_unequal_latent_and_feature_width(L_, F_):
    sd = random_state(L_, F_, 3, 2, seed=L_)
    c = random_condition(2, 3, (9, 18), seed=F_)
    z = torch.randn(2, L_, generator=torch.Generator().manual_seed(5))
    out = pack.StyleInputPlan(sd, PREFIX, DEV).run(c.to(DEV), z.to(DEV)).cpu()
    assert rel_err(out, NR.style_input(sd, c, z)) < LAYER_BAR


@pytest.mark.parametrize("name", GOLDENS)
def test_forward_golden(name):
    g = load_golden(name)
    G, cfg = build(g["meta"], g["state"])
    out = G.forward(g["z"].to(DEV), cond_to(g["cond"]), **dict(cfg, disable_render=True))
    e = rel_err(out["rgbs"].cpu(), g["out"]["rgbs"])
    print(f"{name}: forward(disable_render=True) rgbs {e:.3e}")
    assert out["rgbs"].shape == g["out"]["rgbs"].shape and e < TOL
    assert out["rgbs_render"].shape == g["out"]["rgbs_render"].shape and out["rgbs_render"].is_cuda
    assert float(out["rgbs_render"].abs().max()) == 0.0
    plain = G.forward(g["z"].to(DEV), cond_to(g["cond"]), **dict(cfg, disable_render=True, disable_synthesis=True))
    assert plain["rgbs"].shape == g["out"]["rgbs_render"].shape and float(plain["rgbs"].abs().max()) == 0.0


@pytest.mark.parametrize("name", GOLDENS)
def test_staged_forward_golden(name):
    """What the reference's staged_forward returns in this mode: the truncated latent feeds the style input, the render image
    is zero, the depth map comes from zero depths, and the keys are rgbs, rgbs_render, depths, skeletons."""
    g = load_golden(name)
    G, cfg = build(g["meta"], g["state"])
    run = dict(cfg, disable_render=True, truncation_psi=0.7, nerf_noise=0, last_back=cfg["eval_last_back"])
    avg = tuple(g["avg"][k].to(DEV) for k in ("z", "freq", "phase", "styles"))
    out = G.staged_forward(g["z"].to(DEV), cond_to(g["cond"]), avg_latent=avg, **run)
    s = g["staged"]
    assert sorted(out) == ["depths", "rgbs", "rgbs_render", "skeletons"]
    assert not out["depths"].is_cuda and out["depths"].shape == s["depths"].shape
    assert rel_err(out["depths"], s["depths"]) < TOL
    assert float(out["rgbs_render"].abs().max()) == 0.0 and out["rgbs_render"].shape == s["rgbs_render"].shape
    e = rel_err(out["rgbs"].cpu(), s["rgbs"])
    print(f"{name}: staged_forward(disable_render=True) rgbs {e:.3e}")
    assert e < TOL
    assert torch.equal(out["skeletons"].cpu(), g["cond"]["skeletons_xyz"])
    plain = G.staged_forward(g["z"].to(DEV), cond_to(g["cond"]), avg_latent=avg, disable_synthesis=True, **run)
    assert plain["rgbs"].shape == s["rgbs"].shape and float(plain["rgbs"].abs().max()) == 0.0


@pytest.mark.parametrize("name", [GOLDENS[0], GOLDENS[2]])
@pytest.mark.parametrize("gen_hw,cond_hw", [((16, 8), (16, 8)), ((16, 8), (24, 12)), ((64, 32), (64, 32)), ((64, 32), (96, 48))])
def test_resize_ratios_and_engine_fallback(name, gen_hw, cond_hw):
    """A condition map as large as the image, and larger: the x3 engine's matrix-core resize covers neither ratio (16 x 8 it
    refuses for its width as well; 64 x 32 for the ratio alone), so the SPADE plan has to run another engine, and it must
    not raise.  The reference is the float64 restatement of the style input fed through _synthesize on the fp32 engine."""
    g = load_golden(name)
    G, cfg = build(g["meta"], g["state"], gen_height=gen_hw[0], gen_width=gen_hw[1])
    assert not L.load().h3d_synthesis_x3_geometry_ok(gen_hw[0], gen_hw[1], cond_hw[0], cond_hw[1])
    seg = torch.randint(0, cfg["label_dim"], (2,) + cond_hw, generator=torch.Generator().manual_seed(cond_hw[0]))
    cond = cond_to(g["cond"])
    cond["rasterized_segments"] = seg.to(DEV)
    c = NR.scale_segments(seg, cfg["label_dim"])
    z = g["z"].to(DEV)
    out = G.forward(z, cond, **dict(cfg, disable_render=True))["rgbs"]
    # reference: restatement -> the existing _synthesize on the fp32 engine
    fmap = NR.style_input(g["state"], c, g["z"]).float().to(DEV).contiguous()
    plan = G.synthesis_plan(DEV)
    keep = plan.engine
    plan.engine = "f32"
    try:
        ref = G._synthesize(fmap, g["stage"]["styles"].to(DEV), cond_hw)
    finally:
        plan.engine = keep
    e = rel_err(out, ref)
    print(f"{name} {gen_hw[0]}x{gen_hw[1]} <- {cond_hw[0]}x{cond_hw[1]} engine {keep}: rel_err {e:.3e}")
    assert out.shape == (2, 3) + tuple(gen_hw) and torch.isfinite(out).all()
    assert e < TOL


@pytest.mark.parametrize("Cc", [1, 3])
def test_batch_independence(Cc):
    """Image i of a B = 3 call equals the B = 1 call on that image alone, bit for bit (same bias-table rows): a slip in the
    bias-table or tile-to-image indexing shows here."""
    sd = random_state(64, 64, Cc, 2, seed=9)
    c = random_condition(3, Cc, (9, 18), seed=Cc).to(DEV)
    z = torch.randn(3, 64, generator=torch.Generator().manual_seed(2)).to(DEV)
    plan = pack.StyleInputPlan(sd, PREFIX, DEV)
    table = plan.bias_table(z)
    both = plan.launch(c, table)
    assert not torch.equal(both[0], both[1]) and not torch.equal(both[1], both[2])
    for i in range(3):
        alone = plan.launch(c[i:i + 1], table[i:i + 1])
        assert torch.equal(alone[0], both[i]), i


@pytest.mark.parametrize("name", GOLDENS)
def test_two_runs_are_bit_identical(name):
    g = load_golden(name)
    G, cfg = build(g["meta"], g["state"])
    plan = G.style_input_plan(DEV)
    c = condition_of(g).to(DEV)
    assert torch.equal(plan.run(c, g["z"].to(DEV)), plan.run(c, g["z"].to(DEV)))
    a = G.forward(g["z"].to(DEV), cond_to(g["cond"]), **dict(cfg, disable_render=True))["rgbs"]
    b = G.forward(g["z"].to(DEV), cond_to(g["cond"]), **dict(cfg, disable_render=True))["rgbs"]
    assert torch.equal(a, b)


def test_argument_errors():
    lib = L.load()
    assert lib.h3d_style_input_lds_bytes(512, 512) > 0 and lib.h3d_style_input_lds_bytes(32, 512) > 0
    assert lib.h3d_style_input_lds_bytes(544, 32) < 0 and lib.h3d_style_input_lds_bytes(32, 544) < 0
    sd = random_state(32, 32, 1, 2, seed=1)
    plan = pack.StyleInputPlan(sd, PREFIX, DEV)
    cond = torch.zeros(1, 3, 4, 4, device=DEV)
    bias = torch.zeros(1, 544, device=DEV)
    out = torch.zeros(1, 16, 544, device=DEV)

    def call(cond_=cond, Cc=1, Lw=32, Fw=32, Hc=4, out_=out):
        return lib.h3d_style_input(L.ptr(cond_), L.ptr(bias), L.ptr(plan.w_coord), L.ptr(plan.w0), L.ptr(plan.w1), L.ptr(plan.b1),
                                   L.ptr(out_), 1, Cc, Hc, 4, Lw, Fw, 2, L.stream_handle())

    assert call(Cc=2) == -1 and b"1 (segments) or 3 (semantics)" in lib.h3d_last_error()
    assert call(cond_=None) == -1 and b"null pointer" in lib.h3d_last_error()
    assert call(out_=None) == -1 and b"null pointer" in lib.h3d_last_error()
    assert call(Hc=0) == -1 and b"bad shape" in lib.h3d_last_error()
    assert call(Fw=544) == -2 and b"width 544" in lib.h3d_last_error()
    assert call(Lw=544) == -2 and b"width 544" in lib.h3d_last_error()
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0                      # refused before any launch
    wide = pack.StyleInputPlan(random_state(544, 32, 1, 1, seed=2), PREFIX, DEV)
    with pytest.raises(L.H3DError, match="width 544"):
        wide.run(torch.zeros(1, 1, 4, 4, device=DEV), torch.zeros(1, 544, device=DEV))
    g = load_golden(GOLDENS[0])
    G, cfg = build(g["meta"], g["state"])
    args = (g["z"].to(DEV), cond_to(g["cond"]))
    with pytest.raises(NotImplementedError, match="disable_render"):
        G.forward(*args, differentiable=True, **dict(cfg, disable_render=True))
    G.train()
    with pytest.raises(NotImplementedError, match="disable_render"):
        G.forward(*args, **dict(cfg, disable_render=True))


def test_rasteriser_feeds_the_generator_end_to_end():
    """h3d_mesh_rasterize (through the camera front-end, on the tube body of test_gpu_raster.py) -> forward(disable_render=True)
    for segments and for semantics, and the sample app's frame loop (staged_forward) on the same front-end."""
    app = importlib.import_module("3dhumangan_amd.apps.sample_from_generator")
    B = 2
    mesh, faces, labels = synthetic.make_mesh_conditions(B, seed=2, scale=0.7)
    pre = conditions.CameraPreprocessor(DEV)
    pre.init_smpl(faces, labels)
    data = cond_to(mesh)
    for name, hw in ((GOLDENS[0], (24, 12)), (GOLDENS[1], (16, 8)), (GOLDENS[2], (32, 16))):
        g = load_golden(name)
        G, cfg = build(g["meta"], g["state"])
        view = pre.forward_with_rotation(data, torch.tensor([0.0, 0.9]), torch.tensor([0.0, 0.2]), torch.zeros(B),
                                         gen_height=hw[0], gen_width=hw[1])
        seg = view["rasterized_segments"]
        assert seg.shape == (B,) + hw and (seg != 1).any() and (seg == 1).any()          # body and background
        out = G.forward(g["z"].to(DEV), view, **dict(cfg, disable_render=True))
        assert out["rgbs"].shape == (B, 3, cfg["gen_height"], cfg["gen_width"]) and torch.isfinite(out["rgbs"]).all()
        assert float(out["rgbs"].std()) > 0 and float(out["rgbs_render"].abs().max()) == 0.0
        # the body matters: another view gives another image
        other = pre.forward_with_rotation(data, torch.tensor([2.0, -1.5]), torch.tensor([0.1, 0.0]), torch.zeros(B),
                                          gen_height=hw[0], gen_width=hw[1])
        assert not torch.equal(G.forward(g["z"].to(DEV), other, **dict(cfg, disable_render=True))["rgbs"], out["rgbs"])
    # the app's loop: one record, the front-end rasterises at the config's image size, staged_forward per angle
    config = dict(cfg, disable_render=True, truncation_psi=0.7, nerf_noise=0, last_back=cfg["eval_last_back"], cache_avg_latent=True)
    single = {k: v[:1] for k, v in mesh.items()}
    frames, semantics = app.generate_frames(G, pre, config, 3, single, 2, math.pi / 6, 0, False)
    assert frames.shape == (2, cfg["gen_height"], cfg["gen_width"], 3) and frames.std() > 0
    assert semantics.shape == frames.shape and not (frames[0] == frames[1]).all()
