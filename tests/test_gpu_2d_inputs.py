"""GPU parity of the synthesis input variants: the h3d_synth_input op (forward, adjoint, determinism) against its float64
restatement, and the generator with 2d_label_input / 2d_latent_input / feature_dim != hidden_dim against vectors written by the
reference module (inference through forward and staged_forward, train mode through forward + backward)."""
import importlib

import pytest
import torch

import _2d_inputs_reference as R
from conftest import grad_errors, load_golden, rel_err

pytestmark = pytest.mark.gpu

gens = importlib.import_module("3dhumangan_amd.lib.generators")
impl = importlib.import_module("3dhumangan_amd.lib.implicit_funcitions")
op = importlib.import_module("3dhumangan_amd.lib.components.ops.synth_input")
_lib = importlib.import_module("3dhumangan_amd._lib")

DEV = "cuda"
LABEL_DIM = 26

# (B, H, W, F, L, K): H == 1 and a tile tail | latent as wide as the sine part | F no multiple of 32, P = 63 | the released
# checkpoint's width, P = 201 (two forward workgroups) | widths that are no multiple of 4 (the scalar kernels) | P = 1200: three
# backward workgroups per image, ten forward ones, without / with the label map
SHAPES = [(1, 1, 5, 8, 0, 2), (3, 16, 8, 32, 32, 3), (2, 9, 7, 40, 24, 3), (2, 67, 3, 420, 0, 3),
          (2, 5, 3, 30, 5, 3), (1, 40, 30, 8, 4, 2), (2, 40, 30, 12, 8, 3)]


def op_case(B, H, W, F, L, K):
    g = torch.Generator().manual_seed(1000 * B + 100 * H + 10 * F + L + K)
    w = (torch.rand(F, K, generator=g) * 2 - 1) * (9 / K) ** 0.5          # SynthesisInput's own initialisation range
    b = torch.randn(F, generator=g)
    z = torch.randn(B, L, generator=g) if L else None
    seg = None
    if K == 3:
        seg = torch.randint(0, LABEL_DIM, (B, H, W), generator=g)
        seg.view(B, -1)[:, 0], seg.view(B, -1)[:, -1] = 0, LABEL_DIM - 1
    p = torch.randn(B, H * W, F + L, generator=g)
    return w, b, z, seg, p


def to_dev(t, grad=False):
    return None if t is None else (t.to(DEV).requires_grad_(True) if grad else t.to(DEV))


@pytest.mark.parametrize("shape", SHAPES)
def test_op_forward_against_float64(shape):
    """|err| <= 4 * 2^-23 * max(1, A), A = max_n (sum_k |w_nk| + |b_n|): coordinates and label lie in [-1, 1], the argument is
    three fused fp32 operations (each rounds a value of at most A), |sin'| <= 1, the sine adds about one ulp of its own.
    The latent channels are copies."""
    B, H, W, F, L, K = shape
    w, b, z, seg, _ = op_case(*shape)
    ref = R.block0_input(w, b, H, W, B, seg, LABEL_DIM, z)
    out = op.synth_input(to_dev(w), to_dev(b), (H, W), B, seg=to_dev(seg), z=to_dev(z), label_dim=LABEL_DIM)
    assert out.shape == (B, H * W, F + L) and out.dtype == torch.float32 and not out.requires_grad
    A = float((w.abs().sum(dim=1) + b.abs()).max())
    err = float((out[..., :F].cpu().double() - ref[..., :F]).abs().max())
    print(f"synth_input forward {shape}: max |err| {err:.3e}, bound {4 * 2.0 ** -23 * max(1.0, A):.3e}")
    assert err <= 4 * 2.0 ** -23 * max(1.0, A)
    if L:
        assert torch.equal(out[..., F:].cpu(), z[:, None].expand(B, H * W, L))


@pytest.mark.parametrize("shape", SHAPES)
def test_op_backward_against_float64_autograd_and_is_deterministic(shape):
    """dw, db (the sine's adjoint reduced over all pixels: test_film_sin_forward_backward's 4e-5) and dz (a plain fp32 reduction:
    test_wgrad_narrow_vs_fp64's 2e-5) against float64 autograd; a second run gives the same bits."""
    B, H, W, F, L, K = shape
    w, b, z, seg, p = op_case(*shape)
    leaves = [t.double().requires_grad_(True) for t in (w, b)] + ([z.double().requires_grad_(True)] if L else [])
    ref = R.block0_input(leaves[0], leaves[1], H, W, B, seg, LABEL_DIM, leaves[2] if L else None)
    want = torch.autograd.grad((ref * p.double()).sum(), leaves)
    runs = []
    for _ in range(2):
        wd, bd, zd = to_dev(w, True), to_dev(b, True), to_dev(z, bool(L))
        out = op.synth_input(wd, bd, (H, W), B, seg=to_dev(seg), z=zd, label_dim=LABEL_DIM)
        assert out.requires_grad
        (out * p.to(DEV)).sum().backward()
        runs.append([wd.grad, bd.grad] + ([zd.grad] if L else []))
    for name, got, ref_g, tol in zip(("dw", "db", "dz"), runs[0], want, (4e-5, 4e-5, 2e-5)):
        e = rel_err(got.cpu(), ref_g)
        print(f"synth_input backward {shape}: {name} rel err {e:.3e} (bound {tol:.0e})")
        assert got.shape == ref_g.shape and e < tol, name
    for a, c in zip(*runs):
        assert torch.equal(a, c)


def test_op_refuses_what_it_does_not_take():
    w, b, z, seg, _ = op_case(2, 4, 4, 8, 4, 3)
    with pytest.raises(ValueError, match="3 input channels"):
        op.synth_input(to_dev(w), to_dev(b), (4, 4), 2, seg=None, z=to_dev(z))
    with pytest.raises(ValueError, match="seg must be int64"):
        op.synth_input(to_dev(w), to_dev(b), (4, 4), 2, seg=to_dev(seg)[:, :3], z=to_dev(z), label_dim=LABEL_DIM)
    with pytest.raises(_lib.H3DError):
        op.synth_input(w, b, (4, 4), 2, seg=seg, z=z, label_dim=LABEL_DIM)          # CPU tensors: no fallback


# ------------------------------------------------------------------ the generator

LAYERWISE = ["gen_tiny_2d_label", "gen_tiny_2d_latent", "gen_tiny_2d_label_latent", "gen_tiny_wide_feature",
             "gen_tiny_2d_label_norender"]
# tests/test_gpu_generator.py: (field engine, synthesis engine)
ENGINES = [("f16x2", "f16x2"), ("f16x2t", "f16x2t"), ("f16x3", "bf16x3"), ("f16x3t", "bf16x3t"), ("f32", "f32")]
TOL = 1e-3                # tests/test_gpu_generator.py: generator outputs within 1e-3 relative of the reference CPU path
TOL_LAYERWISE = 1e-4      # test_differentiable_path_in_eval_mode_matches_the_inference_engines: the layer-wise path against a golden


def build(g, train=False):
    cfg = dict(g["meta"])
    cfg["neural_field_cls"] = impl.COORDCONCATSIREN
    G = gens.Map3DGenerator(**cfg)
    G.load_state_dict(g["state"], strict=True)
    G = G.to(DEV)
    G.set_device(DEV)
    if g["meta"]["condition_modal_gen"] != "rasterized_segments":          # the fixture without the 3D render
        cfg["disable_render"] = True
    return (G.train() if train else G.eval()), cfg


def cond_to(cond):
    return {k: v.to(DEV) for k, v in cond.items()}


def run_both(G, cfg, g):
    """forward and staged_forward (truncation 0.7 with the stored average latent) as the reference ran them."""
    out = G.forward(g["z"].to(DEV), cond_to(g["cond"]), jitter=g["jitter"].to(DEV), noise=g["noise"].to(DEV), **cfg)
    run = dict(cfg)
    run.update(truncation_psi=0.7, nerf_noise=0, last_back=cfg["eval_last_back"])
    avg = tuple(g["avg"][k].to(DEV) for k in ("z", "freq", "phase", "styles"))
    sout = G.staged_forward(g["z"].to(DEV), cond_to(g["cond"]), jitter=g["staged"]["jitter"].to(DEV), avg_latent=avg, **run)
    return out, sout


@pytest.mark.parametrize("name", LAYERWISE)
def test_layerwise_variants_against_the_golden(name):
    """Label map / latent / a wider feature_dim as block 0's input: inference runs layer by layer (running statistics, stored
    spectral-norm vectors) behind the new input op.  The image is held to the layer-wise path's 1e-4 with the render in front
    of it on the fp32 field engine and on the default one; the render image to the generator's 1e-3."""
    g = load_golden(name)
    G, cfg = build(g)
    before = {k: v.clone() for k, v in G.state_dict().items()}
    assert G._layerwise_synthesis()
    for precision, tol in (("f32", TOL_LAYERWISE), (G.neural_field.precision, TOL_LAYERWISE)):
        G.neural_field.precision = precision
        out, sout = run_both(G, cfg, g)
        for got, want, what in ((out, g["out"], "forward"), (sout, g["staged"], "staged_forward")):
            e_render, e_rgb = rel_err(got["rgbs_render"].cpu(), want["rgbs_render"]), rel_err(got["rgbs"].cpu(), want["rgbs"])
            print(f"{name} {what} field engine {precision}: rgbs_render {e_render:.2e}, rgbs {e_rgb:.2e} (bound {tol:.0e})")
            assert not got["rgbs"].requires_grad and got["rgbs"].shape == want["rgbs"].shape
            assert e_render < TOL and e_rgb < tol, (what, precision)
        assert rel_err(sout["depths"], g["staged"]["depths"]) < TOL
    assert all(torch.equal(v, before[k]) for k, v in G.state_dict().items())         # inference leaves every buffer alone


@pytest.mark.parametrize("engines", [None] + ENGINES)
def test_narrow_feature_runs_on_the_fused_engines(engines):
    """feature_dim 16 under hidden_dim 32: block 0's input side zero-padded in the plan, every SPADE engine tier (None: the
    plan's own choice)."""
    g = load_golden("gen_tiny_narrow_feature")
    G, cfg = build(g)
    assert not G._layerwise_synthesis()
    plan = G.synthesis_plan(DEV)
    assert plan.x3t_supported() and plan.engine != "f32"          # a network the matrix-core engines take: nothing falls to fp32
    if engines is not None:
        G.neural_field.precision, plan.engine = engines
    out, sout = run_both(G, cfg, g)
    for got, want, what in ((out, g["out"], "forward"), (sout, g["staged"], "staged_forward")):
        e_render, e_rgb = rel_err(got["rgbs_render"].cpu(), want["rgbs_render"]), rel_err(got["rgbs"].cpu(), want["rgbs"])
        print(f"narrow feature {what} engines {engines or G.synthesis_plan(DEV).engine}: rgbs_render {e_render:.2e}, rgbs {e_rgb:.2e}")
        assert e_render < TOL and e_rgb < TOL, what


@pytest.mark.parametrize("engine", ["f16x2", "bf16x3"])
def test_narrow_feature_on_the_register_engines_vs_float64(engine):
    """The tiny fixture's 16 x 8 image is outside the register engines' resize geometry (they hand over to the LDS-resident
    engine): feature_dim 32 under hidden_dim 64 at a geometry they accept, against the float64 restatement (bound: the
    generator's 1e-3, as tests/test_gpu_generator.py::test_x3_synthesis_geometries_vs_oracle)."""
    synthetic = importlib.import_module("3dhumangan_amd.synthetic")
    meta = dict(load_golden("gen_tiny_mixed")["meta"])
    meta.update(hidden_dim=64, latent_dim=64, feature_dim=32, gen_height=41, gen_width=32, render_height=7, render_width=6,
                num_steps=8)
    torch.manual_seed(105)
    cfg = dict(meta, neural_field_cls=impl.COORDCONCATSIREN)
    G = gens.Map3DGenerator(**cfg).to(DEV).eval()
    G.set_device(DEV)
    plan = G.synthesis_plan(DEV)
    assert (plan.C, plan.Cin) == (64, 32) and plan.engine == "f16x2" and plan.x3_supported()
    assert _lib.load().h3d_synthesis_x3_geometry_ok(41, 32, 7, 6) == 1
    plan.engine = engine
    sd = {k: v.detach().cpu().clone() for k, v in G.state_dict().items()}
    cond = synthetic.make_conditions(2, n_vertices=100, seed=5)
    z, jit = torch.randn(2, 64), torch.rand(2, 42, 8, 1)
    ref = R.generator_forward(sd, meta, z, cond, jit, None)
    out = G.forward(z.to(DEV), cond_to(cond), jitter=jit.to(DEV), **cfg)
    e = rel_err(out["rgbs"].cpu(), ref["rgbs"])
    print(f"narrow feature on {engine}: rgbs {e:.2e}")
    assert e < TOL


def test_latent_pool_feeds_block_0():
    """forward with latent_indices: the pool's latent is the one block 0 reads (reference :215, :264)."""
    g = load_golden("gen_tiny_2d_latent")
    G, cfg = build(g)
    with torch.no_grad():
        G.latent_pool.latents[:2].copy_(g["z"].to(DEV))
    kw = dict(jitter=g["jitter"].to(DEV), noise=g["noise"].to(DEV))
    other = torch.randn_like(g["z"]).to(DEV)
    out = G.forward(other, cond_to(g["cond"]), latent_indices=torch.tensor([0, 1], device=DEV), **kw, **cfg)
    assert rel_err(out["rgbs"].cpu(), g["out"]["rgbs"]) < TOL


@pytest.fixture(params=["library_wgrad", "hip_wgrad"])
def wgrad_route(request, monkeypatch):
    """As in tests/test_gpu_train_path.py: once as it would run, once with every eligible layer on the HIP weight-gradient kernel."""
    lin = importlib.import_module("3dhumangan_amd.lib.components.ops.linear")
    if request.param == "hip_wgrad":
        monkeypatch.setattr(lin, "MIN_ROWS", 0)
    return request.param


@pytest.mark.parametrize("name", ["gen_train_2d_label_latent", "gen_train_narrow_feature"])
def test_train_step_against_reference_autograd(name, wgrad_route):
    """Train-mode forward, the gradient of a fixed projection of both outputs w.r.t. EVERY parameter and the latent, and the
    buffers the forward overwrites, against the reference module -- the checks and bounds of
    tests/test_gpu_train_path.py::test_train_step_against_reference_autograd."""
    g = load_golden(name)
    G, cfg = build(g, train=True)
    cond = cond_to(g["cond"])
    z = g["z"].to(DEV).requires_grad_(True)
    out = G(z, cond, jitter=g["jitter"].to(DEV), noise=g["noise"].to(DEV), **cfg)
    assert out["rgbs"].requires_grad and out["rgbs_render"].requires_grad
    assert rel_err(out["rgbs_render"].detach().cpu(), g["out"]["rgbs_render"]) < 1e-4
    assert rel_err(out["rgbs"].detach().cpu(), g["out"]["rgbs"]) < 2e-4
    loss = (out["rgbs"] * g["p_rgb"].to(DEV)).sum() + (out["rgbs_render"] * g["p_render"].to(DEV)).sum()
    loss.backward()
    got = {n: p.grad for n, p in G.named_parameters()}
    got["__z__"] = z.grad
    for k in g["grad"]:
        assert got.get(k) is not None, f"no gradient for {k}"
    worst, where = grad_errors(got, g["grad"])
    print(f"{name} {wgrad_route}: worst gradient rel err {worst:.2e} ({where})")
    assert worst < 1e-3, (where, worst)
    unused = [n for n, v in got.items() if v is not None and n not in g["grad"] and float(v.abs().max()) > 0]
    assert not unused, unused
    sd = G.state_dict()
    for k, ref in g["buffers_after"].items():
        if ref.is_floating_point():
            assert rel_err(sd[k].cpu(), ref) < 1e-4, k
        else:
            assert torch.equal(sd[k].cpu(), ref), k
    changed = {k for k, v in sd.items() if k in g["state"] and not torch.equal(v.cpu(), g["state"][k])}
    assert changed == set(g["buffers_after"]), changed ^ set(g["buffers_after"])
