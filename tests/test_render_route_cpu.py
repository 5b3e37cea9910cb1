"""Which kernels a render call reaches, on which field engine, and what it draws from the RNG on the way
(lib/generators/map3d_generator.py: Map3DGenerator.render), pinned without a GPU.  A real Map3DGenerator with a real COORDCONCATSIREN
(its capability predicates decide as they do on the device) is driven through the public render() with small CPU tensors; every
leaf that would launch a kernel is a recorder that returns zeros of the right shape, and torch.rand / torch.randn / Tensor.normal_
record the shape they are asked for.  Each case compares the whole log -- stages entered, leaves reached, the engine each ran on,
the noise / background arguments it was handed, every draw in order -- with a model of the route table written out below.
A wrong route would not fail anywhere else: it only runs slower, rounds differently or shifts the RNG stream.

The field tensor has two spellings in the code (differentiable.field_forward and COORDCONCATSIREN.forward): both are logged as
`field(...)` with the `differentiable` flag they amount to."""
import contextlib
import importlib
import itertools
from unittest import mock

import pytest
import torch

from conftest import load_golden

mg = importlib.import_module("3dhumangan_amd.lib.generators.map3d_generator")
impl = importlib.import_module("3dhumangan_amd.lib.implicit_funcitions")
diffmod = importlib.import_module("3dhumangan_amd.lib.generators.differentiable")
vr, smpl = mg.vr, mg.smpl

B, W, H = 1, 2, 1
R = W * H
X2X3 = ("f16x2", "f16x3")
TILE = {"f16x2": 32, "f16x3": 32, "f16x2t": 64, "f16x3t": 64, "f16x1t": 64, "f32": 64}
HIER_DIFF = "hierarchical_sample=True has no differentiable path (no shipped config trains with it)"


class Field(impl.COORDCONCATSIREN):
    """The real module; assignments to `precision` while a render call runs are recorded."""
    armed = False
    assigned = []

    def __setattr__(self, name, value):
        if name == "precision" and Field.armed:
            Field.assigned.append(value)
        super().__setattr__(name, value)


@pytest.fixture(scope="module")
def world():
    g = load_golden("gen_tiny_mixed")
    cfg = dict(g["meta"])
    cfg["neural_field_cls"] = Field
    G = mg.Map3DGenerator(**cfg).eval()
    cond = {k: v[:B] for k, v in g["cond"].items()}
    return G, cond


def case(differentiable=False, grad=False, hier=False, fused=True, train_field="x3", fuse_geo=True, device_pack=True,
         precision="f16x2", S=8, lock=True, sample_dist=None, inject_jitter=True, inject_noise=True, nerf_noise=0, fine=None):
    return dict(locals())


def fused_ok(S, engine):
    t = TILE[engine]
    return (8 <= S <= t and S & (S - 1) == 0) or (S > t and S % t == 0)


def model(c):
    """The route table: -> (route, engine, differentiable) of a call; route None: the call is refused."""
    if c["hier"]:
        return (None, None, None) if c["differentiable"] else ("hierarchical", c["precision"], False)
    # a train-mode forward that nothing records takes the fused render on device-packed weights
    promoted = (c["differentiable"] and not c["grad"] and c["fused"] and c["train_field"] in ("x3", "x2") and c["device_pack"]
                and c["precision"] in X2X3 and fused_ok(c["S"], c["precision"]))
    engine = ("f16x3" if c["train_field"] == "x3" else "f16x2") if promoted else c["precision"]
    diff = c["differentiable"] and not promoted
    can_fuse = c["fused"] and not diff and fused_ok(c["S"], engine)
    if can_fuse and c["fuse_geo"] and engine in X2X3:
        return "fused_geo", engine, diff
    return ("fused" if can_fuse else "unfused"), engine, diff


def camera_draws(sample_dist):
    return {None: [], "uniform": [f"rand({B}, 1)"] * 2, "gaussian": [f"randn({B}, 1)"] * 2,
            "truncated_gaussian": [f"normal_({B}, 1, 4)"] * 2}[sample_dist]


def expected(c):
    route, engine, diff = model(c)
    if route is None:
        return [f"raise {HIER_DIFF}"]
    S, own = c["S"], c["precision"]
    Sf = S if c["fine"] is None else c["fine"]
    noise = "given" if c["inject_noise"] or c["nerf_noise"] != 0 else "none"
    flags = f"noise={noise} clamp=relu last_back=True white_back=True"
    jitter = [] if c["inject_jitter"] else [f"rand({B}, {R}, {S}, 1)"]
    drawn = lambda n: [] if c["inject_noise"] else [f"randn({B}, {R}, {n}, 1)"]
    log = ["stage ray_setup", f"sample_rays S={S}"] + jitter
    if route == "hierarchical":
        field = f"field engine={own} differentiable=False dirs={'none' if c['lock'] else 'given'} scaler=0.5"
        return (log + ["ray_frame_world"] + camera_draws(c["sample_dist"])
                + ["stage geo_features", "get_geo_features", "stage neural_field", field] + drawn(S)
                + ["stage ray_integrate", f"ray_integration S={S} noise={noise} clamp=relu last_back=False white_back=False consume_rng=False",
                   "stage resample", f"sample_pdf n={Sf}"] + ([] if c["inject_noise"] else [f"rand({B * R}, {Sf})"])
                + ["ray_points", "stage geo_features", "get_geo_features", "stage neural_field", field, "stage resample", "merge_samples"]
                + drawn(S + Sf) + ["stage ray_integrate", f"ray_integration S={S + Sf} {flags} consume_rng=False"])
    log += camera_draws(c["sample_dist"]) + drawn(S) + ["stage geo_features"]
    log += ["vertex_inverse_transforms", "nearest_vertex"] if route == "fused_geo" else ["get_geo_features"]
    dirs = "none" if c["lock"] else "given"
    if not c["lock"]:
        log.append("ray_directions_world")
    if route == "fused_geo":
        return log + ["stage render_fused", f"render_geo engine={engine} S={S} dirs={dirs} scaler=0.5 {flags}"]
    if route == "fused":
        return log + ["stage render_fused", f"render engine={engine} S={S} dirs={dirs} scaler=0.5 {flags}"]
    return log + ["stage neural_field", f"field engine={own} differentiable={diff} dirs={dirs} scaler=0.5",
                  "stage ray_integrate", f"ray_integration S={S} {flags} consume_rng=False"]


def drive(G, cond, c):
    """G.render(...) for the case on recording leaves -> the log."""
    nf, S, F = G.neural_field, c["S"], G.feature_dim
    Sf = S if c["fine"] is None else c["fine"]
    log = []
    zeros = torch.zeros
    none = lambda t: "none" if t is None else "given"

    def draw(name):
        def rec(*size, **kw):
            size = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
            log.append(f"{name}{size}")
            return zeros(size)
        return rec

    def normal_(t, *a, **k):
        log.append(f"normal_{tuple(t.shape)}")
        return t

    def sample_rays(focals, scales, c2w, num_steps, resolution, ray_start, ray_end, jitter=None, perturb=True):
        assert perturb and tuple(resolution) == (W, H)
        log.append(f"sample_rays S={num_steps}")
        if jitter is None:
            torch.rand((B, R, num_steps, 1))                         # where the leaf draws it
        return zeros(B, R * num_steps, 3), zeros(B, R, num_steps, 1)

    def integrated(n):
        return zeros(B, R, F + 3), zeros(B, R, 1), zeros(B, R, n, 1)

    def flags(k):
        return (f"noise={none(k.get('noise'))} clamp={k.get('clamp_mode')} last_back={k.get('last_back', False)} "
                f"white_back={k.get('white_back', False)}")

    def ray_integration(field, z_vals, **k):
        assert k.pop("noise_std") == 0
        log.append(f"ray_integration S={field.shape[2]} {flags(k)} consume_rng={k['consume_rng']}")
        return integrated(field.shape[2])

    def sample_pdf(bins, weights, n, det=False, eps=1e-5, u=None):
        log.append(f"sample_pdf n={n}")
        if u is None:
            torch.rand(weights.shape[0], n)                          # where the leaf draws it
        return zeros(weights.shape[0], n)

    def leaf(name, result):
        def rec(*a, **k):
            log.append(name)
            return result(*a, **k)
        return rec

    def field(engine, differentiable, pts, dirs, scaler):
        log.append(f"field engine={engine} differentiable={differentiable} dirs={none(dirs)} scaler={scaler}")
        return zeros(B, pts.shape[1], F + 4)

    def nf_forward(pts, fr, ph, geo, dirs, input_scaler=1., **k):
        return field(k.get("precision", nf.precision), bool(k["differentiable"]), pts, dirs, input_scaler)

    def field_forward(nf_, pts, fr, ph, geo, dirs, input_scaler=1.):
        return field(nf_.precision, True, pts, dirs, input_scaler)

    def render(pts, fr, ph, geo, dirs, z_vals, num_steps, **k):
        log.append(f"render engine={k.get('precision', nf.precision)} S={num_steps} dirs={none(dirs)} scaler={k['input_scaler']} {flags(k)}")
        return integrated(num_steps)

    def render_geo(pts, fr, ph, idx, sk, vt, tv, vik, dirs, z_vals, num_steps, **k):
        assert k.pop("legacy_mode") == G.legacy_mode
        log.append(f"render_geo engine={k.get('precision', nf.precision)} S={num_steps} dirs={none(dirs)} scaler={k['input_scaler']} {flags(k)}")
        return integrated(num_steps)

    @contextlib.contextmanager
    def stage(owner, name):
        assert owner is G
        log.append(f"stage {name}")
        yield

    V = cond["vertices"].shape[1]
    nf.precision, nf.device_pack, G.train_field, G.fuse_geo, G.side_length = c["precision"], c["device_pack"], c["train_field"], c["fuse_geo"], 4.0
    given = lambda *shape: zeros(*shape) + 0.25
    kw = dict(hierarchical_sample=c["hier"], sample_dist=c["sample_dist"], lock_view_dependence=c["lock"], fused=c["fused"],
              differentiable=c["differentiable"], nerf_noise=c["nerf_noise"], clamp_mode="relu", last_back=True, white_back=True,
              jitter=given(B, R, S, 1) if c["inject_jitter"] else None)
    if c["inject_noise"]:
        kw["noise"] = given(B, R, S + Sf if c["hier"] else S, 1)
        if c["hier"]:
            kw.update(noise_coarse=given(B, R, S, 1), fine_u=given(B * R, Sf))
    with contextlib.ExitStack() as st:
        for obj, name, value in (
                (vr, "sample_rays", sample_rays), (vr, "ray_integration", ray_integration), (vr, "sample_pdf", sample_pdf),
                (vr, "ray_directions_world", leaf("ray_directions_world", lambda f, m, res, n: zeros(B, R * n, 3))),
                (vr, "ray_frame_world", leaf("ray_frame_world", lambda f, m, res: (zeros(B, 3), zeros(B, R, 3)))),
                (vr, "ray_points", leaf("ray_points", lambda o, d, z: zeros(B, R * z.shape[2], 3))),
                (vr, "merge_samples", leaf("merge_samples", lambda f, co, fz, z: (zeros(B, R, f.shape[2] + co.shape[2], F + 4),
                                                                                   zeros(B, R, f.shape[2] + co.shape[2], 1)))),
                (smpl, "nearest_vertex", leaf("nearest_vertex", lambda p, v, ray_shape=None: zeros(B, p.shape[1], dtype=torch.int32))),
                (smpl, "vertex_inverse_transforms", leaf("vertex_inverse_transforms", lambda fk, lbs: zeros(B, V, 16))),
                (G, "get_geo_features", leaf("get_geo_features", lambda p, *a, **k: zeros(B, p.shape[1], 31))),
                (nf, "render", render), (nf, "render_geo", render_geo), (nf, "forward", nf_forward),
                *((m, "field_forward", field_forward) for m in (mg, diffmod) if hasattr(m, "field_forward")),     # wherever it is bound
                (mg, "stage", stage),
                (torch, "rand", draw("rand")), (torch, "randn", draw("randn")), (torch.Tensor, "normal_", normal_)):
            st.enter_context(mock.patch.object(obj, name, value))
        st.enter_context(torch.enable_grad() if c["grad"] else torch.no_grad())
        st.enter_context(mock.patch.object(Field, "armed", True))
        del Field.assigned[:]
        try:
            out = G.render(zeros(B, 4 * G.hidden_dim), zeros(B, 4 * G.hidden_dim), cond, W, H, -0.5, 0.5, S, c["fine"], **kw)
        except NotImplementedError as e:
            log.append(f"raise {e}")
        else:
            rgb, fmap, depths, weights, last = out
            assert rgb.shape == (B, 3, H, W) and fmap.shape == (B, R, F) and depths.shape == (B, R, 1) and last is None
            assert weights.shape == (B, R, S + Sf if c["hier"] else S, 1)
    assert nf.precision == c["precision"] and Field.assigned == []         # the engine of a call is an argument, never a swap
    return log


def pruned_cases():
    """Every 23rd point of the product of what the route depends on (23 is coprime to every factor, so each value of each factor
    and most pairs come up), what only the draws and arguments depend on cycling along; then the promoted calls in full ..."""
    core = itertools.product((False, True), (False, True), (False, True), (True, False), ("x3", "x2", "off"), (True, False),
                             (True, False), tuple(TILE), (8, 16, 24, 32, 64, 96, 128))
    dists = (None, "uniform", "gaussian", "truncated_gaussian")
    out = []
    for k, (d, g, h, f, tf, fg, dp, p, S) in enumerate(itertools.islice(core, 0, None, 23)):
        out.append(case(d, g, h, f, tf, fg, dp, p, S, lock=k % 2 == 0, sample_dist=dists[k // 2 % 4], inject_jitter=k // 8 % 2 == 0,
                        inject_noise=k // 16 % 2 == 0, nerf_noise=(0, 0.5)[k // 32 % 2], fine=(None, 8)[k // 64 % 2]))
    for k, (p, tf, fg, S) in enumerate(itertools.product(X2X3, ("x3", "x2"), (True, False), (8, 24, 32, 64, 96))):
        out.append(case(True, False, False, True, tf, fg, True, p, S, lock=k % 2 == 1, sample_dist=dists[k % 4],
                        inject_jitter=k % 3 == 0, inject_noise=k % 5 < 2, nerf_noise=(0.5, 0)[k % 2]))
    # ... and each condition of the promotion failing on its own
    for k, (p, tf, broken) in enumerate(itertools.product(X2X3, ("x3", "x2"), (
            dict(grad=True), dict(fused=False), dict(train_field="off"), dict(device_pack=False), dict(precision="f16x2t"),
            dict(precision="f32"), dict(S=24)))):
        out.append(case(**dict(dict(differentiable=True, train_field=tf, precision=p, S=(8, 64)[k % 2], inject_noise=k % 3 == 0), **broken)))
    return out


CASES = pruned_cases()


def case_id(c):
    return "-".join(f"{k}={v}" for k, v in c.items() if v != case()[k]) or "default"


def test_the_sample_covers_every_route():
    routes = {(model(c)[0], model(c)[1] not in (None, c["precision"])) for c in CASES}
    assert routes == {(None, False), ("hierarchical", False), ("fused_geo", False), ("fused_geo", True), ("fused", False),
                      ("fused", True), ("unfused", False)}
    assert 300 <= len(CASES) <= 500


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_route(world, c):
    G, cond = world
    log = drive(G, cond, c)
    assert log == expected(c)
    # the routing function on its own, on plain values, says what the driven call did
    nf = G.neural_field
    nf.precision = c["precision"]
    ask = lambda: mg._render_route(c["differentiable"], c["grad"], c["hier"], c["fused"], c["train_field"], c["fuse_geo"], c["device_pack"],
                                   c["precision"], c["S"], nf.fused_supported, nf.render_geo_supported)
    if log[0].startswith("raise"):
        with pytest.raises(NotImplementedError, match="has no differentiable path"):
            ask()
        return
    route, engine, differentiable = ask()
    ran = [e.split() for e in log if e.split()[0] in ("render_geo", "render", "field")]
    assert route == ("hierarchical" if "ray_frame_world" in log else {"render_geo": "fused_geo", "render": "fused", "field": "unfused"}[ran[-1][0]])
    assert {e[1] for e in ran} == {f"engine={engine}"}
    assert differentiable == (f"differentiable=True" in ran[-1])


def test_patches_are_undone(world):
    G, cond = world
    drive(G, cond, case(sample_dist="truncated_gaussian", inject_noise=False))
    assert torch.rand(2).shape == (2,) and "forward" not in vars(G.neural_field) and "render" not in vars(G.neural_field)
    assert "normal_" not in vars(torch.Tensor) and not Field.armed
