"""Map3DGenerator.density_grid / .extract_mesh and the app's `--save mesh`, on the tiny fixture generator (gen_tiny_mixed: two
bodies in different poses, conditioned weights).

The density is held to the bar tests/_field_arithmetic.py derives for the engine in use, on the grid's own points: the grid is
entered as a field case of its own (its points, the oracle's geometry features of them, the generator's own frequencies and
phases) and ladder_of() gives the bars of the density group exactly as for the cases of tests/test_gpu_field_ladder.py --
    f16x3 (the x3 class) against float64:  (smallest single-defect error D1 / D2 in the contractions the density sees) / 3
    f16x2 (the default at this width) against float64:  3 x the healthy x2 emulation's error,
                                     against the x2 emulation:  (smallest distance of a one-layer dead fp6 product) / 3
No constant of this file enters a bar."""
import importlib
import math

import numpy as np
import pytest
import torch

import _field_arithmetic as A
import h3d_oracle as O
from _isosurface_reference import parse_ply
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
gens = importlib.import_module("3dhumangan_amd.lib.generators")
impl = importlib.import_module("3dhumangan_amd.lib.implicit_funcitions")
iso = importlib.import_module("3dhumangan_amd.lib.components.isosurface")
DEV = "cuda"
MESH_KEYS = ("skeletons_xyz", "vertices", "tpose_vertices", "fk_matrices", "lbs_weights")
GRIDS = {"r12": dict(resolution=12), "r7-chunked": dict(resolution=7, max_points=100)}
_G, _GRID, _CASE = {}, {}, {}


def fixture():
    """-> (generator on the device, its config, latent [2, L], the five mesh conditions) -- built once"""
    if not _G:
        g = load_golden("gen_tiny_mixed")
        cfg = dict(g["meta"])
        cfg["neural_field_cls"] = impl.COORDCONCATSIREN
        G = gens.Map3DGenerator(**cfg)
        G.load_state_dict(g["state"], strict=True)
        G = G.to(DEV).eval()
        G.set_device(DEV)
        _G.update(G=G, cfg=cfg, z=g["z"].to(DEV), cond={k: g["cond"][k].to(DEV) for k in MESH_KEYS}, state=g["state"], cpu_cond=g["cond"])
    return _G["G"], _G["cfg"], _G["z"], _G["cond"]


def grid(name, precision=None, **override):
    """density_grid of the fixture for one entry of GRIDS and one engine -> (sigma, origin, spacing), run once"""
    key = (name, precision, tuple(sorted(override.items())))
    if key not in _GRID:
        G, cfg, z, cond = fixture()
        _GRID[key] = G.density_grid(z, cond, precision=precision, **{**GRIDS[name], **override}, **cfg)
    return _GRID[key]


def grid_points(origin, spacing, shape):
    """node (i, j, k) -> origin + spacing * (i, j, k), node id = (i Ny + j) Nz + k, fp32 as density_grid states it"""
    Nx, Ny, Nz = shape
    n = torch.arange(Nx * Ny * Nz)
    ijk = torch.stack([n // (Ny * Nz), (n // Nz) % Ny, n % Nz], dim=-1).float()
    return origin.cpu()[:, None] + spacing.cpu()[:, None] * ijk[None]


def arithmetic_case(name):
    """The grid as a case of tests/_field_arithmetic.py -> (case, float64 density, x2-emulation density, bars of the density)"""
    if name not in _CASE:
        G, cfg, z, cond = fixture()
        sigma, origin, spacing = grid(name)
        pts = grid_points(origin, spacing, sigma.shape[1:])
        c = _G["cpu_cond"]
        geo = O.geo_features(pts, c["skeletons_xyz"], c["vertices"], c["tpose_vertices"], c["fk_matrices"], c["lbs_weights"],
                             cfg.get("legacy_mode", False))
        with torch.no_grad():
            fr, ph, _ = G._mapping(z, cfg)
        dirs = torch.zeros_like(pts)
        dirs[..., 2] = -1                                  # ray_directions=None is the locked direction; the density does not read it
        case = A.Case(f"density-grid-{name}", "field", cfg["hidden_dim"], cfg["feature_dim"], seed=-1, gseed=-GRIDS[name]["resolution"],
                      N=pts.shape[1])
        A._INPUTS[case.input_key] = dict(state={k: v for k, v in _G["state"].items() if k.startswith("neural_field.")}, net=None,
                                         pts=pts, geo=geo, dirs=dirs, freq=fr.cpu(), phase=ph.cpu(), scaler=2.0 / G.side_length)
        L, out = A.ladder_of(case), A.outputs_of(case)
        _CASE[name] = (case, {"exact": out["exact"][..., -1:], "x2": out["x2"][..., -1:]}, {a: L["bars"][a]["sigma"] for a in L["bars"]})
    return _CASE[name]


@pytest.mark.parametrize("precision", ["f16x3", None])
@pytest.mark.parametrize("name", list(GRIDS))
def test_density_meets_the_bar_of_its_engine(name, precision):
    G, cfg, z, cond = fixture()
    engine = G.neural_field.precision if precision is None else precision
    assert A.engine_class(engine) == ("x3" if precision else "x2")          # one run per engine class
    case, ref, bars = arithmetic_case(name)
    sigma, origin, spacing = grid(name, precision)
    assert sigma.dtype == torch.float32 and sigma.dim() == 4 and sigma.shape[0] == 2
    got = sigma.reshape(2, -1, 1).cpu()
    for assertion, against in A.assertions_for(engine):
        err = rel_err(got.double(), ref[against])
        print(f"{name} {engine} {assertion}: density error {err:.3e} bar {bars[assertion]:.3e}")
        assert err < bars[assertion], (assertion, err, bars[assertion])


@pytest.mark.parametrize("precision", ["f16x3", None])
def test_chunked_equals_unchunked_within_the_bar(precision):
    """resolution 7 is 7 x 7 x 5 = 245 points per item: max_points=100 makes chunks of 50 per item, the last one ragged (45)"""
    G, cfg, z, cond = fixture()
    engine = G.neural_field.precision if precision is None else precision
    _, _, bars = arithmetic_case("r7-chunked")
    chunked, o1, s1 = grid("r7-chunked", precision)
    whole, o2, s2 = grid("r7-chunked", precision, max_points=2 ** 21)
    assert chunked.shape == whole.shape and chunked.shape[1] * chunked.shape[2] * chunked.shape[3] % 50 != 0
    assert torch.equal(o1, o2) and torch.equal(s1, s2)
    err, bar = rel_err(chunked.cpu().double(), whole.cpu().double()), min(bars[a] for a, _ in A.assertions_for(engine))
    print(f"{engine}: chunked vs unchunked {err:.3e} bar {bar:.3e}")
    assert err < bar


@pytest.mark.parametrize("name", list(GRIDS))
def test_grid_geometry(name):
    G, cfg, z, cond = fixture()
    sigma, origin, spacing = grid(name)
    resolution, margin = GRIDS[name]["resolution"], 0.1
    assert origin.shape == (2, 3) and spacing.shape == (2, 3)
    assert torch.equal(spacing[:, 0], spacing[:, 1]) and torch.equal(spacing[:, 0], spacing[:, 2])       # cubic voxels
    v = cond["vertices"].double()
    lo, hi = v.amin(dim=1), v.amax(dim=1)
    longest = (hi - lo).amax(dim=1, keepdim=True)
    shape = torch.tensor(sigma.shape[1:], device=DEV)
    top = origin.double() + spacing.double() * (shape - 1)
    slack = 1e-6 * longest                                 # the frame is rounded to fp32
    assert (origin.double() <= lo - margin * longest + slack).all() and (top >= hi + margin * longest - slack).all()
    assert max(sigma.shape[1:]) == resolution              # `resolution` nodes along the longest axis of the grown box
    assert torch.allclose(spacing[:, 0].double() * (resolution - 1), (longest * (1 + 2 * margin))[:, 0], rtol=1e-6)
    # the two bodies differ and share the node counts: each item alone asks for no more nodes than the batch, per axis, and the
    # batch takes the larger of the two
    alone = [G.density_grid(z[b:b + 1], {k: t[b:b + 1] for k, t in cond.items()}, **GRIDS[name], **cfg) for b in range(2)]
    assert not torch.equal(cond["vertices"][0], cond["vertices"][1])
    for axis in range(3):
        assert sigma.shape[1 + axis] == max(a[0].shape[1 + axis] for a in alone)
    for b, (s, o, sp) in enumerate(alone):
        assert torch.equal(o[0], origin[b]) and torch.equal(sp[0], spacing[b])


def test_only_the_mesh_conditions_are_read():
    G, cfg, z, cond = fixture()
    assert set(cond) == set(MESH_KEYS) == set(G.MESH_CONDITIONS)       # no camera, no intrinsics: the fixture passes five entries
    with pytest.raises(importlib.import_module("3dhumangan_amd._lib").H3DError):
        G.density_grid(z.cpu(), cond, resolution=7, **cfg)


@pytest.mark.parametrize("b", [0, 1])
def test_extract_mesh_is_the_iso_surface_of_the_grid(b):
    G, cfg, z, cond = fixture()
    body = {k: t[b:b + 1] for k, t in cond.items()}
    sigma, origin, spacing = G.density_grid(z[b:b + 1], body, resolution=12, **cfg)
    level = float(sigma[0].median())                       # a surface exists whatever the weights are
    (vertices, faces), = G.extract_mesh(z[b:b + 1], body, level=level, resolution=12, **cfg)
    v0, f0 = iso.marching_tetrahedra(sigma[0], level, origin[0].tolist(), spacing[0].tolist())
    assert len(faces) > 0 and torch.equal(vertices, v0) and torch.equal(faces, f0)
    assert vertices.dtype == torch.float32 and faces.dtype == torch.int32
    top = origin[0] + spacing[0] * (torch.tensor(sigma.shape[1:], device=DEV) - 1)
    ulp = 2.0 ** -22 * float(torch.maximum(origin[0].abs(), top.abs()).max())
    assert (vertices >= origin[0] - ulp).all() and (vertices <= top + ulp).all()
    assert int(faces.min()) >= 0 and int(faces.max()) < len(vertices)
    # the whole batch at once: one mesh per item (on the batch's shared grid, which may be larger than the item's own)
    both = G.extract_mesh(z, cond, level=level, resolution=12, **cfg)
    assert len(both) == 2 and all(m[0].shape[1] == 3 and m[1].shape[1] == 3 for m in both)


def test_default_level_and_refusals():
    G, cfg, z, cond = fixture()
    # ln 2 * num_steps / (ray_end - ray_start); with the fixture's 8 steps it lies above every density of these weights (an empty
    # mesh), with one step it lies inside their range
    sigma, origin, spacing = grid("r12")
    for steps, empty in ((cfg["num_steps"], True), (1, False)):
        want = math.log(2.0) * steps / (cfg["ray_end"] - cfg["ray_start"])
        v0, f0 = iso.marching_tetrahedra(sigma[0], want, origin[0].tolist(), spacing[0].tolist())
        meshes = G.extract_mesh(z, cond, resolution=12, **dict(cfg, num_steps=steps))
        assert (len(f0) == 0) == empty and tuple(meshes[0][0].shape[1:]) == (3,) and tuple(meshes[0][1].shape[1:]) == (3,)
        assert torch.equal(meshes[0][0], v0) and torch.equal(meshes[0][1], f0)
    with pytest.raises(NotImplementedError, match="clamp_mode='softplus'"):
        G.extract_mesh(z, cond, resolution=7, **dict(cfg, clamp_mode="softplus"))


def test_truncation_and_seeds():
    G, cfg, z, cond = fixture()
    g = load_golden("gen_tiny_mixed")
    avg = tuple(g["avg"][k].to(DEV) for k in ("z", "freq", "phase", "styles"))
    plain, _, _ = grid("r7-chunked")
    truncated, _, _ = G.density_grid(z, cond, truncation_psi=0.7, avg_latent=avg, **GRIDS["r7-chunked"], **cfg)
    assert plain.shape == truncated.shape and not torch.equal(plain, truncated)
    # psi = 1 never looks at the mean; psi = 0 is the mean's field whatever the latent is
    same, _, _ = G.density_grid(z, cond, truncation_psi=1.0, avg_latent=avg, **GRIDS["r7-chunked"], **cfg)
    assert torch.equal(same, plain)
    mean_a, _, _ = G.density_grid(z, cond, truncation_psi=0.0, avg_latent=avg, resolution=7, **cfg)
    mean_b, _, _ = G.density_grid(torch.flip(z, dims=(1,)), cond, truncation_psi=0.0, avg_latent=avg, resolution=7, **cfg)
    assert torch.equal(mean_a, mean_b)
    app = importlib.import_module("3dhumangan_amd.apps.sample_from_generator")
    level = float(plain[0].median())
    # equal seeds, equal meshes; another seed, another mesh -- with the latent fed to the field (the fixture's own config feeds it
    # zeros: neural_field_latent_input=False, where every seed has the same body)
    fed = dict(cfg, neural_field_latent_input=True)
    runs = []
    for seed in (4, 4, 5):
        latent = app.latent_for_seed(seed, cfg["latent_dim"]).to(DEV).expand(2, -1).contiguous()
        runs.append(G.extract_mesh(latent, cond, level=level, resolution=7, **fed))
    for (va, fa), (vb, fb) in zip(runs[0], runs[1]):
        assert torch.equal(va, vb) and torch.equal(fa, fb)
    assert not (runs[0][0][0].shape == runs[2][0][0].shape and torch.equal(runs[0][0][0], runs[2][0][0]))


def test_app_saves_one_mesh_per_pose(tmp_path):
    app = importlib.import_module("3dhumangan_amd.apps.sample_from_generator")
    configs = importlib.import_module("3dhumangan_amd.configs")
    g = load_golden("gen_tiny_mixed")
    cfg = dict(g["meta"])
    cfg.update(neural_field_cls="COORDCONCATSIREN", name="tiny_mesh")
    configs.TINY_MESH = cfg
    ckpt = str(tmp_path / "tiny_state_dict.pth")
    torch.save(g["state"], ckpt)
    level = -2.0                       # inside the density range of the fixture's weights (the derived default lies above it)
    out_dir = app.main(["--config", "TINY_MESH", "--checkpoint", ckpt, "--dataset_length", "4", "--pose-sequence", "synthetic", "--n_poses", "2",
                        "--seeds", "3", "--save", "mesh", "--mesh_resolution", "16", "--mesh_level", str(level), "--output_dir", str(tmp_path)])
    files = [f"{out_dir}/003_mesh_{i:03d}.ply" for i in range(2)]
    parsed = [parse_ply(f) for f in files]
    # the same thing by hand: the app's config, its seed -> latent convention, one extract_mesh call per pose
    G, base, _, _ = fixture()
    G.avg_latent = None
    run = dict(base, truncation_psi=0.7, cache_avg_latent=True, dataset_length=4)
    sequence, _ = app.load_pose_sequence(None, "synthetic", torch.device(DEV), 2)
    for i, (v, f) in enumerate(parsed):
        latent = app.latent_for_seed(3, run["latent_dim"]).to(DEV)
        body = {k: sequence[k][i:i + 1].to(DEV) for k in MESH_KEYS}
        (v0, f0), = G.extract_mesh(latent, body, level=level, resolution=16, **run)
        assert len(f) > 0 and (len(v), len(f)) == (len(v0), len(f0))
        assert np.array_equal(v, v0.cpu().numpy()) and np.array_equal(f, f0.cpu().numpy())
        assert f.min() >= 0 and f.max() < len(v)
    assert not (parsed[0][0].shape == parsed[1][0].shape and np.array_equal(parsed[0][0], parsed[1][0]))      # two poses, two bodies
