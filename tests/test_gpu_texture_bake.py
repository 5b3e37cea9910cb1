"""h3d_mesh_bake_texture against the float64 restatement (tests/_texture_bake_reference.py, itself checked by
tests/test_texture_bake_cpu.py) on every texel, owned and unowned; then the generator and the app, held to the kernel bit for bit.

Bars, the convention of tests/test_gpu_mesh_attributes.py.  No constant of this file enters one: bar = 8 x max |restatement in float32 -
restatement in float64| on the case's own inputs, and not less than 4 * 2^-23 x max |float64 output|, for coverage, numerator and -- where
the reference coverage is at least 0.1 -- colour.  The maximum needs enough texels to be the size of the rounding and not one draw of
it: a case that owns fewer than 257 texels takes the bars of the (128, 50) case on the same views, which owns 2304.  A lost view or
vertex is of order 0.1 - 1.  Measured errors and bars are printed and stand in DESIGN 4.5f."""
import importlib
import math

import numpy as np
import pytest
import torch

import _mesh_rig_reference as RIG
import _texture_bake_reference as R
from _mesh_attributes_reference import parse_attributed_ply
from conftest import load_golden
from test_texture_bake_cpu import glb_image

pytestmark = pytest.mark.gpu
mesh_texture = importlib.import_module("3dhumangan_amd.lib.components.mesh_texture")
mesh_color = importlib.import_module("3dhumangan_amd.lib.components.mesh_color")
DEV = "cuda"
f32, f64 = np.float32, np.float64
FILL, EPS, POWER = 0.25, 1e-3, 2
GRID = (64, 64, 128, 128)
# render grid -> depth tolerance: the few rays of the tiny grids pass the sphere, so their depth maps hold the far value (6 units
# from the camera, the sphere's front is at 3) and only a tent that wide reaches the mesh.  Checked on the CPU: with 6.0 the reference
# sees 98 % of the owned texels of both, 1191 and 1630 of 2304 with coverage >= 0.1 (with 3.0: none and 1407)
TOLERANCE = {GRID: 0.05, (2, 2, 2, 2): 6.0, (5, 3, 12, 7): 6.0}
_CACHE = {}


def bar_of(low, high):
    return max(8.0 * float(np.abs(low.astype(f64) - high).max()), 4.0 * 2.0 ** -23 * float(np.abs(high).max()))


def dev(a, dtype=f32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def scene_of(K, grid):
    """the detailed sphere scene in the kernel's format: every number format sees the same fp32 inputs"""
    key = ("scene", K, grid)
    if key not in _CACHE:
        s = dict(R.detailed_scene(K, *grid))
        for name in ("images", "depths", "focals", "cam2world"):
            s[name] = s[name].astype(f32)
        _CACHE[key] = s
    return _CACHE[key]


def mesh_of(T, scene, zero_normals=False):
    """the first T triangles of the 128-triangle sphere mesh, or of the 512-triangle one; T = 513: that one and a degenerate triangle
    with a repeated vertex.  zero_normals: the three vertices of triangle 5 have the normal (0,0,0)."""
    vertices, normals, faces = R.octa_sphere(2 if T <= 128 else 3, scene["centre"], scene["radius"])
    if T == 513:
        faces = np.concatenate([faces, [[7, 7, 100]]]).astype(np.int32)
    normals = normals.copy()
    if zero_normals:
        normals[faces[5]] = 0.0
    return vertices.astype(f32), normals.astype(f32), np.ascontiguousarray(faces[:T])


def reference(T, S, K, grid, zero_normals=False):
    """-> dict per dtype of (texture, coverage, numerator), and the owner map -- computed once per case and shared"""
    key = ("ref", T, S, K, grid, zero_normals)
    if key not in _CACHE:
        s = scene_of(K, grid)
        vertices, normals, faces = mesh_of(T, s, zero_normals)
        out = {}
        for dtype in (f32, f64):
            texture, coverage, owner = R.bake(vertices, faces, normals, s, TOLERANCE[grid], S, POWER, FILL, EPS, dtype)
            numerator = texture.astype(f64) * (coverage.astype(f64) + EPS)[..., None] - EPS * FILL
            out[dtype] = (texture, coverage, numerator)
        out["owner"] = owner
        _CACHE[key] = out
    return _CACHE[key]


def bars(ref):
    own = ref["owner"] >= 0
    (t32, c32, n32), (t64, c64, n64) = ref[f32], ref[f64]
    seen = own & (c64 >= 0.1)
    return {"coverage": bar_of(c32[own], c64[own]), "numerator": bar_of(n32[own], n64[own]),
            "colour": bar_of(t32[seen], t64[seen]) if seen.any() else 0.0}


def run_kernel(T, S, K, grid, zero_normals=False, fill=FILL, change=None):
    s = scene_of(K, grid)
    vertices, normals, faces = mesh_of(T, s, zero_normals)
    args = dict(vertices=dev(vertices), faces=dev(faces, np.int32), normals=dev(normals), images=dev(s["images"]), depths=dev(s["depths"]),
                focals=dev(s["focals"]), scales=dev(s["scales"]), cam2world=dev(s["cam2world"]))
    if change:
        change(args)
    return mesh_texture.bake_texture(depth_tolerance=TOLERANCE[grid], size=S, normal_power=POWER, fill=fill, eps=EPS, **args)


CASES = [(1, 4, 1, GRID, False), (2, 4, 5, GRID, False), (3, 8, 1, GRID, False), (7, 9, 5, GRID, False), (8, 8, 1, GRID, False),
         (128, 50, 5, GRID, False), (513, 100, 1, GRID, False), (512, 256, 5, GRID, False), (128, 50, 1, GRID, False),
         (128, 50, 5, GRID, True), (128, 50, 5, (2, 2, 2, 2), False), (128, 50, 5, (5, 3, 12, 7), False)]


@pytest.mark.parametrize("T,S,K,grid,zero_normals", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_bake_against_the_restatement(T, S, K, grid, zero_normals):
    ref = reference(T, S, K, grid, zero_normals)
    owner, (t64, c64, n64) = ref["owner"], ref[f64]
    own = owner >= 0
    bar = bars(ref if own.sum() >= 257 else reference(128, 50, K, grid))
    texture, coverage = run_kernel(T, S, K, grid, zero_normals)
    assert texture.shape == (S, S, 3) and coverage.shape == (S, S) and texture.dtype == coverage.dtype == torch.float32
    texture, coverage = texture.cpu().numpy(), coverage.cpu().numpy()
    # unowned texels: the fill colour itself and coverage 0
    assert (texture[~own] == f32(FILL)).all() and (coverage[~own] == 0).all()
    texture, coverage = texture.astype(f64), coverage.astype(f64)
    numerator = texture * (coverage + EPS)[..., None] - EPS * FILL
    seen = own & (c64 >= 0.1)
    cov_err, num_err = np.abs(coverage - c64)[own].max(), np.abs(numerator - n64)[own].max()
    col_err = np.abs(texture - t64)[seen].max(initial=0.0)
    print(f"bake T={T} S={S} K={K} grid={grid} zero_normals={zero_normals}: {int(own.sum())} owned texels, {int((own & (c64 > 0)).sum())} "
          f"seen, {int(seen.sum())} with coverage >= 0.1 (max {c64.max():.2f}); coverage err {cov_err:.2e} bar {bar['coverage']:.2e}; "
          f"numerator err {num_err:.2e} bar {bar['numerator']:.2e}; colour err {col_err:.2e} bar {bar['colour']:.2e}")
    if grid == GRID and T >= 128:
        assert (own & (c64 > 0)).sum() >= own.sum() / 16         # the case is not empty
    if zero_normals:
        assert (coverage[owner == 5] == 0).all() and np.allclose(texture[owner == 5], FILL, rtol=1e-6, atol=0)
    assert cov_err <= bar["coverage"] and num_err <= bar["numerator"] and col_err <= bar["colour"]


@pytest.mark.parametrize("T,S,K", [(128, 50, 5), (513, 100, 1)])
def test_corner_texels_carry_the_vertex_colours(T, S, K):
    """the texel under a corner has one-hot barycentrics: it is project_colors at that vertex (the sphere's normals are unit vectors
    up to their rounding to fp32, which the texel's normalisation undoes), within the bars of the case"""
    ref = reference(T, S, K, GRID)
    bar = bars(ref)
    s = scene_of(K, GRID)
    vertices, normals, faces = mesh_of(T, s)
    texture, coverage = (t.cpu().numpy().astype(f64) for t in run_kernel(T, S, K, GRID))
    unit = torch.nn.functional.normalize(dev(normals), dim=1)
    colors, seen = mesh_color.project_colors(dev(vertices), unit, dev(s["images"]), dev(s["depths"]), dev(s["focals"]),
                                             dev(s["scales"]), dev(s["cam2world"]), TOLERANCE[GRID], POWER, FILL, EPS)
    colors, seen = colors.cpu().numpy().astype(f64), seen.cpu().numpy().astype(f64)
    centre = np.round(R.uvs(T, S) * S - 0.5).astype(int)
    q, r = centre[..., 0], centre[..., 1]
    assert np.array_equal(ref["owner"][r, q], np.repeat(np.arange(T)[:, None], 3, axis=1))
    cov_err = np.abs(coverage[r, q] - seen[faces]).max()
    well = seen[faces] >= 0.1
    col_err = np.abs(texture[r, q] - colors[faces])[well].max()
    print(f"corners T={T} S={S} K={K}: coverage err {cov_err:.2e} bar {bar['coverage']:.2e}; colour err {col_err:.2e} bar {bar['colour']:.2e} "
          f"on {int(well.sum())} of {well.size} corners")
    assert well.sum() >= well.size // 16
    assert cov_err <= bar["coverage"] and col_err <= bar["colour"]


def test_twice_noncontiguous_nonfinite_empty_and_wrong_indices():
    T, S, K, fill = 128, 50, 5, -0.5
    a = run_kernel(T, S, K, GRID, fill=fill)
    b = run_kernel(T, S, K, GRID, fill=fill)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert float(a[1].max()) > 0.5

    def strided(args):
        images = args["images"]
        args["images"] = images.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)          # channels-last: copied
        args["faces"] = torch.stack([args["faces"], args["faces"]], dim=2)[:, :, 0]          # stride 2
        args["vertices"] = args["vertices"].t().contiguous().t()
        assert not any(args[k].is_contiguous() for k in ("images", "faces", "vertices"))

    c = run_kernel(T, S, K, GRID, fill=fill, change=strided)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    # a NaN vertex: coverage 0 and the fill colour on the texels of its triangles, the same bits on every other texel
    s = scene_of(K, GRID)
    _, _, faces = mesh_of(T, s)
    vertex = int(faces[9, 1])

    def poisoned(args):
        args["vertices"][vertex, 1] = float("nan")

    texture, coverage = run_kernel(T, S, K, GRID, fill=fill, change=poisoned)
    owner = reference(T, S, K, GRID)["owner"]
    hit = torch.as_tensor(np.isin(owner, np.flatnonzero((faces == vertex).any(axis=1)))).to(DEV)
    assert int(hit.sum()) >= 4 * 15 and float(a[1][hit].max()) > 0
    assert (coverage[hit] == 0).all() and torch.allclose(texture[hit], torch.full_like(texture[hit], fill), rtol=1e-6, atol=0)
    assert torch.equal(texture[~hit], a[0][~hit]) and torch.equal(coverage[~hit], a[1][~hit])
    # no triangles: everything is the fill colour
    texture, coverage = run_kernel(T, S, K, GRID, fill=fill, change=lambda args: args.update(faces=args["faces"][:0]))
    assert texture.shape == (S, S, 3) and (texture == fill).all() and (coverage == 0).all()

    # face indices out of range are clamped into it: a wrong texel, no fault and no error
    def wrong(args):
        args["faces"][3] = torch.tensor([-7, 2 ** 31 - 1, 10 ** 6], dtype=torch.int32)

    texture, coverage = run_kernel(T, S, K, GRID, fill=fill, change=wrong)
    torch.cuda.synchronize()
    other = torch.as_tensor(owner != 3).to(DEV)
    assert torch.isfinite(texture).all() and torch.equal(texture[other], a[0][other]) and torch.equal(coverage[other], a[1][other])


# ------------------------------------------------------------------------------------------------------- generator and app
def smallest_size(T, at_least=64):
    """the texture edge of these tests, 64, or where the mesh has too many triangles for it the smallest edge that holds them"""
    return max(at_least, 4 * (math.isqrt(max((T + 1) // 2 - 1, 0)) + 1))


def test_extract_textured_mesh_bakes_the_replayed_frames():
    from test_gpu_textured_mesh import fixture
    G, cfg, z, cond, views, level = fixture()
    torch.manual_seed(7)
    plain = G.extract_textured_mesh(z, cond, views, level=level, **cfg)
    size = smallest_size(max(len(m["faces"]) for m in plain))
    torch.manual_seed(7)
    meshes = G.extract_textured_mesh(z, cond, views, level=level, texture_size=size, **cfg)
    torch.manual_seed(7)                                    # the same seed: the same ray jitter in every frame
    frames = [G.staged_forward(z, view, keep_depth_on_device=True, **cfg) for view in views]
    tolerance = 2.0 * (cfg["ray_end"] - cfg["ray_start"]) / cfg["num_steps"]
    covered = 0
    for b, (mesh, base) in enumerate(zip(meshes, plain)):
        assert set(mesh) == set(base) | {"uvs", "texture", "texture_coverage"}
        assert all(torch.equal(mesh[k], base[k]) for k in base)                        # colours included: bit-identical
        images = torch.stack([f["rgbs"][b].float().clamp(-1, 1) for f in frames])
        depths = torch.stack([f["depths"][b, 0] * (cfg["depth_length"] / 2.0) + v["intrinsics"][b, 0, 0] / v["scales"][b]
                              for f, v in zip(frames, views)])
        texture, coverage = mesh_texture.bake_texture(mesh["vertices"], mesh["faces"], mesh["normals"], images, depths,
                                                      torch.stack([v["intrinsics"][b, 0, 0] for v in views]),
                                                      torch.stack([v["scales"][b] for v in views]),
                                                      torch.stack([v["cam2world_matrices"][b] for v in views]), tolerance, size, 2)
        assert mesh["texture"].shape == (size, size, 3) and torch.equal(mesh["texture"], texture)
        assert torch.equal(mesh["texture_coverage"], coverage)
        assert np.array_equal(mesh["uvs"].cpu().numpy(), mesh_texture.atlas_uvs(len(mesh["faces"]), size))
        covered += int((coverage > 0).sum())
    print(f"texture {size}: {covered} covered texels, {[len(m['faces']) for m in meshes]} triangles")
    assert covered > 0
    state = torch.cuda.get_rng_state()
    with pytest.raises(ValueError, match="texture_size needs at least one view"):
        G.extract_textured_mesh(z, cond, [], level=level, texture_size=size, **cfg)
    assert torch.equal(torch.cuda.get_rng_state(), state)
    torch.manual_seed(7)
    avatar = G.extract_avatar(z, cond, level=level, views=views, texture_size=size, **cfg)
    assert torch.equal(avatar[1]["texture"], meshes[1]["texture"]) and torch.equal(avatar[1]["uvs"], meshes[1]["uvs"])
    assert len(avatar[1]["rest_vertices"]) == len(meshes[1]["vertices"])


def app_setup(tmp_path, name):
    app = importlib.import_module("3dhumangan_amd.apps.sample_from_generator")
    configs = importlib.import_module("3dhumangan_amd.configs")
    gens = importlib.import_module("3dhumangan_amd.lib.generators")
    impl = importlib.import_module("3dhumangan_amd.lib.implicit_funcitions")
    g = load_golden("gen_tiny_mixed")
    cfg = dict(g["meta"])
    cfg.update(neural_field_cls="COORDCONCATSIREN", name=name.lower())
    setattr(configs, name, cfg)
    ckpt = str(tmp_path / "tiny_state_dict.pth")
    torch.save(g["state"], ckpt)
    G = gens.Map3DGenerator(**dict(g["meta"], neural_field_cls=impl.COORDCONCATSIREN))
    G.load_state_dict(g["state"], strict=True)
    G = G.to(DEV).eval()
    G.set_device(DEV)
    run = dict(g["meta"], neural_field_cls=impl.COORDCONCATSIREN, truncation_psi=0.7, cache_avg_latent=True, dataset_length=4,
               v_stddev=0, h_stddev=0, nerf_noise=0, last_back=g["meta"].get("eval_last_back", False))
    common = ["--config", name, "--checkpoint", ckpt, "--dataset_length", "4", "--seeds", "3", "--mesh_resolution", "24", "--mesh_level",
              "-2.0", "--output_dir", str(tmp_path)]
    return app, G, run, common


def test_app_writes_a_textured_avatar(tmp_path):
    app, G, run, common = app_setup(tmp_path, "TINY_TEXTURE_AVATAR")
    common += ["--save", "avatar", "--pose-sequence", "synthetic", "--n_poses", "2"]
    with pytest.raises(SystemExit):
        app.main(common + ["--mesh_texture", "64"])          # no views to bake from
    sequence, pre, _ = app.load_pose_sequence(None, "synthetic", torch.device(DEV), 2, return_skeleton=True)
    by_hand, = app.generate_textured_meshes(G, pre, run, 3, {k: v[:1] for k, v in sequence.items()}, 24, -2.0, 0, avatar_k=4)
    size = smallest_size(len(by_hand["faces"]))
    out_dir = app.main(common + ["--mesh_color_views", "2", "--mesh_texture", str(size)])
    glb = RIG.Glb(f"{out_dir}/003_avatar.glb")
    mesh, = app.generate_textured_meshes(G, pre, run, 3, {k: v[:1] for k, v in sequence.items()}, 24, -2.0, 2, avatar_k=4,
                                         texture_size=size)
    T = len(mesh["faces"])
    corner = mesh["faces"].cpu().numpy().reshape(-1)
    assert T > 0 and np.array_equal(glb.faces(), np.arange(3 * T).reshape(T, 3))
    assert np.array_equal(glb.attribute("POSITION"), mesh["rest_vertices"].cpu().numpy()[corner])
    assert np.array_equal(glb.attribute("JOINTS_0"), mesh["joints"].cpu().numpy()[corner])
    assert np.array_equal(glb.attribute("TEXCOORD_0"), mesh_texture.atlas_uvs(T, size).reshape(-1, 2))
    assert "COLOR_0" not in glb.json["meshes"][0]["primitives"][0]["attributes"] and len(glb.keys()) == 2
    image = glb_image(glb)
    assert image.shape == (size, size, 3) and np.array_equal(image, mesh_texture.texture_bytes(mesh["texture"]))
    assert float(mesh["texture_coverage"].max()) > 0 and len(np.unique(image)) > 2


def test_app_writes_the_ply_unchanged_and_a_static_glb(tmp_path):
    app, G, run, common = app_setup(tmp_path, "TINY_TEXTURE_MESH")
    common += ["--save", "mesh", "--mesh_color_views", "2"]
    synthetic = importlib.import_module("3dhumangan_amd.synthetic")
    plain_dir = app.main(common + ["--postfix", "_plain"])
    names, rows, faces = parse_attributed_ply(f"{plain_dir}/003_mesh.ply")
    size = smallest_size(len(faces))
    out_dir = app.main(common + ["--postfix", "_texture", "--mesh_texture", str(size)])
    assert open(f"{out_dir}/003_mesh.ply", "rb").read() == open(f"{plain_dir}/003_mesh.ply", "rb").read()
    assert names[-3:] == ["red", "green", "blue"] and len(faces) > 0
    glb = RIG.Glb(f"{out_dir}/003_mesh.glb")
    mesh, = app.generate_textured_meshes(G, synthetic.SyntheticPreprocessor(torch.device(DEV)), run, 3, synthetic.make_conditions(1, 6890, seed=3),
                                         24, -2.0, 2, texture_size=size)
    corner = mesh["faces"].cpu().numpy().reshape(-1)
    assert np.array_equal(mesh["faces"].cpu().numpy(), faces)
    assert np.array_equal(glb.attribute("POSITION"), mesh["vertices"].cpu().numpy()[corner])
    assert np.array_equal(glb.attribute("NORMAL"), mesh["normals"].cpu().numpy()[corner])
    assert np.array_equal(glb.attribute("TEXCOORD_0"), mesh_texture.atlas_uvs(len(faces), size).reshape(-1, 2))
    assert "skins" not in glb.json and "animations" not in glb.json
    assert np.array_equal(glb_image(glb), mesh_texture.texture_bytes(mesh["texture"]))
