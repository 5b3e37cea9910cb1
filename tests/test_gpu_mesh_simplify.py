"""lib/components/mesh_simplify.simplify (h3d_mesh_cluster_cells / _faces / _solve) against the numpy restatement
(tests/_mesh_simplify_reference.py, itself checked by tests/test_mesh_simplify_cpu.py); then the generator and the app, held to the
stage bit for bit.

cluster, the cell table and the faces are integers and must be equal.  Positions: the bar convention of tests/test_gpu_mesh_attributes.py.
No constant of this file enters one: bar = 8 x max |restatement in float32 - restatement in float64| on the case's own inputs, and not
less than 4 * 2^-23 x max |float64 coordinate|.  The maximum needs enough clusters to be the size of the rounding and not one draw of
it: a case with fewer than 257 clusters takes the bar of the rotated 32^3 box at cell 4.  The fan cases are built so that the cluster of
1 / 63 / 64 / 65 / 129 records moves by more than that bar when any one of its records is lost (asserted here and in
tests/test_mesh_simplify_cpu.py with the restatement: at least 6.6e-3 against 6.9e-4).  Measured errors and bars are printed and stand
in DESIGN 4.5g."""
import importlib
import math

import numpy as np
import pytest
import torch

import _mesh_rig_reference as RIG
import _mesh_simplify_reference as R
from _mesh_attributes_reference import parse_attributed_ply

pytestmark = pytest.mark.gpu
mesh_simplify = importlib.import_module("3dhumangan_amd.lib.components.mesh_simplify")
mesh_texture = importlib.import_module("3dhumangan_amd.lib.components.mesh_texture")
mesh_rig = importlib.import_module("3dhumangan_amd.lib.components.mesh_rig")
iso = importlib.import_module("3dhumangan_amd.lib.components.isosurface")
DEV = "cuda"
f32, f64 = np.float32, np.float64
_CACHE = {}


def dev(a, dtype=f32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def case_of(name):
    """-> (vertices fp32, faces int32, cell, origin, counts, reach)"""
    if name.startswith("fan"):                               # the hubs' cluster has exactly that many corner records, and needs each
        v, f = R.fan(int(name[3:]))
        return v, f, 1.0, (0.0, 0.0, 0.0), (9, 9, 9), 1.0
    if name == "vertex":                                     # V = 1, T = 0
        return np.array([[0.25, 1.5, 0.75]], f32), np.zeros((0, 3), np.int32), 1.0, (0.0, 0.0, 0.0), (2, 2, 2), 1.0
    if name == "triangle":                                   # one triangle across three cells
        return np.array([[0.3, 0.2, 0.1], [1.6, 0.4, 0.2], [0.5, 1.7, 0.9]], f32), np.array([[0, 1, 2]], np.int32), 1.0, (0.0, 0.0, 0.0), (2, 2, 2), 1.0
    if name == "one_cell":                                   # every vertex in one cell
        return R.sphere_mesh(24, 9.0) + (100.0, (0.0, 0.0, 0.0), (1, 1, 1), 1.0)
    if name == "sphere_2":
        return R.sphere_mesh(24, 9.0) + (2.0,) + R.grid_of((0, 0, 0), (23, 23, 23), 2.0) + (1.0,)
    if name == "sphere_3.5":                                 # a non-integer cell; 7 cells of 3.5 over 23: the last is ragged on every axis
        return R.sphere_mesh(24, 9.0) + (3.5,) + R.grid_of((0, 0, 0), (23, 23, 23), 3.5) + (0.5,)
    if name == "sphere_clamped":                             # counts that end inside the mesh: what lies beyond joins the last cell
        return R.sphere_mesh(24, 9.0) + (2.0, (3.0, 2.5, 4.0), (7, 8, 6), 1.0)
    if name == "box_4":
        return R.box_mesh() + (4.0,) + R.grid_of((0, 0, 0), (31, 31, 31), 4.0) + (1.0,)
    raise KeyError(name)


def restated(name):
    """-> {f32: ..., f64: ...} of the restatement's dicts, computed once per case and shared"""
    if name not in _CACHE:
        v, f, cell, origin, counts, reach = case_of(name)
        _CACHE[name] = {dtype: R.simplify(v, f, cell, origin, counts, reach=reach, dtype=dtype) for dtype in (f32, f64)}
    return _CACHE[name]


def bar_between(low, high):
    """low, high: the restatement's dicts in float32 and float64 on one case"""
    if len(high["cells"]) < 257:
        low, high = restated("box_4")[f32], restated("box_4")[f64]
    low, high = low["vertices"].astype(f64), high["vertices"]
    return max(8.0 * float(np.abs(low - high).max()), 4.0 * 2.0 ** -23 * float(np.abs(high).max()))


def bar_of(name):
    return bar_between(restated(name)[f32], restated(name)[f64])


def fan_sensitivity(n):
    """the least move of the fan's hub cluster (float64 restatement) when one of its n corner records is taken away"""
    if ("fan", n) not in _CACHE:
        v, f, cell, origin, counts, reach = case_of(f"fan{n}")
        full = restated(f"fan{n}")[f64]
        hub = full["cluster"][0]
        moves = [np.abs(R.simplify(v, np.delete(f, k, axis=0), cell, origin, counts, reach=reach)["vertices"][hub] - full["vertices"][hub]).max()
                 for k in range(n)]
        _CACHE["fan", n] = float(min(moves))
    return _CACHE["fan", n]


def run(name, change=None, **kwargs):
    v, f, cell, origin, counts, reach = case_of(name)
    args = dict(vertices=dev(v), faces=dev(f, np.int32))
    if change:
        change(args)
    return mesh_simplify.simplify(args["vertices"], args["faces"], cell, origin=origin, counts=counts, reach=reach, return_cells=True, **kwargs)


CASES = ["vertex", "triangle", "fan1", "fan63", "fan64", "fan65", "fan129", "one_cell", "sphere_2", "sphere_3.5", "sphere_clamped", "box_4"]


@pytest.mark.parametrize("name", CASES)
def test_simplify_against_the_restatement(name):
    ref, bar = restated(name)[f64], bar_of(name)
    vertices, faces, cluster, cells = run(name)
    assert vertices.dtype == torch.float32 and faces.dtype == cluster.dtype == cells.dtype == torch.int32
    assert vertices.shape == ref["vertices"].shape and faces.shape == ref["faces"].shape
    assert np.array_equal(cells.cpu().numpy(), ref["cells"])
    assert np.array_equal(cluster.cpu().numpy(), ref["cluster"])
    assert np.array_equal(faces.cpu().numpy(), ref["faces"])
    err = float(np.abs(vertices.cpu().numpy().astype(f64) - ref["vertices"]).max())
    print(f"simplify {name}: V={len(ref['cluster'])} T={len(case_of(name)[1])} -> C={len(ref['cells'])} T'={len(ref['faces'])}; "
          f"position err {err:.2e} bar {bar:.2e}")
    assert err <= bar
    if name.startswith("fan"):                               # the case is what it says: the two hubs' cluster has that many records
        n = int(name[3:])
        hub = ref["cluster"][0]
        assert (ref["cluster"] == hub).sum() == 2 and (ref["cluster"][case_of(name)[1]] == hub).sum() == n
        hub_err = float(np.abs(vertices[hub].cpu().numpy().astype(f64) - ref["vertices"][hub]).max())
        print(f"    the hubs' cluster: err {hub_err:.2e}; without any one of its records it moves by at least "
              f"{fan_sensitivity(n):.2e} (tests/test_mesh_simplify_cpu.py)")
        assert fan_sensitivity(n) > bar
    if name == "one_cell":
        assert len(ref["cells"]) == 1 and len(ref["faces"]) == 0
    if name == "sphere_clamped":
        assert ref["cells"][-1] == 7 * 8 * 6 - 1


def test_default_grid_is_the_box_of_the_vertices():
    v, f = R.sphere_mesh(24, 9.0)
    origin, counts = R.grid_of(v.min(axis=0), v.max(axis=0), 2.5)
    ref = R.simplify(v, f, 2.5, origin, counts)
    vertices, faces, cluster = mesh_simplify.simplify(dev(v), dev(f, np.int32), 2.5)
    assert np.array_equal(cluster.cpu().numpy(), ref["cluster"]) and np.array_equal(faces.cpu().numpy(), ref["faces"])
    assert np.abs(vertices.cpu().numpy() - ref["vertices"]).max() <= bar_between(R.simplify(v, f, 2.5, origin, counts, dtype=f32), ref)
    poisoned = dev(v)
    poisoned[5] = float("nan")                               # the box is that of the finite coordinates
    again = mesh_simplify.simplify(poisoned, dev(f, np.int32), 2.5)
    assert torch.isfinite(again[0]).all() and int(again[2][5]) == 0
    empty = mesh_simplify.simplify(dev(v)[:0], dev(f, np.int32)[:0], 2.5)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3) and empty[2].shape == (0,)


def test_twice_noncontiguous_nonfinite_and_wrong_indices():
    name = "sphere_2"
    a, b = run(name), run(name)
    assert all(torch.equal(x, y) for x, y in zip(a, b))

    def strided(args):
        args["faces"] = torch.stack([args["faces"], args["faces"]], dim=2)[:, :, 0]          # stride 2
        args["vertices"] = args["vertices"].t().contiguous().t()
        assert not args["faces"].is_contiguous() and not args["vertices"].is_contiguous()

    c = run(name, change=strided)
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    # a NaN vertex: it goes to cell 0, which opens a cluster in front of all others; every cluster that holds neither it nor a corner
    # of one of its faces keeps its bits
    v, f = case_of(name)[:2]
    victim = int(f[100, 0])

    def poisoned(args):
        args["vertices"][victim] = float("nan")

    vertices, faces, cluster, cells = run(name, change=poisoned)
    assert int(a[3][0]) > 0 and int(cells[0]) == 0 and int(cluster[victim]) == 0 and len(cells) == len(a[3]) + 1
    assert torch.isfinite(vertices).all() and torch.equal(vertices[0], torch.tensor([1.0, 1.0, 1.0], device=DEV))
    before = a[2].cpu().numpy()
    touched = np.unique(before[f[(f == victim).any(axis=1)]])
    same = torch.as_tensor(np.setdiff1d(np.arange(len(a[3])), touched)).to(DEV)
    assert len(same) > len(a[3]) // 2 and torch.equal(vertices[1:][same], a[0][same])
    moved = torch.as_tensor(touched).to(DEV)
    assert not torch.equal(vertices[1:][moved], a[0][moved])

    # face indices out of range are clamped into it: a wrong mesh, no fault and no error
    def wrong(args):
        args["faces"][7] = torch.tensor([-5, 2 ** 31 - 1, 10 ** 6], dtype=torch.int32)

    vertices, faces, cluster, cells = run(name, change=wrong)
    torch.cuda.synchronize()
    bad = f.astype(np.int64).copy()
    bad[7] = [-5, 2 ** 31 - 1, 10 ** 6]
    _, _, cell, origin, counts, reach = case_of(name)
    ref = R.simplify(v, bad, cell, origin, counts, reach=reach)
    assert torch.isfinite(vertices).all() and np.array_equal(faces.cpu().numpy(), ref["faces"])
    assert np.abs(vertices.cpu().numpy() - ref["vertices"]).max() <= bar_between(R.simplify(v, bad, cell, origin, counts, reach=reach, dtype=f32), ref)
    # regularization and reach reach the kernel
    other = run(name, regularization=1.0)
    assert torch.equal(other[1], a[1]) and not torch.equal(other[0], a[0])


# ------------------------------------------------------------------------------------------------------- generator and app
def grid_of_density(sigma, origin, spacing, b, k):
    nodes = sigma.shape[1:]
    o, s = origin[b].tolist(), spacing[b].tolist()
    return o, s, k * s[0], [int(math.floor((n - 1) / k)) + 1 for n in nodes]


def test_extract_mesh_is_the_stage_after_marching_tetrahedra():
    from test_gpu_textured_mesh import fixture
    G, cfg, z, cond, views, level = fixture()
    plain = G.extract_mesh(z, cond, level=level, **cfg)
    off = G.extract_mesh(z, cond, level=level, simplify=None, **cfg)
    assert all(torch.equal(a, b) for p, q in zip(plain, off) for a, b in zip(p, q))
    small = G.extract_mesh(z, cond, level=level, simplify=3, **cfg)
    sigma, origin, spacing = G.density_grid(z, cond, **cfg)
    for b, ((v0, f0), (v1, f1)) in enumerate(zip(plain, small)):
        o, s, cell, counts = grid_of_density(sigma, origin, spacing, b, 3)
        v, f = iso.marching_tetrahedra(sigma[b], level, o, s)
        assert torch.equal(v, v0) and torch.equal(f, f0)
        by_hand = mesh_simplify.simplify(v, f, cell, origin=o, counts=counts)
        assert torch.equal(v1, by_hand[0]) and torch.equal(f1, by_hand[1])
        print(f"item {b}: {len(f0)} -> {len(f1)} faces, {len(v0)} -> {len(v1)} vertices")
        assert 0 < len(f1) < len(f0) and len(v1) < len(v0)
    for bad in (0, -1.0, float("nan"), float("inf"), "3", True):
        with pytest.raises(ValueError, match="simplify=.* must be a positive number"):
            G.extract_mesh(z, cond, level=level, simplify=bad, **cfg)


def test_textured_mesh_and_avatar_belong_to_the_simplified_mesh():
    from test_gpu_textured_mesh import fixture
    G, cfg, z, cond, views, level = fixture()
    torch.manual_seed(7)
    plain = G.extract_textured_mesh(z, cond, views, level=level, **cfg)
    torch.manual_seed(7)
    off = G.extract_textured_mesh(z, cond, views, level=level, simplify=None, **cfg)
    assert all(torch.equal(p[k], q[k]) for p, q in zip(plain, off) for k in p)
    small = G.extract_mesh(z, cond, level=level, simplify=3, **cfg)
    size = max(smallest_size(len(f1)) for _, f1 in small)
    torch.manual_seed(7)
    textured = G.extract_textured_mesh(z, cond, views, level=level, simplify=3, texture_size=size, **cfg)
    torch.manual_seed(7)
    avatars = G.extract_avatar(z, cond, level=level, views=views, simplify=3, texture_size=size, **cfg)
    sigma, origin, spacing = G.density_grid(z, cond, **cfg)
    for b, (mesh, avatar, (v1, f1), base) in enumerate(zip(textured, avatars, small, plain)):
        assert torch.equal(mesh["vertices"], v1) and torch.equal(mesh["faces"], f1)
        V, T = len(v1), len(f1)
        assert 0 < T < len(base["faces"])
        assert mesh["normals"].shape == mesh["colors"].shape == (V, 3) and mesh["coverage"].shape == (V,)
        assert mesh["uvs"].shape == (T, 3, 2) and mesh["texture"].shape == (size, size, 3)
        assert torch.equal(mesh["normals"], iso.vertex_normals(sigma[b], v1, origin[b].tolist(), spacing[b].tolist()))
        length = mesh["normals"].double().norm(dim=1)
        assert ((length == 0) | ((length - 1).abs() < 1e-5)).all() and (length > 0).float().mean() > 0.9
        assert mesh_texture.atlas_layout(T, 2048)[0] > mesh_texture.atlas_layout(len(base["faces"]), 2048)[0]
        assert all(torch.equal(avatar[k], mesh[k]) for k in mesh)
        assert all(len(avatar[k]) == V for k in ("rest_vertices", "rest_normals", "joints", "weights", "det"))
        # posing the rest mesh with the item's own transforms gives back the simplified vertices: the bar of tests/test_gpu_mesh_rig.py,
        # the float32 round trip of the restatement on a pool of the mesh's own vertices
        posed, _ = mesh_rig.pose(avatar["rest_vertices"], avatar["joints"], avatar["weights"], cond["fk_matrices"][b:b + 1])
        pool = slice(0, 257)
        lbs = cond["lbs_weights"][b] if cond["lbs_weights"].dim() == 3 else cond["lbs_weights"]
        X, P, W, A = (t.cpu().numpy() for t in (v1[pool], cond["vertices"][b], lbs, cond["fk_matrices"][b]))
        lo = RIG.bind(X, P, W, A, K=4, dtype=f32)
        trip, _ = RIG.pose(lo["rest_vertices"], lo["joints"], lo["weights"], A[None], dtype=f32)
        bar = RIG.bar_of(trip[0], X.astype(f64))
        err = float((posed[0] - v1).abs().max())
        print(f"item {b}: V={V} T={T} (from {len(base['faces'])}); pose round trip err {err:.2e} bar {bar:.2e}")
        assert err <= bar


def app_setup(tmp_path, name):
    from test_gpu_texture_bake import app_setup as setup
    return setup(tmp_path, name)


def smallest_size(T):
    from test_gpu_texture_bake import smallest_size as smallest
    return smallest(T)


def test_app_writes_the_simplified_mesh(tmp_path):
    app, G, run_cfg, common = app_setup(tmp_path, "TINY_SIMPLIFY_MESH")
    synthetic = importlib.import_module("3dhumangan_amd.synthetic")
    mesh_io = importlib.import_module("3dhumangan_amd.lib.components.mesh_io")
    with pytest.raises(SystemExit):
        app.main(common + ["--save", "png", "--mesh_simplify", "3"])
    with pytest.raises(SystemExit):
        app.main(common + ["--save", "mesh", "--mesh_simplify", "-1"])
    # without the flag: the plain export, byte for byte
    plain_dir = app.main(common + ["--save", "mesh", "--postfix", "_plain"])
    data = synthetic.make_conditions(1, 6890, seed=3)
    latent = app.latent_for_seed(3, run_cfg["latent_dim"]).to(DEV)
    body = {k: data[k][:1].to(DEV) for k in G.MESH_CONDITIONS}
    (v0, f0), = G.extract_mesh(latent, body, level=-2.0, resolution=24, **run_cfg)
    by_hand = str(tmp_path / "by_hand.ply")
    mesh_io.write_ply(by_hand, v0, f0)
    assert open(by_hand, "rb").read() == open(f"{plain_dir}/003_mesh.ply", "rb").read()
    # with it: the files hold what generate_textured_meshes returns with the same setting
    (v1, f1), = app.generate_meshes(G, run_cfg, 3, data, 24, -2.0, simplify=3.0)
    size = smallest_size(len(f1))
    out_dir = app.main(common + ["--save", "mesh", "--postfix", "_small", "--mesh_color_views", "2", "--mesh_texture", str(size),
                                 "--mesh_simplify", "3"])
    mesh, = app.generate_textured_meshes(G, synthetic.SyntheticPreprocessor(torch.device(DEV)), run_cfg, 3, data, 24, -2.0, 2,
                                         texture_size=size, simplify=3.0)
    names, rows, faces = parse_attributed_ply(f"{out_dir}/003_mesh.ply")
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert 0 < len(faces) < len(f0) and np.array_equal(faces, mesh["faces"].cpu().numpy())
    assert np.array_equal(np.stack([rows[k] for k in "xyz"], axis=1), mesh["vertices"].cpu().numpy())
    assert np.array_equal(np.stack([rows[k] for k in ("nx", "ny", "nz")], axis=1), mesh["normals"].cpu().numpy())
    glb = RIG.Glb(f"{out_dir}/003_mesh.glb")
    corner = mesh["faces"].cpu().numpy().reshape(-1)
    assert np.array_equal(glb.attribute("POSITION"), mesh["vertices"].cpu().numpy()[corner])
    assert np.array_equal(glb.attribute("TEXCOORD_0"), mesh_texture.atlas_uvs(len(faces), size).reshape(-1, 2))
    assert torch.equal(v1, mesh["vertices"]) and torch.equal(f1, mesh["faces"])


def test_app_writes_the_simplified_avatar(tmp_path):
    app, G, run_cfg, common = app_setup(tmp_path, "TINY_SIMPLIFY_AVATAR")
    common += ["--save", "avatar", "--pose-sequence", "synthetic", "--n_poses", "2"]
    out_dir = app.main(common + ["--mesh_simplify", "3"])
    sequence, pre, skeleton = app.load_pose_sequence(None, "synthetic", torch.device(DEV), 2, return_skeleton=True)
    first = {k: v[:1] for k, v in sequence.items()}
    mesh, = app.generate_textured_meshes(G, pre, run_cfg, 3, first, 24, -2.0, 0, avatar_k=4, simplify=3.0)
    full, = app.generate_textured_meshes(G, pre, run_cfg, 3, first, 24, -2.0, 0, avatar_k=4)
    # without the flag: the file of the export as it was, byte for byte -- written here with simplify=None, as the app wrote it before
    mesh_io = importlib.import_module("3dhumangan_amd.lib.components.mesh_io")
    plain_dir = app.main(common + ["--postfix", "_plain"])
    off, = app.generate_textured_meshes(G, pre, run_cfg, 3, first, 24, -2.0, 0, avatar_k=4, simplify=None)
    assert all(torch.equal(off[k], full[k]) for k in full if full[k] is not None)
    by_hand = str(tmp_path / "by_hand.glb")
    mesh_io.write_glb(by_hand, off["rest_vertices"], off["faces"], off["joints"], off["weights"], skeleton["rest_joints"][0],
                      skeleton["parents"], normals=off["rest_normals"], frames=sequence["fk_matrices"], fps=20, colors=off["colors"])
    assert open(by_hand, "rb").read() == open(f"{plain_dir}/003_avatar.glb", "rb").read()
    glb = RIG.Glb(f"{out_dir}/003_avatar.glb")
    assert 0 < len(mesh["faces"]) < len(full["faces"]) and np.array_equal(glb.faces(), mesh["faces"].cpu().numpy())
    assert np.array_equal(glb.attribute("POSITION"), mesh["rest_vertices"].cpu().numpy())
    assert np.array_equal(glb.attribute("NORMAL"), mesh["rest_normals"].cpu().numpy())
    assert np.array_equal(glb.attribute("JOINTS_0"), mesh["joints"].cpu().numpy())
    assert np.array_equal(glb.attribute("WEIGHTS_0"), mesh["weights"].cpu().numpy())
