"""h3d_mesh_bind and h3d_mesh_pose against the float64 restatement (tests/_mesh_rig_reference.py, itself checked by
tests/test_mesh_rig_cpu.py), on every vertex: both definitions are continuous, nothing is left undecided.

Bars, the convention of tests/test_gpu_mesh_attributes.py.  No constant of this file enters one: bar = 8 x max |restatement in float32 -
restatement in float64| on the case's own inputs, and not less than 4 * 2^-23 x max |float64 output|; the maximum is taken over a pool of
at least 257 vertices made by the same generator, of which a smaller case launches the first M.  tests/test_mesh_rig_cpu.py holds every
case's bar for weights and rest positions under 1e-4; a lost neighbour or joint is of order 0.1.  Measured errors and bars are printed
and stand in DESIGN 4.5e."""
import importlib

import numpy as np
import pytest
import torch

import _mesh_rig_reference as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
mesh_rig = importlib.import_module("3dhumangan_amd.lib.components.mesh_rig")
smpl = importlib.import_module("3dhumangan_amd.lib.components.smpl")
_lib = importlib.import_module("3dhumangan_amd._lib")
DEV = "cuda"
f32, f64 = np.float32, np.float64


def dev(a, dtype=f32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def host(t):
    return t.cpu().numpy().astype(f64)


def run_bind(case, M, K, eps=1e-8, normals=True):
    return mesh_rig.bind(dev(case["X"][:M]), dev(case["P"][0] if case["P"].ndim == 3 else case["P"]), dev(case["W"]), dev(case["A"][0]),
                         normals=dev(case["N"][:M]) if normals else None, k=K, eps=eps)


def check_slots(out, J):
    """the [M,4] form: descending weights summing to 1, joints in range, a zero slot carries joint 0"""
    joints, weights = out["joints"].cpu().numpy(), host(out["weights"])
    assert out["joints"].dtype == torch.int32 and out["weights"].dtype == torch.float32
    assert ((joints >= 0) & (joints < J)).all() and (weights >= 0).all()
    assert (np.diff(weights, axis=1) <= 0).all() and (joints[weights == 0] == 0).all()
    assert np.abs(weights.sum(axis=1) - 1).max() <= 4 * 2.0 ** -23
    for a in range(4):
        for b in range(a + 1, 4):
            both = (weights[:, a] > 0) & (weights[:, b] > 0)
            assert (joints[both, a] != joints[both, b]).all()


@pytest.mark.parametrize("M,V,J,K", R.CASES, ids=lambda v: str(v))
def test_bind_against_the_restatement(M, V, J, K):
    case = R.make_case(M, V, J, K)
    hi, bars = R.case_bars(case)
    out = run_bind(case, M, K)
    assert out["rest_vertices"].shape == out["rest_normals"].shape == (M, 3) and out["det"].shape == (M,)
    assert out["joints"].shape == out["weights"].shape == (M, 4)
    check_slots(out, J)
    dense = host(mesh_rig.dense_weights(out["joints"], out["weights"], J))
    errs = {"dense": np.abs(dense - hi["dense"][:M]).max(), "rest_vertices": np.abs(host(out["rest_vertices"]) - hi["rest_vertices"][:M]).max(),
            "rest_normals": np.abs(host(out["rest_normals"]) - hi["rest_normals"][:M]).max(), "det": np.abs(host(out["det"]) - hi["det"][:M]).max()}
    print(f"bind M={M} V={V} J={J} K={K}: " + "; ".join(f"{k} err {errs[k]:.2e} bar {bars[k]:.2e}" for k in errs))
    for k in errs:
        assert errs[k] <= bars[k], k
    # without normals: the same rig, no rest normals
    plain = run_bind(case, M, K, normals=False)
    assert plain["rest_normals"] is None
    assert all(torch.equal(plain[k], out[k]) for k in ("rest_vertices", "joints", "weights", "det"))


@pytest.mark.parametrize("K", [1, 4, 7])
def test_exact_degeneracy_on_the_lattice(K):
    case = R.lattice_case(K)
    M, J = len(case["X"]), case["W"].shape[1]
    lo, hi = (R.bind(case["X"], case["P"], case["W"], case["A"][0], K=K, dtype=d) for d in (f32, f64))
    out = mesh_rig.bind(dev(case["X"]), dev(case["P"]), dev(case["W"]), dev(case["A"][0]), k=K)
    check_slots(out, J)
    dense = host(mesh_rig.dense_weights(out["joints"], out["weights"], J))
    decided = R.decided_rows(R.blend_weights(case["X"], case["P"], case["W"], K, 1e-8, f64)[0])
    assert np.array_equal(dense[decided] > 0, hi["dense"][decided] > 0)                 # the joint sets, exactly
    # equal weights over the K lowest-index ties: w' of the plain mean of their rows
    mean = case["W"][case["corners"][:, :K]].astype(f64).mean(axis=1)
    expected, _, _ = R.cut_to_four(mean, f64)
    bar_w, bar_x = R.bar_of(lo["dense"], hi["dense"]), R.bar_of(lo["rest_vertices"], hi["rest_vertices"])
    err_w, err_x = np.abs(dense - expected).max(), np.abs(host(out["rest_vertices"]) - hi["rest_vertices"]).max()
    print(f"lattice K={K}: weights err {err_w:.2e} bar {bar_w:.2e}; rest err {err_x:.2e} bar {bar_x:.2e}; {int(decided.sum())} of {M} decided")
    assert np.abs(expected - hi["dense"]).max() < 1e-12
    assert err_w <= bar_w and err_x <= bar_x


@pytest.mark.parametrize("n", [1, 3])
def test_pose_against_the_restatement_and_round_trip(n):
    M, V, J, K = 257, 97, 24, 4
    case = R.make_case(M, V, J, K, n_poses=n)
    out = run_bind(case, M, K)
    A = dev(case["A"])
    vertices, normals = mesh_rig.pose(out["rest_vertices"], out["joints"], out["weights"], A, out["rest_normals"])
    assert vertices.shape == normals.shape == (n, M, 3) and vertices.dtype == normals.dtype == torch.float32
    # pose alone: the restatement on the kernel's own inputs
    rest, joints, weights, rn = (out[k].cpu().numpy() for k in ("rest_vertices", "joints", "weights", "rest_normals"))
    v64, n64 = R.pose(rest, joints, weights, case["A"], rn, f64)
    v32, n32 = R.pose(rest, joints, weights, case["A"], rn, f32)
    bar_v, bar_n = R.bar_of(v32, v64), R.bar_of(n32, n64)
    err_v, err_n = np.abs(host(vertices) - v64).max(), np.abs(host(normals) - n64).max()
    # the round trip: bind and pose in float32 against the input itself
    lo = R.bind(case["X"], case["P"][0], case["W"], case["A"][0], case["N"], K, dtype=f32)
    rv32, rn32 = R.pose(lo["rest_vertices"], lo["joints"], lo["weights"], case["A"][:1], lo["rest_normals"], f32)
    X, N = case["X"].astype(f64), case["N"].astype(f64) / np.linalg.norm(case["N"].astype(f64), axis=1, keepdims=True)
    bar_rv, bar_rn = R.bar_of(rv32[0], X), R.bar_of(rn32[0], N)
    err_rv, err_rn = np.abs(host(vertices[0]) - X).max(), np.abs(host(normals[0]) - N).max()
    # the existing skinning kernel with the dense form of the same weights
    dense = mesh_rig.dense_weights(out["joints"], out["weights"], J)
    skinned = smpl.skin_vertices(out["rest_vertices"][None].expand(n, M, 3), A, dense)
    err_s = np.abs(host(skinned) - v64).max()
    print(f"pose n={n}: vertices err {err_v:.2e} bar {bar_v:.2e}; normals err {err_n:.2e} bar {bar_n:.2e}; round trip err {err_rv:.2e} "
          f"bar {bar_rv:.2e}, normals {err_rn:.2e} bar {bar_rn:.2e}; skin_vertices err {err_s:.2e}")
    assert err_v <= bar_v and err_n <= bar_n
    assert err_rv <= bar_rv and err_rn <= bar_rn
    assert err_s <= bar_v
    if n > 1:
        assert np.abs(host(vertices[1]) - X).max() > 1e-2                           # another pose is another mesh
    only_vertices, none = mesh_rig.pose(out["rest_vertices"], out["joints"], out["weights"], A)
    assert none is None and torch.equal(only_vertices, vertices)
    first, first_n = mesh_rig.pose(out["rest_vertices"], out["joints"], out["weights"], A[:1], out["rest_normals"])
    assert torch.equal(first[0], vertices[0]) and torch.equal(first_n[0], normals[0])     # a pose does not depend on its batch


def test_empty_twice_and_refusals():
    case = R.make_case(4099, 97, 24, 4, n_poses=2)
    a, b = run_bind(case, 4099, 4), run_bind(case, 4099, 4)
    assert all(torch.equal(a[k], b[k]) for k in a)
    A = dev(case["A"])
    pa, pb = (mesh_rig.pose(a["rest_vertices"], a["joints"], a["weights"], A, a["rest_normals"]) for _ in range(2))
    assert torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1])
    empty = run_bind(case, 0, 4)
    assert empty["rest_vertices"].shape == (0, 3) and empty["joints"].shape == (0, 4) and empty["det"].shape == (0,)
    assert empty["weights"].device.type == "cuda"
    v, n = mesh_rig.pose(empty["rest_vertices"], empty["joints"], empty["weights"], A, empty["rest_normals"])
    assert v.shape == n.shape == (2, 0, 3)
    assert mesh_rig.dense_weights(empty["joints"], empty["weights"], 24).shape == (0, 24)
    X, P, W, fk, N = dev(case["X"][:10]), dev(case["P"][0]), dev(case["W"]), dev(case["A"][0]), dev(case["N"][:10])
    for match, call in [("vertices", lambda: mesh_rig.bind(X[:, :2], P, W, fk)), ("k=9", lambda: mesh_rig.bind(X, P, W, fk, k=9)),
                        ("k=0", lambda: mesh_rig.bind(X, P, W, fk, k=0)), ("smpl_vertices has 4 rows", lambda: mesh_rig.bind(X, P[:4], W[:4], fk)),
                        ("smpl_vertices", lambda: mesh_rig.bind(X, P.reshape(-1), W, fk)), ("lbs_weights", lambda: mesh_rig.bind(X, P, W[:-1], fk)),
                        ("fk_matrices", lambda: mesh_rig.bind(X, P, W, fk[:-1])), ("normals", lambda: mesh_rig.bind(X, P, W, fk, normals=N[:-1])),
                        ("eps", lambda: mesh_rig.bind(X, P, W, fk, eps=0.0)),
                        ("rest_vertices", lambda: mesh_rig.pose(X[:, :2], a["joints"][:10], a["weights"][:10], A)),
                        ("joints", lambda: mesh_rig.pose(X, a["joints"][:9], a["weights"][:10], A)),
                        ("joints", lambda: mesh_rig.pose(X, a["weights"][:10], a["weights"][:10], A)),
                        ("weights", lambda: mesh_rig.pose(X, a["joints"][:10], a["weights"][:10, :3], A)),
                        ("fk_matrices", lambda: mesh_rig.pose(X, a["joints"][:10], a["weights"][:10], A[:, :, :3])),
                        ("rest_normals", lambda: mesh_rig.pose(X, a["joints"][:10], a["weights"][:10], A, N[:-1])),
                        ("dense_weights", lambda: mesh_rig.dense_weights(a["joints"][:10], a["weights"][:9], 24))]:
        with pytest.raises(ValueError, match=match):
            call()
    with pytest.raises(RuntimeError, match="not differentiable"):
        mesh_rig.bind(X.clone().requires_grad_(), P, W, fk)
    with pytest.raises(_lib.H3DError):
        mesh_rig.bind(X.cpu(), P, W, fk)


def test_extract_avatar_is_the_textured_mesh_with_a_direct_bind():
    from test_gpu_textured_mesh import fixture
    G, cfg, z, cond, views, level = fixture()
    torch.manual_seed(7)
    plain = G.extract_textured_mesh(z, cond, views, level=level, **cfg)
    torch.manual_seed(7)
    avatars = G.extract_avatar(z, cond, k=3, level=level, views=views, **cfg)
    assert len(avatars) == len(plain) == 2
    for b, (mesh, base) in enumerate(zip(avatars, plain)):
        assert set(mesh) == set(base) | {"rest_vertices", "rest_normals", "joints", "weights", "det"}
        assert len(base["faces"]) > 0 and all(torch.equal(mesh[k], base[k]) for k in base)
        rig = mesh_rig.bind(base["vertices"], cond["vertices"][b], cond["lbs_weights"][b], cond["fk_matrices"][b], normals=base["normals"], k=3)
        assert all(torch.equal(mesh[k], rig[k]) for k in rig)
        check_slots(mesh, cond["lbs_weights"].shape[-1])
        assert torch.isfinite(mesh["rest_vertices"]).all() and float(mesh["det"].min()) > 0
    other = G.extract_avatar(z, cond, k=4, level=level, **cfg)                       # k reaches the kernel; no views, no colours
    assert other[0]["colors"] is None and not torch.equal(other[0]["weights"], avatars[0]["weights"])
    with pytest.raises(NotImplementedError, match="clamp_mode='softplus'"):
        G.extract_avatar(z, cond, level=level, **dict(cfg, clamp_mode="softplus"))


def test_app_writes_an_avatar_that_plays_back(tmp_path):
    app = importlib.import_module("3dhumangan_amd.apps.sample_from_generator")
    configs = importlib.import_module("3dhumangan_amd.configs")
    gens = importlib.import_module("3dhumangan_amd.lib.generators")
    impl = importlib.import_module("3dhumangan_amd.lib.implicit_funcitions")
    g = load_golden("gen_tiny_mixed")
    cfg = dict(g["meta"])
    cfg.update(neural_field_cls="COORDCONCATSIREN", name="tiny_avatar")
    configs.TINY_AVATAR = cfg
    ckpt = str(tmp_path / "tiny_state_dict.pth")
    torch.save(g["state"], ckpt)
    level, bind_pose = -2.0, 1                       # the level: inside the density range of the fixture's weights
    common = ["--config", "TINY_AVATAR", "--checkpoint", ckpt, "--dataset_length", "4", "--seeds", "3", "--save", "avatar",
              "--mesh_resolution", "24", "--mesh_level", str(level), "--output_dir", str(tmp_path)]
    with pytest.raises(ValueError, match="--pose-sequence"):
        app.main(common)
    out_dir = app.main(common + ["--pose-sequence", "synthetic", "--n_poses", "3", "--avatar_bind_pose", str(bind_pose)])
    glb = R.Glb(f"{out_dir}/003_avatar.glb")
    # by hand: the app's config and seed convention, extract_avatar at the bind pose
    G = gens.Map3DGenerator(**dict(g["meta"], neural_field_cls=impl.COORDCONCATSIREN))
    G.load_state_dict(g["state"], strict=True)
    G = G.to(DEV).eval()
    G.set_device(DEV)
    run = dict(g["meta"], neural_field_cls=impl.COORDCONCATSIREN, truncation_psi=0.7, cache_avg_latent=True, dataset_length=4,
               v_stddev=0, h_stddev=0, nerf_noise=0, last_back=g["meta"].get("eval_last_back", False))
    sequence, _, skeleton = app.load_pose_sequence(None, "synthetic", torch.device(DEV), 3, return_skeleton=True)
    latent = app.latent_for_seed(3, run["latent_dim"]).to(DEV)
    body = {k: sequence[k][bind_pose:bind_pose + 1] for k in G.MESH_CONDITIONS}
    mesh, = G.extract_avatar(latent, body, k=4, level=level, resolution=24, **run)
    M = len(mesh["vertices"])
    assert M > 257 and np.array_equal(glb.faces(), mesh["faces"].cpu().numpy())
    assert np.array_equal(glb.attribute("POSITION"), mesh["rest_vertices"].cpu().numpy())
    assert np.array_equal(glb.attribute("NORMAL"), mesh["rest_normals"].cpu().numpy())
    assert np.array_equal(glb.attribute("JOINTS_0"), mesh["joints"].cpu().numpy())
    assert np.array_equal(glb.attribute("WEIGHTS_0"), mesh["weights"].cpu().numpy())
    assert np.allclose(glb.keys(), np.arange(3) / 20.0, rtol=1e-7, atol=0)
    parents = [int(p) for p in skeleton["parents"]]
    posed, _ = mesh_rig.pose(mesh["rest_vertices"], mesh["joints"], mesh["weights"], sequence["fk_matrices"])
    posed = host(posed)
    bar = R.evaluator_bar(parents, posed)
    played = np.stack([glb.skinned(key) for key in range(3)])
    errs = np.abs(played - posed).max(axis=(1, 2))
    # the bind key against the extracted mesh itself: the evaluator's bar plus the rounding of the round trip, from the restatement
    # on a pool of the mesh's own vertices
    pool = slice(0, 257)
    X, P, W, A = (t.cpu().numpy() for t in (mesh["vertices"][pool], body["vertices"][0], body["lbs_weights"][0], body["fk_matrices"][0]))
    lo = R.bind(X, P, W, A, K=4, dtype=f32)
    trip, _ = R.pose(lo["rest_vertices"], lo["joints"], lo["weights"], A[None], dtype=f32)
    bar_trip = R.bar_of(trip[0], X.astype(f64))
    err_bind = np.abs(played[bind_pose] - host(mesh["vertices"])).max()
    print(f"avatar M={M}: playback errs {errs} bar {bar:.2e}; bind key against the mesh {err_bind:.2e} bar {bar + bar_trip:.2e}")
    assert bar < 1e-3 and (errs <= bar).all()
    assert err_bind <= bar + bar_trip
    assert np.abs(played[0] - played[2]).max() > 1e-2                                 # the poses differ
