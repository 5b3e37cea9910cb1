"""No GPU: the numpy restatement of the mesh-rig definitions (tests/_mesh_rig_reference.py) held to the properties the text of
include/h3d.h promises, the glTF writer held to an independent evaluator, and the bars of every GPU case held under their cap."""
import ctypes
import importlib
import json
import struct

import numpy as np
import pytest

import _mesh_rig_reference as R

mesh_io = importlib.import_module("3dhumangan_amd.lib.components.mesh_io")
f32, f64 = np.float32, np.float64


def test_weights_are_a_partition_of_unity_over_at_most_four_joints():
    for M, V, J, K in [(300, 97, 24, 4), (300, 97, 64, 8), (300, 97, 4, 4), (300, 9, 5, 8), (300, 97, 1, 4), (300, 97, 24, 1)]:
        case = R.make_case(M, V, J, K)
        out = R.bind(case["X"], case["P"][0], case["W"], case["A"][0], case["N"], K)
        assert (out["dense"] >= 0).all() and np.abs(out["dense"].sum(axis=1) - 1).max() < 1e-12
        assert ((out["dense"] > 0).sum(axis=1) <= 4).all()
        assert (np.diff(out["weights"], axis=1) <= 0).all() and (out["joints"][out["weights"] == 0] == 0).all()
        assert np.array_equal(R.dense_weights(out["joints"], out["weights"], J), out["dense"])
        assert ((out["joints"] >= 0) & (out["joints"] < J)).all()
        assert np.abs(np.linalg.norm(out["rest_normals"], axis=1) - 1).max() < 1e-12


def test_round_trip_in_float64():
    case = R.make_case(300, 97, 24, 4, n_poses=3)
    out = R.bind(case["X"], case["P"][0], case["W"], case["A"][0], case["N"], 4)
    vertices, normals = R.pose(out["rest_vertices"], out["joints"], out["weights"], case["A"], out["rest_normals"])
    assert vertices.shape == normals.shape == (3, 300, 3)
    assert np.abs(vertices[0] - case["X"]).max() < 1e-12
    assert np.abs(normals[0] - case["N"].astype(f64) / np.linalg.norm(case["N"].astype(f64), axis=1, keepdims=True)).max() < 1e-12
    assert np.abs(vertices[1] - case["X"]).max() > 1e-2                       # another pose is another mesh
    # posing is linear blend skinning with the dense weights
    T = np.einsum("vj,njab->nvab", out["dense"], case["A"].astype(f64))
    lbs = (T[..., :3, :3] @ out["rest_vertices"][None, :, :, None])[..., 0] + T[..., :3, 3]
    assert np.abs(lbs - vertices).max() < 1e-12


def _line(start, direction, steps):
    return np.stack([np.asarray(start, dtype=f64) + t * np.asarray(direction, dtype=f64) for t in steps])


def test_continuous_across_a_neighbour_swap():
    """K = 2: at t = 0 the second and the third nearest vertex trade places (equal distance) and carry quite different weights.  a_2 is
    the difference of two inverse squared distances whose derivative along the path is below 2 . 0.7 / 0.58^2 each, and a_1 = 1/0.18 -
    1/0.58 = 3.8: the weights move by less than 10 per unit of t."""
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], dtype=f64)
    W = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 0]], dtype=f64)
    A = R.make_rig(4, 3, seed=1)["A"][0]
    for h in (1e-3, 1e-5, 1e-7):
        out = R.bind(_line((0.3, 0.3, 0), (0, 1, 0), (-h, h)), P, W, A, K=2, eps=1e-8)
        assert out["neighbours"][0, 1] == 1 and out["neighbours"][1, 1] == 2              # the swap happens
        assert np.abs(out["dense"][0] - out["dense"][1]).max() <= 10 * 2 * h
        assert np.abs(out["rest_vertices"][0] - out["rest_vertices"][1]).max() <= 100 * 2 * h
    far = R.bind(_line((0.3, 0.3, 0), (0, 1, 0), (-0.2, 0.2)), P, W, A, K=2)
    assert np.abs(far["dense"][0] - far["dense"][1]).max() > 0.1                          # the neighbours do differ


def test_continuous_across_a_joint_swap():
    """J = 6, K = 2: the two neighbours share joints 0..2 and carry 0.1 on joint 3 and on joint 4 respectively; where their blend
    weights cross, the fourth and the fifth largest joint trade places.  The subtracted fifth value makes the leaving joint's weight 0
    at the swap."""
    P = np.array([[0, 0, 0], [1, 0, 0], [0.5, 3, 0], [9, 9, 9]], dtype=f64)
    W = np.array([[.4, .3, .2, .1, 0, 0], [.4, .3, .2, 0, .1, 0], [0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 1]], dtype=f64)
    A = R.make_rig(4, 6, seed=2)["A"][0]
    for h in (1e-3, 1e-5, 1e-7):
        out = R.bind(_line((0.5, 0.2, 0), (1, 0, 0), (-h, h)), P, W, A, K=2, eps=1e-8)
        kept = [set(j[w > 0]) for j, w in zip(out["joints"], out["weights"])]
        assert kept == [{0, 1, 2, 3}, {0, 1, 2, 4}]
        assert np.abs(out["dense"][0] - out["dense"][1]).max() <= 10 * 2 * h
        assert np.abs(out["rest_vertices"][0] - out["rest_vertices"][1]).max() <= 100 * 2 * h


@pytest.mark.parametrize("K", [1, 4, 7])
def test_degenerate_rule_on_the_lattice(K):
    case = R.lattice_case(K)
    for dtype in (f32, f64):
        order, d2 = R.neighbours(case["X"], case["P"], K, dtype)
        assert (d2 == dtype(0.1875)).all()                                               # exact in both formats
        assert np.array_equal(order[:, :K], case["corners"][:, :K])                      # the K lowest-index ties
        w, _ = R.blend_weights(case["X"], case["P"], case["W"], K, 1e-8, dtype)
        assert np.abs(w - case["W"][case["corners"][:, :K]].astype(f64).mean(axis=1)).max() < 1e-6
    out = R.bind(case["X"], case["P"], case["W"], case["A"][0], K=K)
    assert np.isfinite(out["rest_vertices"]).all() and np.abs(out["dense"].sum(axis=1) - 1).max() < 1e-12


def test_every_gpu_case_has_a_bar_under_its_cap():
    """A near-degenerate pool would widen a bar until it hides a failure: every case's bar for weights and rest positions is <= 1e-4."""
    for M, V, J, K in R.CASES:
        case = R.make_case(M, V, J, K)
        assert len(case["X"]) >= R.POOL
        hi, bars = R.case_bars(case)
        print(f"M={M} V={V} J={J} K={K}: bars {bars}, min |det| {np.abs(hi['det']).min():.3f}")
        assert bars["dense"] <= 1e-4 and bars["rest_vertices"] <= 1e-4
        assert np.abs(hi["det"]).min() > 0.1
    for K in (1, 4, 7):
        case = R.lattice_case(K)
        assert len(case["X"]) >= R.POOL
        lo, hi = (R.bind(case["X"], case["P"], case["W"], case["A"][0], K=K, dtype=d) for d in (f32, f64))
        assert R.bar_of(lo["dense"], hi["dense"]) <= 1e-4 and R.bar_of(lo["rest_vertices"], hi["rest_vertices"]) <= 1e-4
        decided = R.decided_rows(R.blend_weights(case["X"], case["P"], case["W"], K, 1e-8, f64)[0])
        print(f"lattice K={K}: {decided.mean():.3f} of the joint sets decided")
        assert decided.mean() >= 0.9                                                     # the exact comparison of joint sets has rows


# ---------------------------------------------------------------------------------------------------------------------- glTF
def avatar(n_poses=4, M=200, J=24, seed=3):
    case = R.make_case(M, 97, J, 4, n_poses=n_poses)
    out = R.bind(case["X"], case["P"][0], case["W"], case["A"][0], case["N"], 4)
    rng = np.random.default_rng(seed)
    faces = rng.integers(len(case["X"]), size=(50, 3))
    colors = rng.uniform(-1, 1, size=(len(case["X"]), 3))
    return case, out, faces, colors


def test_glb_plays_back_as_float64_skinning(tmp_path):
    case, out, faces, colors = avatar()
    path = str(tmp_path / "a.glb")
    mesh_io.write_glb(path, out["rest_vertices"], faces, out["joints"], out["weights"], case["rest_joints"], case["parents"],
                      normals=out["rest_normals"], colors=colors, frames=case["A"], fps=20)
    glb = R.Glb(path)
    assert np.array_equal(glb.faces(), faces) and np.array_equal(glb.attribute("JOINTS_0"), out["joints"])
    assert np.array_equal(glb.attribute("POSITION"), out["rest_vertices"].astype(f32))
    assert np.array_equal(glb.attribute("WEIGHTS_0"), out["weights"].astype(f32))
    assert np.allclose(glb.keys(), np.arange(4) / 20.0, rtol=1e-7, atol=0)
    rest32, w32 = out["rest_vertices"].astype(f32), out["weights"].astype(f32)
    expected, _ = R.pose(rest32, out["joints"], w32, case["A"], dtype=f64)
    bar = R.evaluator_bar(case["parents"], expected)
    assert bar < 1e-4
    for key in range(4):
        err = np.abs(glb.skinned(key) - expected[key]).max()
        print(f"key {key}: err {err:.2e} bar {bar:.2e}")
        assert err <= bar
    assert np.abs(expected[0] - case["X"]).max() < 1e-5                                   # key 0 is the bound mesh
    assert np.abs(glb.skinned(None) - rest32).max() <= bar                                # at rest the skin is the identity
    # consecutive quaternion keys never flip sign
    anim = glb.json["animations"][0]
    for ch in anim["channels"]:
        if ch["target"]["path"] == "rotation":
            q = glb.accessor(anim["samplers"][ch["sampler"]]["output"]).astype(f64)
            assert np.abs(np.linalg.norm(q, axis=1) - 1).max() < 1e-6 and ((q[1:] * q[:-1]).sum(axis=1) >= 0).all()
    assert sum(ch["target"]["path"] == "translation" for ch in anim["channels"]) == 1


def test_glb_structure(tmp_path):
    case, out, faces, colors = avatar(n_poses=2, M=7)
    path = str(tmp_path / "b.glb")
    mesh_io.write_glb(path, out["rest_vertices"][:7], faces % 7, out["joints"][:7], out["weights"][:7], case["rest_joints"],
                      case["parents"], colors=colors[:7], frames=case["A"])
    raw = open(path, "rb").read()
    magic, version, total = struct.unpack_from("<III", raw, 0)
    assert raw[:4] == b"glTF" and magic == 0x46546C67 and version == 2 and total == len(raw)
    n_json, kind = struct.unpack_from("<II", raw, 12)
    assert kind == 0x4E4F534A and n_json % 4 == 0
    n_bin, kind = struct.unpack_from("<II", raw, 20 + n_json)
    assert kind == 0x004E4942 and n_bin % 4 == 0 and 28 + n_json + n_bin == total
    doc = json.loads(raw[20:20 + n_json])
    assert doc["asset"]["version"] == "2.0" and doc["buffers"] == [{"byteLength": n_bin}]
    assert all(v["byteOffset"] % 4 == 0 for v in doc["bufferViews"])
    prim = doc["meshes"][0]["primitives"][0]
    assert set(prim["attributes"]) == {"POSITION", "COLOR_0", "JOINTS_0", "WEIGHTS_0"}         # no normals given, none written
    position = doc["accessors"][prim["attributes"]["POSITION"]]
    assert position["min"] == [float(x) for x in out["rest_vertices"][:7].astype(f32).min(axis=0)]
    assert position["max"] == [float(x) for x in out["rest_vertices"][:7].astype(f32).max(axis=0)]
    joints = doc["accessors"][prim["attributes"]["JOINTS_0"]]
    assert joints["componentType"] == 5121 and joints["type"] == "VEC4"                        # 7 vertices x 4 bytes: padded views follow
    assert doc["accessors"][prim["indices"]]["componentType"] == 5125
    J = len(case["parents"])
    assert doc["skins"][0]["joints"] == list(range(J)) and len(doc["nodes"]) == J + 1
    for j, p in enumerate(case["parents"]):
        want = case["rest_joints"][j] - (case["rest_joints"][p] if p >= 0 else 0)
        assert np.allclose(doc["nodes"][j]["translation"], want, rtol=1e-6, atol=1e-7)
        assert p < 0 or j in doc["nodes"][p]["children"]
    inverse_bind = R.Glb(path).accessor(doc["skins"][0]["inverseBindMatrices"]).reshape(J, 4, 4)      # column-major rows = columns
    assert np.allclose(inverse_bind[:, 3, :3], -case["rest_joints"], rtol=1e-6, atol=1e-7) and (inverse_bind[:, :3, 3] == 0).all()
    # without frames there is no animation
    mesh_io.write_glb(path, out["rest_vertices"][:7], faces % 7, out["joints"][:7], out["weights"][:7], case["rest_joints"], case["parents"])
    assert "animations" not in R.Glb(path).json


def test_glb_refusals(tmp_path):
    case, out, faces, colors = avatar(n_poses=2)
    path = str(tmp_path / "c.glb")
    good = dict(vertices=out["rest_vertices"], faces=faces, joints=out["joints"], weights=out["weights"],
                rest_joints=case["rest_joints"], parents=case["parents"], frames=case["A"])

    def refused(match, **change):
        with pytest.raises(ValueError, match=match):
            mesh_io.write_glb(path, **dict(good, **change))

    refused("vertices", vertices=out["rest_vertices"][:, :2])
    refused("faces", faces=faces[:, :2])
    refused("face index", faces=faces + len(case["X"]))
    refused("joints", joints=out["joints"][:-1])
    refused("joints outside", joints=out["joints"] + 24)
    refused("weights", weights=out["weights"][:, :3])
    refused("normals", normals=out["rest_normals"][:-1])
    refused("colors", colors=colors[:-1])
    refused("parents", parents=case["parents"][:-1])
    refused(r"parents\[3\]", parents=case["parents"][:3] + [5] + case["parents"][4:])
    refused("frames", frames=case["A"][:, :-1])
    refused("fps", fps=0)
    sheared = case["A"].copy()
    sheared[1, 5, 0, 1] += 0.01                                                            # joint 5, frame 1: not a rotation
    refused("joint 5 in frame 1", frames=sheared)
    moved = case["A"].copy()
    moved[0, 7, :3, 3] += 0.01                                                             # joint 7 slides against its parent
    refused("joint 7 in frame 0", frames=moved)
    mirrored = case["A"].copy()
    mirrored[1, 0, :3, 0] *= -1
    refused("joint 0 in frame 1", frames=mirrored)


def test_argument_validation_needs_no_gpu():
    build = importlib.import_module("3dhumangan_amd._build")
    sig = importlib.import_module("3dhumangan_amd._lib")._SIGNATURES
    lib = ctypes.CDLL(build.build_lib())
    lib.h3d_last_error.restype = ctypes.c_char_p
    for name in ("h3d_mesh_bind", "h3d_mesh_pose"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = sig[name]
    p = ctypes.c_void_p(16)
    bind = lambda M, V, J, K, eps: lib.h3d_mesh_bind(p, None, M, p, p, p, V, J, K, eps, p, None, p, p, p, None)   # noqa: E731
    assert bind(1, 10, 24, 9, 1e-8) == -1 and b"K=9" in lib.h3d_last_error()
    assert bind(1, 10, 24, 0, 1e-8) == -1 and b"K=0" in lib.h3d_last_error()
    assert bind(1, 4, 24, 4, 1e-8) == -1 and b"V=4" in lib.h3d_last_error()
    assert bind(1, 10, 65, 4, 1e-8) == -1 and b"J=65" in lib.h3d_last_error()
    assert bind(1, 10, 24, 4, 0.0) == -1 and b"eps" in lib.h3d_last_error()
    assert bind(-1, 10, 24, 4, 1e-8) == -1 and b"M=-1" in lib.h3d_last_error()
    assert lib.h3d_mesh_bind(p, p, 1, p, p, p, 10, 24, 4, 1e-8, p, None, p, p, p, None) == -1 and b"go together" in lib.h3d_last_error()
    assert bind(0, 10, 24, 4, 1e-8) == 0                                                   # M = 0 launches nothing
    assert lib.h3d_mesh_pose(p, None, p, p, 0, p, 3, 24, p, None, None) == 0
    assert lib.h3d_mesh_pose(p, None, p, p, 1, p, 3, 0, p, None, None) == -1 and b"J=0" in lib.h3d_last_error()
    assert lib.h3d_mesh_pose(p, p, p, p, 1, p, 3, 24, p, None, None) == -1 and b"go together" in lib.h3d_last_error()
