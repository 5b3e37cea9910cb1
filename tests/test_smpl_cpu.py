"""CPU side of the SMPL forward: the float64 restatement (tests/_smpl_reference.py) against the reference's own lbs() (golden
fixture) and against synthetic.forward_kinematics, the host-side pieces of lib/components/smpl.py (validation, the joint-regressor
fold), the synthetic model, the front-end formulas of smpl_conditions, the app's pose-sequence flags and the C ABI entries."""
import importlib
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import _smpl_reference as SR
from conftest import GOLDEN, ROOT, load_golden

sys.path.insert(0, GOLDEN)
from _stub_generator import StubGenerator, StubPreprocessor  # noqa: E402

smpl = importlib.import_module("3dhumangan_amd.lib.components.smpl")
conditions = importlib.import_module("3dhumangan_amd.lib.data.conditions")
synthetic = importlib.import_module("3dhumangan_amd.synthetic")
app = importlib.import_module("3dhumangan_amd.apps.sample_from_generator")
_lib = importlib.import_module("3dhumangan_amd._lib")


def test_restatement_matches_the_reference_lbs():
    g = load_golden("smpl_lbs_tiny")
    m = g["model"]
    assert m["v_template"].shape == (67, 3) and m["shapedirs"].shape == (67, 3, 10) and m["posedirs"].shape == (207, 201)
    for tag, pose2rot in (("aa", True), ("mat", False)):
        c = g[tag]
        assert c["betas"].shape == (3, 10)
        out = SR.lbs(c["betas"].double(), c["pose"].double(), *(m[k] for k in SR.MODEL_KEYS), pose2rot=pose2rot)
        for name, got in zip(SR.OUTPUTS, out):
            assert got.shape == c[name].shape, name
            assert float((got - c[name]).abs().max()) <= 1e-6, (tag, name)
    # the two halves are different poses, so a mix-up of the flag would show
    assert not torch.allclose(g["aa"]["verts"], g["mat"]["verts"], atol=1e-3)


def test_restatement_matches_synthetic_forward_kinematics():
    """betas = 0, posedirs = 0, a regressor that picks the rest joints out of the template: the restatement is then the procedural
    body's forward kinematics and skinning.  The synthetic side is fp32 with chains up to nine products deep on values of scale
    1: a few ulp of 1, bounded here by 1e-6."""
    J, V, W = synthetic.template_body(n_vertices=200, seed=3)
    g = torch.Generator().manual_seed(5)
    aa = (torch.rand(24, 3, generator=g) - 0.5) * 2.0
    A_syn, posed_syn = synthetic.forward_kinematics(J, synthetic._axis_angle_to_matrix(aa))
    VA = torch.einsum("vj,jab->vab", W, A_syn)
    verts_syn = torch.einsum("vab,vb->va", VA, torch.cat([V, torch.ones(200, 1)], 1))[:, :3]
    v_template = torch.cat([J, V])
    reg = torch.cat([torch.eye(24), torch.zeros(24, 200)], dim=1)
    weights = torch.cat([torch.eye(24), W])
    A, v_shaped, verts, joints, posed = SR.lbs(torch.zeros(1, 0, dtype=torch.float64), aa.double().reshape(1, 72), v_template,
                                               torch.zeros(224, 3, 0), torch.zeros(207, 672), reg, synthetic.PARENTS, weights)
    assert float((A[0] - A_syn).abs().max()) <= 1e-6
    assert float((posed[0] - posed_syn).abs().max()) <= 1e-6
    assert float((joints[0] - J).abs().max()) == 0.0
    assert float((verts[0, 24:] - verts_syn).abs().max()) <= 1e-6
    assert float((verts[0, :24] - posed_syn).abs().max()) <= 1e-6          # a vertex bound to one joint, sitting on it, moves with it


def test_joint_regressor_fold_is_exact_algebra():
    m = SR.make_model(301, 24, 10, "smpl", seed=2)
    betas = torch.randn(5, 10, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    jt, jd = smpl.fold_joint_regressor(m["J_regressor"], m["v_template"], m["shapedirs"])
    assert jt.dtype == torch.float64 and jt.shape == (24, 3) and jd.shape == (24, 3, 10)
    v_shaped = m["v_template"].double()[None] + torch.einsum("bl,mkl->bmk", betas, m["shapedirs"].double())
    want = torch.einsum("bik,ji->bjk", v_shaped, m["J_regressor"].double())
    got = jt[None] + torch.einsum("jkl,bl->bjk", jd, betas)
    assert float((got - want).abs().max()) <= 1e-12
    jt0, jd0 = smpl.fold_joint_regressor(m["J_regressor"], m["v_template"], torch.zeros(301, 3, 0))
    assert jd0.shape == (24, 3, 0) and torch.equal(jt0, jt)


def test_model_validation_messages():
    m = SR.make_model(67, 24, 10, "smpl")
    args = lambda **kw: [kw.get(k, m[k]) for k in smpl.MODEL_KEYS]                         # noqa: E731
    assert smpl.validate_model(*args()) == (67, 24, 10)
    bad = m["parents"].clone()
    bad[7] = 9
    with pytest.raises(ValueError, match=r"parents\[7\] = 9"):
        smpl.validate_model(*args(parents=bad))
    bad = m["parents"].clone()
    bad[0] = 0
    with pytest.raises(ValueError, match=r"parents\[0\] must be -1"):
        smpl.validate_model(*args(parents=bad))
    bad = m["parents"].clone()
    bad[3] = -1
    with pytest.raises(ValueError, match=r"parents\[3\] = -1"):
        smpl.validate_model(*args(parents=bad))
    with pytest.raises(ValueError, match="parents must have 24 entries"):
        smpl.validate_model(*args(parents=m["parents"][:23]))
    with pytest.raises(ValueError, match="shapedirs must be"):
        smpl.validate_model(*args(shapedirs=m["shapedirs"][:66]))
    with pytest.raises(ValueError, match=r"posedirs must be \[\(J-1\)\*9, V\*3\] = \[207,201\]"):
        smpl.validate_model(*args(posedirs=m["posedirs"].T))
    with pytest.raises(ValueError, match="lbs_weights must be"):
        smpl.validate_model(*args(lbs_weights=m["lbs_weights"][:, :23]))
    with pytest.raises(ValueError, match="J_regressor must be"):
        smpl.validate_model(*args(J_regressor=m["J_regressor"][:, :66]))
    with pytest.raises(ValueError, match="1 <= J <= 64"):
        big = SR.make_model(5, 65, 0, "chain")
        smpl.validate_model(*(big[k] for k in smpl.MODEL_KEYS))
    # the class validates before it touches a device
    with pytest.raises(ValueError, match="missing arrays"):
        smpl.SMPL({"v_template": m["v_template"]})
    with pytest.raises(ValueError, match=r"parents\[0\] must be -1"):
        smpl.SMPL(dict(m, parents=bad.clone().fill_(0)))


def test_ops_refuse_cpu_tensors_and_grad():
    m = SR.make_model(5, 2, 1, "chain")
    c = SR.make_case(5, 1, 1, 2, True, False, "chain")
    with pytest.raises(_lib.H3DError, match="no CPU fallback"):
        smpl.lbs(c["betas"], c["pose"], *(m[k] for k in smpl.MODEL_KEYS))
    with pytest.raises(_lib.H3DError, match="no CPU fallback"):
        smpl.skin_vertices(torch.zeros(1, 5, 3), torch.zeros(1, 2, 4, 4), m["lbs_weights"])
    with pytest.raises(RuntimeError, match="smpl.skin_vertices is not differentiable"):
        smpl._refuse_grad("smpl.skin_vertices", torch.zeros(3, requires_grad=True))
    with torch.no_grad():
        smpl._refuse_grad("smpl.lbs", torch.zeros(3, requires_grad=True))


def test_synthetic_smpl_model_invariants():
    m = synthetic.make_smpl_model(seed=1)
    V = m["v_template"].shape[0]
    assert smpl.validate_model(*(torch.as_tensor(m[k]) for k in smpl.MODEL_KEYS)) == (V, 24, 10)
    reg, w = torch.as_tensor(m["J_regressor"]), torch.as_tensor(m["lbs_weights"])
    assert float((reg.sum(1) - 1).abs().max()) <= 1e-6 and float(reg.min()) >= 0 and int((reg > 0).sum(1).max()) <= 32
    assert float((w.sum(1) - 1).abs().max()) <= 1e-6 and float(w.min()) >= 0
    assert m["faces"].shape == (13776, 3) and int(m["faces"].max()) < V and m["faces_to_labels"].shape == (13776,)
    assert 0 < float(np.abs(m["shapedirs"]).max()) <= 0.02 + 1e-6 and 0 < float(np.abs(m["posedirs"]).max()) < 0.02
    # the regressed joints sit near the rest joints of the tube body
    rest = synthetic.tube_body()[0]
    assert float((reg @ torch.as_tensor(m["v_template"]) - rest).norm(dim=1).max()) < 0.12
    assert all(np.array_equal(a, b) for a, b in zip(m.values(), synthetic.make_smpl_model(seed=1).values()))
    seq = synthetic.make_pose_sequence(6, seed=2)
    assert seq["poses"].shape == (6, 24, 3) and seq["betas"].shape == (1, 10) and seq["orig_cam"].shape == (6, 4)
    assert np.abs(seq["poses"][:, 0]).max() == 0 and np.abs(seq["poses"]).max() <= 0.5
    step = np.abs(np.diff(seq["poses"], axis=0)).max()
    assert 0 < step < 0.5 * 2 * math.pi * 2 / 6 + 1e-6                  # smooth: bounded by amplitude x angular rate x dt
    assert np.array_equal(seq["poses"], synthetic.make_pose_sequence(6, seed=2)["poses"])


def test_smpl_conditions_formulas_match_the_record_front_end():
    """smpl_conditions' torch part and a float64 skinning against preprocess_smpl_fix_body, item by item, on the restatement's
    float64 outputs (rounded to the float32 the record stores)."""
    B, V, n_j = 4, 67, 24
    case = SR.make_case(V, B, 10, n_j, True, False, "smpl", seed=3)
    case["pose"][0, :3] = torch.tensor([0.3, -0.2, 0.5])                                   # item 0: a root rotation, else zero pose
    m = case["model"]
    A, v_shaped, verts, joints, posed = SR.lbs(case["betas"].double(), case["pose"].double(), *(m[k] for k in SR.MODEL_KEYS))
    A, v_shaped, posed = A.float(), v_shaped.float(), posed.float()
    full_pose = SR.batch_rodrigues(case["pose"].double().reshape(-1, 3)).view(B, n_j, 3, 3).float()
    cam = torch.tensor([[1.6, 1.6, 0.0, 0.0], [1.2, 1.2, 0.1, -0.2], [2.0, 2.0, -0.3, 0.05], [0.9, 0.9, 0.0, 0.4]])
    idx = [0, 5, 23, 7, 7, 12]
    got = conditions.smpl_conditions_math(A, posed, full_pose, cam, idx)
    per_vertex = torch.einsum("vj,bjrc->bvrc", m["lbs_weights"].double(), got["fk_matrices"])
    homo = torch.cat([v_shaped.double(), torch.ones(B, V, 1, dtype=torch.float64)], dim=2)
    got["vertices"] = torch.einsum("bvrc,bvc->bvr", per_vertex, homo)[..., :3]
    for b in range(B):
        rec = {"orig_cam": cam[b:b + 1].numpy(), "joints": posed[b:b + 1].numpy(), "full_pose": full_pose[b:b + 1].numpy(),
               "tpose_vertices": v_shaped[b:b + 1].numpy(), "fk_matrices": A[b:b + 1].numpy(), "lbs_weights": m["lbs_weights"].numpy()}
        want = conditions.preprocess_smpl_fix_body(rec, idx, m["v_template"])
        for k in ("scales", "skeletons_xyz", "intrinsics", "vertices", "fk_matrices", "cano_matrices", "T"):
            assert torch.allclose(got[k][b].float(), want[k], rtol=1e-6, atol=1e-7), (b, k)
    assert not torch.allclose(got["cano_matrices"][0, :3, :3], got["cano_matrices"][1, :3, :3])


def test_every_grid_case_stays_under_the_cap():
    """The GPU tests' bar is FACTOR x the fp32 composition's own error per case; a case whose composition alone loses more than
    CAP would make that bar meaningless.  Every case of the grid, on the CPU."""
    worst = 0.0
    n = 0
    for V, B, NB, n_j, pose2rot, with_transl, tree in SR.grid():
        _, err = SR.composition_error(SR.make_case(V, B, NB, n_j, pose2rot, with_transl, tree))
        assert 0 < err <= SR.CAP, (V, B, NB, n_j, pose2rot, with_transl, tree, err)
        worst, n = max(worst, err), n + 1
    assert n == 3 * 3 * 4 * 3 * 2 * 2 * 3
    print(f"fp32 composition error over {n} cases: worst {worst:.2e}")


def test_app_pose_sequence_flags_with_a_stub_generator():
    cfg = dict(latent_dim=16, gen_height=12, gen_width=6)
    cond = {"scales": torch.ones(3), "dummy": torch.arange(18.0).view(3, 6)}
    G = StubGenerator()
    pan, tilt = app.camera_sweep(2, 0.5, 0.2, False)
    frames, sem = app.generate_pose_frames(G, StubPreprocessor(), cfg, 7, cond, pan, tilt)
    assert frames.dtype == np.uint8 and frames.shape == (3, 12, 6, 3) and sem.shape == (3, 12, 6, 3)
    assert len(G.calls) == 3 and all(torch.equal(c[0], G.calls[0][0]) for c in G.calls)     # one latent for the whole strip
    assert [float(c[1][0, 0, 3]) for c in G.calls] == [float(pan[0]), float(pan[1]), float(pan[0])]      # angle i mod K
    assert np.array_equal(frames[0], frames[2]) and not np.array_equal(frames[0], frames[1])
    # the camera-sweep path is what it was: the same frames as through the shared per-frame helper
    G1, G2 = StubGenerator(), StubGenerator()
    one = {"scales": torch.ones(1), "dummy": torch.arange(6.0).view(1, 6)}
    f1, _ = app.generate_frames(G1, StubPreprocessor(), cfg, 7, one, 2, 0.5, 0.2, False)
    f2, _ = app.generate_pose_frames(G2, StubPreprocessor(), cfg, 7, {k: v.repeat(2, *([1] * (v.dim() - 1))) for k, v in one.items()},
                                     pan, tilt)
    assert np.array_equal(f1, f2)
    for argv in (["--smpl-model", "m.npz"], ["--pose-sequence", "synthetic", "--smpl-record", "r.npz"]):
        with pytest.raises(ValueError, match="--pose-sequence"):
            app.main(argv)
    with pytest.raises(ValueError, match="needs --smpl-model"):
        app.load_pose_sequence(None, "poses.npz", "cpu")


def test_new_abi_entries_match_the_header():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "h3d.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(h3d_smpl_[a-z0-9_]+)\s*\(", text)))
    assert names == ["h3d_smpl_pose", "h3d_smpl_shape", "h3d_smpl_skin"]
    for name in names:
        assert name in _lib._SIGNATURES, name
        n_header = len(re.search(name + r"\s*\(([^)]*)\)", text).group(1).split(","))
        assert n_header == len(_lib._SIGNATURES[name][1]), name
    assert "#define H3D_VERSION 101" in text


def test_c_boundary_refuses_bad_shapes_before_any_launch():
    lib = _lib.load()
    one = torch.zeros(4)
    p = _lib.ptr(one)
    assert lib.h3d_smpl_pose(p, p, p, p, p, p, p, p, p, 1, 65, 0, 1, None) == -1 and b"J=65" in lib.h3d_last_error()
    assert lib.h3d_smpl_pose(p, p, p, p, p, p, p, p, p, 1, 2, 0, 2, None) == -1 and b"pose2rot" in lib.h3d_last_error()
    assert lib.h3d_smpl_shape(p, p, p, p, 0, 5, 1, None) == -1 and b"bad shape" in lib.h3d_last_error()
    assert lib.h3d_smpl_shape(None, None, None, p, 1, 5, 0, None) == -1 and b"null pointer" in lib.h3d_last_error()
    assert lib.h3d_smpl_skin(p, p, None, p, None, None, p, p, 1, 5, 2, None) == -1 and b"go together" in lib.h3d_last_error()
    assert lib.h3d_smpl_skin(p, None, None, p, None, None, p, p, 1, 0, 2, None) == -1 and b"bad shape" in lib.h3d_last_error()
