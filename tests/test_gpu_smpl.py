"""The SMPL forward on the device (csrc/smpl_lbs.hip through lib/components/smpl.py) against the float64 restatement
(tests/_smpl_reference.py) and the reference's own lbs() (golden fixture); determinism and item invariance; smpl_conditions
against the per-record front-end; the sample app's pose sequences.

Tolerance.  Per case the bar is FACTOR = 8 times the rounding of the fp32 evaluation of the restatement against its float64
evaluation on the case's own inputs (the largest, over the five outputs, of max|fp32 - float64| / max|float64|), applied to each
output relative to that output's maximum.  The factor covers another summation order in the (J-1)*9- and J-term sums, FMA
contraction and a few ulp between device and host sine / cosine.  The bar is capped at CAP = 1e-5, and a case whose fp32
composition alone loses more than that fails (tests/test_smpl_cpu.py checks the whole grid for that on the CPU).

Measured on an MI355X over the 1296 cases of the grid (error / output maximum): A <= 1.8e-6 (the 54-deep chain; 3.6e-7 at SMPL's
tree), verts <= 1.0e-6, J_transformed <= 1.3e-6, v_shaped <= 9.5e-8, J <= 1.0e-7; never above 0.43 of the case's bar."""
import importlib

import numpy as np
import pytest
import torch

import _smpl_reference as SR
from conftest import load_golden

smpl = importlib.import_module("3dhumangan_amd.lib.components.smpl")
conditions = importlib.import_module("3dhumangan_amd.lib.data.conditions")
synthetic = importlib.import_module("3dhumangan_amd.synthetic")

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _forward(body, case):
    """SMPL.forward on a case of the grid -> its five outputs in lbs() order, and the translation on the device."""
    B = case["pose"].shape[0]
    pose, tr = case["pose"].to(DEV), None if case["transl"] is None else case["transl"].to(DEV)
    if case["pose2rot"]:
        go, bp = pose[:, :3], pose[:, 3:]
    else:
        go, bp = pose[:, :1], pose[:, 1:]
    out = body.forward(case["betas"].to(DEV), bp, go, transl=tr, pose2rot=case["pose2rot"])
    assert out["vertices"].shape == (B, body.num_vertices, 3) and out["fk_matrices"].shape == (B, body.num_joints, 4, 4)
    return out["fk_matrices"], out["tpose_vertices"], out["vertices"], out["joints_shaped"], out["joints"], tr


def _check(got, case, where):
    """The five device outputs against the float64 restatement under the case's own bar; -> the worst error / bar ratio."""
    o64, err32 = SR.composition_error(case)
    assert err32 <= SR.CAP, (where, err32)
    if case["transl"] is not None:                  # SMPL.forward moves the posed joints too; lbs() moves the vertices alone
        o64 = list(o64[:4]) + [o64[4] + case["transl"].double()[:, None]]
    bar = min(SR.FACTOR * err32, SR.CAP)
    worst = 0.0
    for name, g, w in zip(SR.OUTPUTS, got, o64):
        assert g.dtype == torch.float32 and g.shape == w.shape, (where, name)
        e = float((g.cpu().double() - w).abs().max() / w.abs().max())
        print(f"{where} {name}: err {e:.2e} bar {bar:.2e}")
        assert e <= bar, (where, name, e, bar)
        worst = max(worst, e / bar)
    return worst


@pytest.mark.parametrize("tree", SR.TREES)
@pytest.mark.parametrize("n_j", SR.GRID_J)
@pytest.mark.parametrize("V", SR.GRID_V)
def test_parity_with_the_float64_restatement(V, n_j, tree):
    """B in {1, 3, 9}: smaller than the item tile of 8, and 9 = one full tile and a tail of one; NB in {0, 1, 10, 17}; both pose
    forms; with and without translation.  Item 0 of every case has an exactly zero pose, the last item a joint at pi - 1e-4."""
    for NB in SR.GRID_NB:
        body = None
        for B in SR.GRID_B:
            for pose2rot in (True, False):
                for with_transl in (False, True):
                    case = SR.make_case(V, B, NB, n_j, pose2rot, with_transl, tree)
                    if body is None:
                        body = smpl.SMPL(case["model"], device=DEV)
                    A, v_shaped, verts, joints, posed, tr = _forward(body, case)
                    where = f"V={V} J={n_j} {tree} NB={NB} B={B} pose2rot={pose2rot} transl={with_transl}"
                    _check((A, v_shaped, verts, joints, posed), case, where)
                    if pose2rot and B > 1:                              # the exactly zero pose: identity rotations, bit for bit
                        assert torch.equal(A[0, :, :3, :3].cpu(), torch.eye(3).expand(n_j, 3, 3))


def test_lbs_matches_the_reference_golden():
    g = load_golden("smpl_lbs_tiny")
    m = g["model"]
    dev_model = [m[k].to(DEV) for k in SR.MODEL_KEYS]
    for tag, pose2rot in (("aa", True), ("mat", False)):
        c = g[tag]
        got = smpl.lbs(c["betas"].to(DEV), c["pose"].to(DEV), *dev_model, pose2rot=pose2rot)
        _, err32 = SR.composition_error({"model": m, "betas": c["betas"], "pose": c["pose"], "pose2rot": pose2rot, "transl": None})
        assert err32 <= SR.CAP
        bar = min(SR.FACTOR * err32, SR.CAP)
        for name, x in zip(SR.OUTPUTS, got):
            e = float((x.cpu().double() - c[name]).abs().max() / c[name].abs().max())
            print(f"golden {tag} {name}: err {e:.2e} bar {bar:.2e}")
            assert x.shape == c[name].shape and e <= bar, (tag, name, e, bar)


def test_full_size():
    case = SR.make_case(6890, 16, 10, 24, True, True, "smpl", seed=1)
    body = smpl.SMPL(case["model"], device=DEV, vertex_joint_ids=[331, 2802, 6262, 3336, 3346])
    A, v_shaped, verts, joints, posed, tr = _forward(body, case)
    assert posed.shape == (16, 29, 3)
    assert torch.equal(posed[:, 24:], verts[:, [331, 2802, 6262, 3336, 3346]])          # the appended vertex joints
    _check((A, v_shaped, verts, joints, posed[:, :24]), case, "V=6890 B=16")


def test_two_runs_are_bit_identical_and_items_do_not_see_their_batch():
    case = SR.make_case(301, 9, 10, 24, True, True, "smpl", seed=4)
    body = smpl.SMPL(case["model"], device=DEV)
    first, second = _forward(body, case)[:5], _forward(body, case)[:5]
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    for i in range(9):
        one = dict(case, betas=case["betas"][i:i + 1], pose=case["pose"][i:i + 1], transl=case["transl"][i:i + 1])
        for name, a, b in zip(SR.OUTPUTS, _forward(body, one)[:5], first):
            assert torch.equal(a[0], b[i]), (i, name)
    # a batch-1 betas is expanded over the poses
    shared = dict(case, betas=case["betas"][:1])
    out = _forward(body, shared)
    assert torch.equal(out[1][5], first[1][0]) and torch.equal(out[1][0], first[1][0])


def test_ops_refuse_what_they_cannot_do():
    case = SR.make_case(67, 2, 10, 24, True, False, "smpl")
    body = smpl.SMPL(case["model"], device=DEV)
    betas, pose = case["betas"].to(DEV), case["pose"].to(DEV)
    with pytest.raises(RuntimeError, match="SMPL.forward is not differentiable"):
        body.forward(betas.clone().requires_grad_(True), pose[:, 3:], pose[:, :3])
    with torch.no_grad():
        body.forward(betas.clone().requires_grad_(True), pose[:, 3:], pose[:, :3])
    with pytest.raises(ValueError, match="pose must hold"):
        body.forward(betas, pose[:, 6:], pose[:, :3])
    with pytest.raises(ValueError, match=r"parents\[5\]"):
        bad = case["model"]["parents"].clone()
        bad[5] = 5
        smpl.lbs(betas, pose, *[(bad if k == "parents" else case["model"][k]).to(DEV) for k in SR.MODEL_KEYS])


def test_smpl_conditions_matches_the_record_front_end():
    """smpl_conditions on the device against preprocess_smpl_fix_body (CPU, float64 inside, pinned to the reference by
    frontend.npz) fed item by item with the same SMPL outputs.  The small matrices are float64 on both sides: equal to float32
    rounding.  The vertices pass through the fp32 skinning kernel: at most J products-and-adds in the blend, four in the transform
    and three in the rigid product, each rounded once, on convex weights -- (J + 7) 2^-24 of the largest coordinate."""
    B, V, n_j = 5, 301, 24
    case = SR.make_case(V, B, 10, n_j, True, False, "smpl", seed=6)
    case["pose"][0, :3] = torch.tensor([0.3, -0.2, 0.5])
    m = case["model"]
    body = smpl.SMPL(m, device=DEV, vertex_joint_ids=[3, 17])
    pose = case["pose"].to(DEV)
    out = body.forward(case["betas"].to(DEV), pose[:, 3:], pose[:, :3])
    cam = torch.tensor([[1.6, 1.6, 0.0, 0.0], [1.2, 1.2, 0.1, -0.2], [2.0, 2.0, -0.3, 0.05], [0.9, 0.9, 0.0, 0.4], [1.0, 1.0, 0.2, 0.2]])
    idx = [0, 5, 23, 7, 25, 12]
    got = conditions.smpl_conditions(out, cam.to(DEV), idx, m["v_template"])
    assert got["vertices"].is_cuda and got["lbs_weights"].shape == (B, V, n_j) and got["scales"].shape == (B,)
    for b in range(B):
        rec = {"orig_cam": cam[b:b + 1].numpy(), "joints": out["joints"][b:b + 1].cpu().numpy(),
               "full_pose": got["full_pose"][b:b + 1].cpu().numpy(), "tpose_vertices": out["tpose_vertices"][b:b + 1].cpu().numpy(),
               "fk_matrices": out["fk_matrices"][b:b + 1].cpu().numpy(), "lbs_weights": m["lbs_weights"].numpy()}
        want = conditions.preprocess_smpl_fix_body(rec, idx, m["v_template"])
        assert set(want) == set(got)
        for k, w in want.items():
            g = got[k][b].cpu()
            assert g.shape == w.shape and g.dtype == w.dtype, (b, k)
            if k == "vertices":
                e, bar = float((g - w).abs().max()), (n_j + 7) * 2.0 ** -24 * float(w.abs().max())
                print(f"smpl_conditions vertices item {b}: err {e:.2e} bar {bar:.2e}")
                assert e <= bar, (b, e, bar)
            else:
                assert torch.allclose(g, w, rtol=1e-6, atol=1e-7), (b, k)
    # the rotation of the root really is undone: its canonical frame differs from an unrotated item's
    assert not torch.allclose(got["cano_matrices"][0], got["cano_matrices"][1])


def _tiny_config():
    configs = importlib.import_module("3dhumangan_amd.configs")
    cfg = dict(load_golden("gen_tiny_mixed")["meta"])
    cfg.update(neural_field_cls="COORDCONCATSIREN", name="tiny_pose")
    configs.TINY_POSE = cfg
    return cfg


def test_app_pose_sequence(tmp_path):
    from PIL import Image
    app = importlib.import_module("3dhumangan_amd.apps.sample_from_generator")
    cfg = _tiny_config()
    H, W = cfg["gen_height"], cfg["gen_width"]
    # the tiny fixture's conditioned weights: the same generator in every run, and one whose image depends on its inputs (a
    # random-init generator of this size paints a nearly flat image, which uint8 frames cannot tell apart)
    ckpt = str(tmp_path / "tiny_state_dict.pth")
    torch.save(load_golden("gen_tiny_mixed")["state"], ckpt)
    out_dir = app.main(["--config", "TINY_POSE", "--checkpoint", ckpt, "--dataset_length", "4", "--pose-sequence", "synthetic", "--n_poses", "3", "--seeds", "3",
                        "--save", "png", "--output_dir", str(tmp_path / "a")])
    frames = np.asarray(Image.open(f"{out_dir}/003_uncond.png")).astype(np.float64)
    sem = np.asarray(Image.open(f"{out_dir}/003_smpl.png"))
    assert frames.shape == (H, 3 * W, 3) and sem.shape == (H, 3 * W, 3) and np.isfinite(frames).all() and frames.std() > 0
    assert not np.array_equal(frames[:, :W], frames[:, W:2 * W]) and not np.array_equal(frames[:, W:2 * W], frames[:, 2 * W:])
    assert (sem != 255).any()                                                   # the rasteriser drew the posed body
    # a sequence and a model from files, the first pose repeated as the third; the camera stays fixed
    seq = synthetic.make_pose_sequence(3, seed=1, pose_scale=1.0)
    seq["poses"][2], seq["orig_cam"][2] = seq["poses"][0], seq["orig_cam"][0]
    np.savez(str(tmp_path / "seq.npz"), **seq)
    np.savez(str(tmp_path / "model.npz"), **synthetic.make_smpl_model(seed=2))
    out_dir = app.main(["--config", "TINY_POSE", "--checkpoint", ckpt, "--dataset_length", "4", "--smpl-model", str(tmp_path / "model.npz"), "--pose-sequence",
                        str(tmp_path / "seq.npz"), "--seeds", "5", "--save", "png", "--output_dir", str(tmp_path / "b")])
    frames = np.asarray(Image.open(f"{out_dir}/005_uncond.png"))
    sem = np.asarray(Image.open(f"{out_dir}/005_smpl.png"))
    assert frames.shape == (H, 3 * W, 3)
    assert np.array_equal(frames[:, :W], frames[:, 2 * W:]) and not np.array_equal(frames[:, :W], frames[:, W:2 * W])
    assert np.array_equal(sem[:, :W], sem[:, 2 * W:]) and not np.array_equal(sem[:, :W], sem[:, W:2 * W])
