"""The mesh rasteriser (csrc/mesh_raster.hip) on the device against the float64 restatement of its contract
(tests/_raster_reference.py), its edge cases, determinism, the front-end path and the sample app's `--smpl-record`."""
import argparse
import importlib
import math

import numpy as np
import pytest
import torch

import _raster_reference as RR

synthetic = importlib.import_module("3dhumangan_amd.synthetic")
conditions = importlib.import_module("3dhumangan_amd.lib.data.conditions")
raster = importlib.import_module("3dhumangan_amd.lib.components.raster")

pytestmark = pytest.mark.gpu
F_R = conditions.FOCAL_RASTER


def _views(B, seed, scale, H, W, shift_last=False):
    """The tube body at B different views through the front-end's camera; with `shift_last` the last item is moved sideways
    so that the image border cuts it in half."""
    cond, faces, labels = synthetic.make_mesh_conditions(B, seed=seed, scale=scale)
    if shift_last:
        cond["T"][-1, 0, 3] = W / min(H, W) / (2 * scale)          # x_ndc = -f_r X / Z with Z = f_r / (2 scale): the border
    hs = torch.linspace(-1.2, 2.5, B) if B > 1 else torch.tensor([0.4])
    vs = torch.linspace(-0.3, 0.3, B) if B > 1 else torch.tensor([0.1])
    view = conditions.CameraPreprocessor().forward_with_rotation(cond, hs, vs, torch.zeros(B), gen_height=H, gen_width=W)
    return cond, faces, labels, view["raster_rotation"], conditions.raster_translation(view)


def _compare(verts, faces, R, T, H, W, labels=None, table=None):
    dev = torch.device("cuda")
    frag = raster.rasterize_meshes(verts.to(dev), faces.to(dev), R.to(dev), T.to(dev), -F_R, (H, W))
    B = verts.shape[0]
    assert frag.pix_to_face.shape == (B, H, W, 1) and frag.pix_to_face.dtype == torch.int64
    assert frag.zbuf.shape == (B, H, W, 1) and frag.bary_coords.shape == (B, H, W, 1, 3)
    ref = RR.rasterize(verts, faces, R, T, -F_R, H, W, labels, table)
    p2f, zbuf, bary = frag.pix_to_face[..., 0].cpu(), frag.zbuf[..., 0].cpu().double(), frag.bary_coords[..., 0, :].cpu().double()
    far = ~ref["near"]
    diff = p2f != ref["pix_to_face"]
    covered = int((ref["pix_to_face"] >= 0).sum())
    assert not (diff & far).any(), f"{int((diff & far).sum())} non-near pixels differ"
    assert int(diff.sum()) <= 0.0005 * max(covered, 1), (int(diff.sum()), covered)
    same = (~diff) & (p2f >= 0)
    assert float(((zbuf - ref["zbuf"]).abs() / ref["zbuf"].abs())[same].max()) <= 1e-6
    assert float((bary - ref["bary"]).abs()[same].max()) <= 1e-5
    assert (zbuf[p2f < 0] == -1).all() and (bary[p2f < 0] == -1).all()
    return frag, ref, covered


@pytest.mark.parametrize("B,H,W", [(4, 512, 256), (2, 256, 128), (3, 77, 100)])
def test_parity_with_the_restatement(B, H, W):
    scale = 0.8 if H >= W else 0.5
    cond, faces, labels, R, T = _views(B, seed=B, scale=scale, H=H, W=W, shift_last=True)
    table = cond["tpose_vertices"][0]
    frag, ref, covered = _compare(cond["vertices"], faces, R, T, H, W, labels, table)
    assert covered > 0.03 * B * H * W
    # the shifted item is cut by the image border
    last = ref["pix_to_face"][-1]
    assert (last >= 0).any() and ((last[:, 0] >= 0).any() or (last[:, -1] >= 0).any())
    dev = torch.device("cuda")
    seg, sem = raster.rasterize_segments_semantics(cond["vertices"].to(dev), faces.to(dev), R.to(dev), T.to(dev), -F_R, (H, W),
                                                   labels.to(dev), table.to(dev))
    far = ~ref["near"]
    assert seg.dtype == torch.int64 and torch.equal(seg.cpu()[far], ref["segments"][far])
    far3 = far[:, None].expand(-1, 3, -1, -1)
    assert torch.equal(sem.cpu()[far3], ref["semantics"].float()[far3])


def test_edge_cases():
    dev = torch.device("cuda")
    R, T = torch.eye(3)[None], torch.tensor([[0.0, 0.0, 10.0]])
    # entirely off-image
    verts = torch.tensor([[[5.0, 5.0, 0.0], [6.0, 5.0, 0.0], [5.0, 6.0, 0.0]]])
    frag = raster.rasterize_meshes(verts.to(dev), torch.tensor([[0, 1, 2]], device=dev), R.to(dev), T.to(dev), -10.0, (32, 16))
    assert (frag.pix_to_face == -1).all() and (frag.zbuf == -1).all()
    # B = 1, F = 70 (not a multiple of 64): a fan of triangles, with degenerate ones and out-of-range indices mixed in
    g = torch.Generator().manual_seed(5)
    verts = torch.cat([(torch.rand(1, 40, 2, generator=g) - 0.5) * 1.6, torch.rand(1, 40, 1, generator=g) * 2 - 1], -1)
    faces = torch.randint(0, 40, (70, 3), generator=g, dtype=torch.int64)
    faces[5] = torch.tensor([3, 3, 7])                      # repeated vertex: zero area
    faces[9] = torch.tensor([0, 1, 40])                     # out of range
    faces[11] = torch.tensor([-1, 2, 3])
    faces[13] = torch.tensor([2, 2**30, 3])
    frag, ref, covered = _compare(verts, faces, R, T, 40, 24)
    assert covered > 100
    hit = set(frag.pix_to_face[frag.pix_to_face >= 0].tolist())
    assert not hit & {5, 9, 11, 13}
    # a vertex behind the camera drops the face
    verts2 = verts.clone()
    verts2[0, faces[0, 0], 2] = -20.0
    ref2 = RR.rasterize(verts2, faces, R, T, -10.0, 40, 24)
    frag2 = raster.rasterize_meshes(verts2.to(dev), faces.to(dev), R.to(dev), T.to(dev), -10.0, (40, 24))
    assert 0 not in set(frag2.pix_to_face[frag2.pix_to_face >= 0].tolist()) and 0 not in set(ref2["pix_to_face"].flatten().tolist())


def test_two_calls_are_bit_identical():
    cond, faces, labels, R, T = _views(4, seed=1, scale=0.8, H=512, W=256)
    dev = torch.device("cuda")
    args = (cond["vertices"].to(dev), faces.to(dev), R.to(dev), T.to(dev), -F_R, (512, 256))
    a, b = raster.rasterize_meshes(*args), raster.rasterize_meshes(*args)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    ex = (labels.to(dev), cond["tpose_vertices"][0].to(dev))
    s1, s2 = raster.rasterize_segments_semantics(*args, *ex), raster.rasterize_segments_semantics(*args, *ex)
    assert torch.equal(s1[0], s2[0]) and torch.equal(s1[1], s2[1])


def test_front_end_segments_and_semantics():
    B, H, W = 3, 512, 256
    cond, faces, labels = synthetic.make_mesh_conditions(B, seed=2, scale=0.7)
    dev = torch.device("cuda")
    pre = conditions.CameraPreprocessor(dev)
    pre.init_smpl(faces, labels)
    data = {k: v.to(dev) for k, v in cond.items()}
    hs, vs = torch.tensor([0.0, 0.9, -2.0]), torch.tensor([0.0, 0.2, -0.1])
    out = pre.forward_with_rotation(data, hs, vs, torch.zeros(B), gen_height=H, gen_width=W)
    seg, sem = out["rasterized_segments"], out["rasterized_semantics"]
    assert seg.shape == (B, H, W) and seg.dtype == torch.int64 and sem.shape == (B, 3, H, W)
    bg = seg == 1
    assert bg.any() and (~bg).any()
    assert int(seg[~bg].min()) >= 2 and int(seg[~bg].max()) <= 25
    assert (sem.permute(0, 2, 3, 1)[bg] == 0).all()
    ref = RR.rasterize(cond["vertices"], faces, out["raster_rotation"].cpu(), conditions.raster_translation(out).cpu(), -F_R, H, W,
                       labels, cond["tpose_vertices"][0])
    far = ~ref["near"]
    assert torch.equal(seg.cpu()[far], ref["segments"][far])
    far3 = far[:, None].expand(-1, 3, -1, -1)
    assert torch.equal(sem.cpu()[far3], ref["semantics"].float()[far3])
    # without init_smpl: unchanged behaviour
    plain = conditions.CameraPreprocessor(dev).forward_with_rotation(data, hs, vs, torch.zeros(B), gen_height=H, gen_width=W)
    assert "rasterized_segments" not in plain and (plain["rasterized_semantics"] == 0).all()


def test_app_smpl_record(tmp_path):
    from PIL import Image
    app = importlib.import_module("3dhumangan_amd.apps.sample_from_generator")
    rec = synthetic.make_smpl_record(seed=4)
    path = str(tmp_path / "rec.npz")
    np.savez(path, **rec)
    out_dir = app.main(["--config", "MAP3DBN", "--smpl-record", path, "--n_angles", "2", "--seeds", "3", "--save", "png",
                        "--output_dir", str(tmp_path / "out")])
    cfg = importlib.import_module("3dhumangan_amd.configs").get_config(argparse.Namespace(config="MAP3DBN", tune="", variant=0))
    H, W = cfg["gen_height"], cfg["gen_width"]
    smpl = np.asarray(Image.open(f"{out_dir}/003_smpl.png"))
    frames = np.asarray(Image.open(f"{out_dir}/003_uncond.png"))
    assert smpl.shape == (H, 2 * W, 3) and frames.shape == (H, 2 * W, 3) and frames.std() > 0
    # the restatement at the app's two views
    data_mod = importlib.import_module("3dhumangan_amd.lib.data")
    cond = data_mod.preprocess_smpl_fix_body(rec, rec["joints_index"].tolist(), rec["smpl_tpose_vertices"])
    cond = {k: v[None] for k, v in cond.items()}
    cond["scales"] = cond["scales"].reshape(1)
    pan, tilt = app.camera_sweep(2, math.pi / 6, 0, False)
    for i in range(2):
        view = conditions.CameraPreprocessor().forward_with_rotation(dict(cond), pan[i:i + 1], tilt[i:i + 1], torch.zeros(1))
        ref = RR.rasterize(cond["vertices"], torch.as_tensor(rec["faces"]), view["raster_rotation"],
                           conditions.raster_translation(view), -F_R, H, W, torch.as_tensor(rec["faces_to_labels"]),
                           cond["tpose_vertices"][0])
        sem = ref["semantics"].float().clamp(-1, 1)
        sem = torch.where((sem == 0).all(dim=1, keepdim=True), torch.ones_like(sem), sem)
        want = app.to_uint8_nhwc(sem)[0]
        got = smpl[:, i * W:(i + 1) * W]
        far = ~ref["near"][0].numpy()
        assert (ref["pix_to_face"][0] >= 0).sum() > 1000
        assert np.array_equal(got[far], want[far])
