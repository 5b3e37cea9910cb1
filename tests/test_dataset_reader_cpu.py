"""The dataset reader on the CPU: the float64 restatement of the ingest against torch's own resampling (the published definitions of
the torchvision and cv2 boundaries), synthetic.write_example_dataset, and SHHQDataset on a dataset written into tmp_path."""
import importlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _ingest_reference import SHAPES, ingest_f64, make_inputs, nearest

pytest.importorskip("PIL")
synthetic = importlib.import_module("3dhumangan_amd.synthetic")
data = importlib.import_module("3dhumangan_amd.lib.data")
conditions = importlib.import_module("3dhumangan_amd.lib.data.conditions")

LENGTH, SRC, SIZE = 4, (16, 8), (8, 4)
ITEM_KEYS = {"indices", "latents", "images", "masks", "body_segments", "scales", "skeletons_xyz", "intrinsics", "vertices", "tpose_vertices",
             "full_pose", "fk_matrices", "lbs_weights", "cano_matrices", "R", "T"}


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return synthetic.write_example_dataset(str(tmp_path_factory.mktemp("shhq")), length=LENGTH, height=SRC[0], width=SRC[1], seed=2)


def _dataset(root, **over):
    kw = dict(dataroot=root, dataset_length=LENGTH, gen_height=SIZE[0], gen_width=SIZE[1], latent_dim=16, joints=list(range(24)),
              smpl_model=os.path.join(root, "smpl_model.npz"))
    kw.update(over)
    return data.SHHQDataset(**kw)


@pytest.mark.parametrize("src,size", SHAPES)
def test_restatement_is_the_published_resize_definitions(src, size):
    """torchvision 0.10.1 Resize on a tensor == F.interpolate(bilinear, align_corners=False) on the white-backed, normalised float
    image; cv2 INTER_NEAREST == torch's mode="nearest" (floor(x * src / dst)).  Bar 1e-6: torch's fp32 scale arithmetic."""
    rgb, mask, seg = make_inputs(2, src[0], src[1], seed=7)
    images, masks, segments = ingest_f64(rgb, mask, seg, size)
    u = np.where(mask[..., None] == 0, 255, rgb)
    t = torch.from_numpy(u).permute(0, 3, 1, 2).float().div(255).sub(0.5).div(0.5)                          # ToTensor, Normalize
    e = float((F.interpolate(t, size=size, mode="bilinear", align_corners=False).double().numpy() - images).__abs__().max())
    tm = torch.from_numpy(mask)[:, None].float().div(255).sub(0.5).div(0.5)
    e_m = float(np.abs(F.interpolate(tm, size=size, mode="bilinear", align_corners=False).double().numpy() - masks).max())
    print(f"{src}->{size}: restatement vs F.interpolate images {e:.2e} masks {e_m:.2e}")
    assert e <= 1e-6 and e_m <= 1e-6
    near = F.interpolate(torch.from_numpy(seg)[:, None].float(), size=size, mode="nearest")[:, 0].long().numpy()
    assert np.array_equal(np.where(near == 0, 1, near + 1), segments)
    assert np.array_equal(nearest(size[0], src[0]), np.floor(np.arange(size[0]) * (src[0] / size[0])).astype(np.int64).clip(max=src[0] - 1))


@pytest.mark.parametrize("src,size", SHAPES)
@pytest.mark.parametrize("geo_only", [False, True])
def test_ingest_torch_against_the_restatement(src, size, geo_only):
    for kind in ("zero", "full", "random"):
        arrays = make_inputs(2, src[0], src[1], seed=3, mask_kind=kind)
        want_i, want_m, want_s = ingest_f64(*arrays, size, geo_only)
        got = data.ingest_torch(*[torch.from_numpy(a) for a in arrays], size, geo_only)
        assert got["images"].dtype == torch.float32 and got["body_segments"].dtype == torch.int64 and got["masks"].shape == (2, 1, *size)
        assert np.array_equal(got["body_segments"].numpy(), want_s)
        assert float(np.abs(got["images"].double().numpy() - want_i).max()) <= 1e-6
        assert float(np.abs(got["masks"].double().numpy() - want_m).max()) <= 1e-6


def test_ingest_torch_refuses_wrong_inputs_by_name():
    rgb, mask, seg = [torch.from_numpy(a) for a in make_inputs(1, 8, 4, seed=1)]
    with pytest.raises(TypeError, match="mask must be a uint8"):
        data.ingest_torch(rgb, mask.float(), seg, (4, 2))
    with pytest.raises(ValueError, match=r"rgb must be \[B,Hs,Ws,3\]"):
        data.ingest_torch(rgb[0], mask, seg, (4, 2))
    with pytest.raises(ValueError, match="rgb is on cpu"):
        data.ingest(rgb, mask, seg, (4, 2))


def test_written_dataset_layout(root):
    from PIL import Image
    for d, ext in (("images", "png"), ("masks", "png"), ("body_seg", "png"), ("inversions", "npy"), ("smpl", "npz")):
        assert sorted(os.listdir(os.path.join(root, d))) == [f"{i + 1:06d}.{ext}" for i in range(LENGTH)]
    seg = np.asarray(Image.open(os.path.join(root, "body_seg", "000001.png")))
    mask = np.asarray(Image.open(os.path.join(root, "masks", "000001.png")))
    assert seg.shape == (*SRC, 3) and mask.shape == SRC and set(np.unique(mask)) == {0, 255}
    assert seg.max() <= 24 and len(np.unique(seg[..., 0])) > 5 and not seg[..., 0][mask == 0].any()
    rec = np.load(os.path.join(root, "smpl", "000001.npz"))
    assert not set(rec.files) & set(synthetic.RECORD_ASSETS) and {"orig_cam", "joints", "full_pose", "fk_matrices", "tpose_vertices"} <= set(rec.files)
    assert set(synthetic.make_smpl_model()) == set(np.load(os.path.join(root, "smpl_model.npz")).files)


def test_item_keys_shapes_and_dtypes_in_every_mode(root):
    ds = _dataset(root)
    item = ds[1]
    assert set(item) == ITEM_KEYS and item["indices"] == 1 and len(ds) == LENGTH
    V = ds.template.shape[0]
    want = {"latents": (16,), "images": (3, *SIZE), "masks": (1, *SIZE), "body_segments": SIZE, "scales": (), "skeletons_xyz": (24, 3),
            "intrinsics": (4, 4), "vertices": (V, 3), "tpose_vertices": (V, 3), "full_pose": (24, 3, 3), "fk_matrices": (24, 4, 4),
            "lbs_weights": (V, 24), "cano_matrices": (4, 4), "R": (4, 4), "T": (4, 4)}
    for k, shape in want.items():
        assert tuple(item[k].shape) == shape, k
        assert item[k].dtype == (torch.int64 if k == "body_segments" else torch.float32), k
    assert float(item["images"].abs().max()) <= 1 and torch.equal(item["latents"], torch.from_numpy(2 * np.load(ds.path("inversions", 1, "npy"))[:16]))
    assert set(_dataset(root, image_only=True)[1]) == {"images", "masks"}
    cond = _dataset(root, condition_only=True, inference=True)[1]
    assert set(cond) == (ITEM_KEYS - {"indices", "latents", "images", "masks", "body_segments"}) | {"body_shape"} and cond["body_shape"].shape == (10,)
    assert "body_shape" in _dataset(root, inference=True)[1]
    geo = _dataset(root, geo_only=True)[1]
    assert torch.equal(geo["images"], geo["masks"].expand(3, -1, -1)) and torch.equal(geo["masks"], item["masks"])
    assert set(_dataset(root, joints=[], smpl_model={k: v for k, v in np.load(os.path.join(root, "smpl_model.npz")).items()
                                                     if k != "joints_index"})[1]) == {"indices", "latents", "images", "masks", "body_segments"}
    # the model's assets
    model = synthetic.make_smpl_model()
    assert torch.equal(ds.faces, torch.from_numpy(model["faces"])) and torch.equal(ds.faces_to_labels, torch.from_numpy(model["faces_to_labels"]))
    assert torch.equal(ds.lbs_weights, torch.from_numpy(model["lbs_weights"])) and torch.equal(ds.template, torch.from_numpy(model["v_template"]))
    with pytest.raises(NotImplementedError, match="fix_body"):
        _dataset(root, coordinate_mode="fix_camera")
    assert _dataset(root, vertex_downsample=4)[0]["vertices"].shape == (V, 3)


def test_item_is_the_transform_of_its_files(root):
    from PIL import Image
    ds = _dataset(root)
    for i in range(LENGTH):
        raw, item = ds.raw(i), ds[i]
        assert raw["rgb"].dtype == raw["mask"].dtype == raw["seg"].dtype == np.uint8 and raw["rgb"].shape == (*SRC, 3) and raw["index"] == i
        assert np.array_equal(raw["seg"], np.asarray(Image.open(ds.path("body_seg", i, "png")))[..., 0])
        images, masks, segments = ingest_f64(raw["rgb"][None], raw["mask"][None], raw["seg"][None], SIZE)
        assert float(np.abs(item["images"].double().numpy() - images[0]).max()) <= 1e-6
        assert float(np.abs(item["masks"].double().numpy() - masks[0]).max()) <= 1e-6
        assert np.array_equal(item["body_segments"].numpy(), segments[0])
        # the label remap: 0 -> 1, k -> k + 1, at the nearest source pixel
        near = raw["seg"][nearest(SIZE[0], SRC[0])][:, nearest(SIZE[1], SRC[1])].astype(np.int64)
        assert np.array_equal(item["body_segments"].numpy(), np.where(near == 0, 1, near + 1)) and int(item["body_segments"].min()) == 1
        assert int(item["body_segments"].max()) > 2
        # the conditions are preprocess_smpl_fix_body of the record with the model's weights and template
        rec = dict(np.load(ds.path("smpl", i, "npz")))
        want = conditions.preprocess_smpl_fix_body(rec, list(range(24)), ds.template)
        for k, w in want.items():
            assert torch.equal(item[k], w), k
        assert set(raw) == {"index", "rgb", "mask", "seg", "latent", "orig_cam", "joints", "full_pose", "fk_matrices", "tpose_vertices"}
    assert "betas" in _dataset(root, inference=True).raw(0)
    # white background at source resolution: outside the ellipse the image is exactly 1
    corner = ds[0]
    assert bool((corner["images"][:, 0, 0] == 1.0).all()) and float(corner["masks"][0, 0, 0]) == -1.0


def test_corrupted_indices_are_skipped(root):
    ds = _dataset(root)
    ds.corrupted = [1, 2]
    assert ds[1]["indices"] == 3 and ds.raw(2)["index"] == 3 and torch.equal(ds[1]["images"], ds[3]["images"])
    ds.corrupted = [LENGTH - 1]
    assert ds[LENGTH - 1]["indices"] == 0                                               # wraps, as the reference's loop does
    assert data.SHHQDataset.corrupted == [118464]


def test_a_missing_file_is_named(root, tmp_path):
    import shutil
    broken = str(tmp_path / "broken")
    shutil.copytree(root, broken)
    os.remove(os.path.join(broken, "masks", "000002.png"))
    os.remove(os.path.join(broken, "smpl", "000003.npz"))
    ds = _dataset(broken)
    with pytest.raises(FileNotFoundError, match=r"masks.000002\.png"):
        ds[1]
    with pytest.raises(FileNotFoundError, match=r"masks.000002\.png"):
        ds.raw(1)
    with pytest.raises(FileNotFoundError, match=r"smpl.000003\.npz"):
        ds[2]
    with pytest.raises(FileNotFoundError, match="nowhere.npz"):
        _dataset(root, smpl_model=str(tmp_path / "nowhere.npz"))
    with pytest.raises(ValueError, match="smpl_model"):
        _dataset(root, smpl_model=None)


def test_pkl_and_npz_records_give_equal_items(root, tmp_path):
    pytest.importorskip("joblib")
    other = synthetic.write_example_dataset(str(tmp_path / "pkl"), length=LENGTH, height=SRC[0], width=SRC[1], seed=2, records="pkl")
    assert sorted(os.listdir(os.path.join(other, "smpl"))) == [f"{i + 1:06d}.pkl" for i in range(LENGTH)]
    a, b = _dataset(root, inference=True), _dataset(other, inference=True)
    for i in range(LENGTH):
        x, y = a[i], b[i]
        assert x.keys() == y.keys()
        for k in x:
            assert torch.equal(x[k], y[k]) if torch.is_tensor(x[k]) else x[k] == y[k], k
    with pytest.raises(ValueError, match="records must be"):
        synthetic.write_example_dataset(str(tmp_path / "bad"), length=1, records="json")


def test_record_with_foreign_lbs_weights_is_refused(root, tmp_path):
    import shutil
    broken = str(tmp_path / "weights")
    shutil.copytree(root, broken)
    path = os.path.join(broken, "smpl", "000001.npz")
    rec = dict(np.load(path))
    assert "lbs_weights" in rec
    rec["lbs_weights"] = np.roll(rec["lbs_weights"], 1, axis=1)
    np.savez(path, **rec)
    with pytest.raises(ValueError, match="lbs_weights that differ"):
        _dataset(broken)[0]
    _dataset(broken)[1]


def test_densepose_composition(root, tmp_path):
    """faces_to_labels[f] = densepose_faces_to_labels[smpl_faces_to_densepose_faces[f]] (reference preprocessor.py:187-192)"""
    model = {k: v for k, v in synthetic.make_smpl_model().items() if k != "faces_to_labels"}
    model["faces"] = model["faces"][:5]
    path = str(tmp_path / "densepose_data.json")
    json.dump({"smpl_faces_to_densepose_faces": [3, 0, 2, 2, 1], "densepose_faces_to_labels": [7, 11, 13, 17]}, open(path, "w"))
    assert data.densepose_faces_to_labels(path, 5).tolist() == [17, 7, 13, 13, 11]
    ds = _dataset(root, smpl_model=model, densepose_data=path)
    assert ds.faces_to_labels.tolist() == [17, 7, 13, 13, 11] and ds.faces_to_labels.dtype == torch.int64
    with pytest.raises(ValueError, match="densepose_data"):
        _dataset(root, smpl_model=model)
    pre = data.get_preprocessor("cpu", model, densepose_data=path, coordinate_mode="fix_body")
    assert pre.smpl_faces_to_labels.tolist() == [17, 7, 13, 13, 11] and pre.smpl_faces.shape == (5, 3)
    full = data.get_preprocessor("cpu", os.path.join(root, "smpl_model.npz"))
    assert torch.equal(full.smpl_faces_to_labels, torch.from_numpy(synthetic.make_smpl_model()["faces_to_labels"]))
