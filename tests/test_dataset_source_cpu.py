"""DatasetTrainingSource on a CPU device: the order, determinism under prefetch and threads, mixed source sizes, errors, the trainer's
control plane on the stand-ins of tests/_trainer_stubs.py, the train app's source-building path, and h3d_ingest's argument checks."""
import ctypes
import importlib
import os
import shutil

import pytest
import torch

from _trainer_stubs import StubD, StubG, StubPreprocessor, curriculum, stub_meta_over, stub_opt

pytest.importorskip("PIL")
synthetic = importlib.import_module("3dhumangan_amd.synthetic")
data = importlib.import_module("3dhumangan_amd.lib.data")
train_app = importlib.import_module("3dhumangan_amd.apps.train")
pt = importlib.import_module("3dhumangan_amd.lib.trainers.phase_trainer")

LENGTH, SRC, SIZE = 8, (8, 4), (4, 2)


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return synthetic.write_example_dataset(str(tmp_path_factory.mktemp("shhq")), length=LENGTH, height=SRC[0], width=SRC[1], seed=4)


def _dataset(root, **over):
    kw = dict(dataroot=root, dataset_length=LENGTH, gen_height=SIZE[0], gen_width=SIZE[1], latent_dim=8, joints=list(range(24)),
              smpl_model=os.path.join(root, "smpl_model.npz"))
    kw.update(over)
    return data.SHHQDataset(**kw)


@pytest.fixture(scope="module")
def dataset(root):
    return _dataset(root)


def _equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("shuffle", [True, False])
def test_an_epoch_holds_each_item_once(dataset, shuffle):
    src = data.DatasetTrainingSource(dataset, seed=3, shuffle=shuffle, prefetch=0)
    try:
        for batch in (1, 2, 3):                                                 # 3 does not divide 8: a batch straddles two epochs
            flat = [i for g in range(LENGTH) for i in src.indices(batch, g)]    # batch epochs' worth of positions
            for e in range(batch):
                assert sorted(flat[e * LENGTH:(e + 1) * LENGTH]) == list(range(LENGTH)), (batch, e)
            if not shuffle:
                assert flat[:LENGTH] == list(range(LENGTH))
        if shuffle:
            first, second = ([i for g in range(e * 4, e * 4 + 4) for i in src.indices(2, g)] for e in (0, 1))
            assert first != list(range(LENGTH)) and first != second
            other = data.DatasetTrainingSource(dataset, seed=4, prefetch=0)
            assert [i for g in range(4) for i in other.indices(2, g)] != first
            other.close()
        assert src.batches(2, 1, "cpu")["indices"].tolist() == src.indices(2, 1)
    finally:
        src.close()


def test_two_ranks_are_disjoint_and_complete(dataset):
    src = data.DatasetTrainingSource(dataset, seed=1, stride=2, prefetch=0)
    ranks = [[i for s in range(2) for i in src.indices(2, s * 2 + r)] for r in (0, 1)]    # steps 0, 1 of a world of 2, batch 2 per rank
    assert not set(ranks[0]) & set(ranks[1]) and sorted(ranks[0] + ranks[1]) == list(range(LENGTH))
    src.close()


def test_batches_are_byte_equal_whatever_the_call_order_threads_and_prefetch(dataset):
    ref_src = data.DatasetTrainingSource(dataset, seed=2, num_workers=1, prefetch=0)
    want = {g: ref_src.batches(2, g, "cpu") for g in range(6)}
    ref_src.close()
    stacked = [dataset[i] for i in want[3]["indices"].tolist()]
    for k in ("images", "masks", "body_segments", "latents", "vertices", "fk_matrices", "skeletons_xyz", "scales", "T"):
        assert torch.equal(want[3][k], torch.stack([torch.as_tensor(it[k]) for it in stacked])), k
    for workers, prefetch, stride, order in ((4, 2, 1, [0, 1, 2, 3, 4, 5]), (4, 2, 2, [1, 3, 5, 0, 2, 4]), (1, 2, 1, [5, 0, 4, 1, 1, 3, 2]),
                                             (4, 0, 1, [2, 0, 5])):
        src = data.DatasetTrainingSource(dataset, seed=2, num_workers=workers, prefetch=prefetch, stride=stride)
        for g in order:
            _equal(src.batches(2, g, "cpu"), want[g])
        assert len(src._pending) <= 2 * max(prefetch, 1)
        src.close()
    assert data.DatasetTrainingSource(dataset, num_workers=400).num_workers == 16


def test_result_holds_every_key_of_the_synthetic_source(dataset):
    src = data.DatasetTrainingSource(dataset, prefetch=0)
    out = src.batches(2, 0, "cpu")
    src.close()
    synth_keys = {"skeletons_xyz", "vertices", "fk_matrices", "cam2world_matrices", "tpose_vertices", "lbs_weights", "intrinsics", "scales",
                  "R", "T", "full_pose", "images", "body_segments", "indices"}         # SyntheticTrainingSource.batches (synthetic.py)
    assert synth_keys | {"masks", "latents"} <= set(out)
    assert out["images"].shape == (2, 3, *SIZE) and out["masks"].shape == (2, 1, *SIZE) and out["latents"].shape == (2, 8)
    assert out["body_segments"].dtype == torch.int64 and out["cam2world_matrices"].shape == (2, 4, 4) and out["scales"].shape == (2,)
    assert torch.equal(src.faces, dataset.faces) and torch.equal(src.faces_to_labels, dataset.faces_to_labels) and src.length == LENGTH
    # the canonical view: what the camera front-end gives for zero angles
    pre = data.CameraPreprocessor("cpu")
    z = torch.zeros(2)
    assert torch.equal(out["cam2world_matrices"], pre.forward_with_rotation(out, z, z, z)["cam2world_matrices"])


def test_a_batch_with_two_source_sizes(root, tmp_path):
    big = synthetic.write_example_dataset(str(tmp_path / "big"), length=LENGTH, height=2 * SRC[0], width=2 * SRC[1], seed=4)
    mixed = str(tmp_path / "mixed")
    shutil.copytree(root, mixed)
    for d in ("images", "masks", "body_seg"):
        for name in ("000002.png", "000005.png"):
            shutil.copy(os.path.join(big, d, name), os.path.join(mixed, d, name))
    ds = _dataset(mixed)
    assert ds.raw(1)["rgb"].shape == (2 * SRC[0], 2 * SRC[1], 3) and ds.raw(0)["rgb"].shape == (*SRC, 3)
    src = data.DatasetTrainingSource(ds, shuffle=False, prefetch=2)
    for g in range(2):
        out = src.batches(4, g, "cpu")
        items = [ds[i] for i in range(4 * g, 4 * g + 4)]
        for k in ("images", "masks", "body_segments"):
            assert torch.equal(out[k], torch.stack([it[k] for it in items])), k
    src.close()


def test_a_worker_error_surfaces_naming_the_file(root, tmp_path):
    broken = str(tmp_path / "broken")
    shutil.copytree(root, broken)
    os.remove(os.path.join(broken, "body_seg", "000004.png"))
    src = data.DatasetTrainingSource(_dataset(broken), shuffle=False, prefetch=2)
    src.batches(2, 0, "cpu")                                                    # schedules g = 1 (items 2, 3) and g = 2
    with pytest.raises(RuntimeError, match=r"item 3 .*body_seg.000004\.png"):
        src.batches(2, 1, "cpu")
    assert src.batches(2, 2, "cpu")["indices"].tolist() == [4, 5]               # the source goes on
    src.close()
    with pytest.raises(RuntimeError):
        src.batches(2, 3, "cpu")                                                # closed: the pool takes no more work


class _Clamped:
    """the dataset source behind the stand-in networks' 3 labels; records what every request returned"""

    def __init__(self, src):
        self.src, self.length, self.faces, self.faces_to_labels, self.fed = src, src.length, src.faces, src.faces_to_labels, []

    def batches(self, batch, g, device):
        out = self.src.batches(batch, g, device)
        self.fed.append((g, out["indices"].tolist()))
        out["body_segments"] = out["body_segments"].clamp(max=2)
        return out


def _trainer(out, dataset, records, **opt):
    torch.manual_seed(11)
    src = _Clamped(data.DatasetTrainingSource(dataset, seed=opt.get("seed", 3), prefetch=2))
    t = pt.PhaseTrainer(0, 1, "cpu", stub_opt(out, **opt), curriculum(**stub_meta_over()), src, generator=StubG(), discriminator=StubD(),
                        preprocessor=StubPreprocessor(), on_step=records.append)
    return t, src


def test_trainer_runs_from_the_source_and_a_resumed_run_feeds_the_same_items(dataset, tmp_path):
    whole, first, second = [], [], []
    t, a = _trainer(tmp_path / "a", dataset, whole, max_steps=3)
    t.run()
    a.src.close()
    assert t.step == 3 and [g for g, _ in a.fed] == [0, 1, 2] and all(len(i) == 4 for _, i in a.fed)
    assert sorted(a.fed[0][1] + a.fed[1][1]) == list(range(LENGTH))            # batch 4: two steps are one epoch
    t1, b1 = _trainer(tmp_path / "b", dataset, first, max_steps=2)
    t1.run()
    b1.src.close()
    t2, b2 = _trainer(tmp_path / "b", dataset, second, max_steps=3)
    assert t2.step == 2
    t2.run()
    b2.src.close()
    assert b1.fed + b2.fed == a.fed
    assert torch.equal(whole[2]["z_d"], second[0]["z_d"]) and whole[2]["d_labels"] == second[0]["d_labels"]


def test_train_app_builds_the_source(root, tmp_path):
    opt = train_app.parse_args(["--dataroot", root, "--smpl-model", os.path.join(root, "smpl_model.npz"), "--dataset_length", "6",
                                "--num_workers", "2", "--seed", "5"])
    assert opt.source == "shhq" and opt.num_workers == 2 and opt.densepose_data is None
    assert train_app.parse_args([]).source == "synthetic" and train_app.parse_args(["--source", "shhq"]).dataroot is None
    meta = dict(gen_height=SIZE[0], gen_width=SIZE[1], latent_dim=8, joints=list(range(24)), batch_size=2, label_dim=26,
                dataroot="/nowhere", dataset_length=3)
    src = train_app.build_source(opt, meta, world=2)
    assert isinstance(src, data.DatasetTrainingSource) and src.length == 6 and src.stride == 2 and src.seed == 5 and src.num_workers == 2
    assert src.dataset.root == root and src.batches(2, 0, "cpu")["images"].shape == (2, 3, *SIZE)
    src.close()
    # dataroot and dataset_length default to the config's
    opt = train_app.parse_args(["--source", "shhq", "--smpl-model", os.path.join(root, "smpl_model.npz")])
    src = train_app.build_source(opt, dict(meta, dataroot=root))
    assert src.dataset.root == root and src.length == 3
    src.close()
    with pytest.raises(ValueError, match="--smpl-model"):
        train_app.build_source(train_app.parse_args(["--dataroot", root]), meta)
    assert train_app.parse_args(["--dataroot", root]).source == "shhq"


def test_sample_app_dataroot_needs_the_model_flag(root):
    app = importlib.import_module("3dhumangan_amd.apps.sample_from_generator")
    with pytest.raises(ValueError, match="--smpl-model"):
        app.main(["--dataroot", root, "--seeds", "1"])
    with pytest.raises(ValueError, match="pass one"):
        app.main(["--dataroot", root, "--smpl-model", os.path.join(root, "smpl_model.npz"), "--pose-sequence", "synthetic"])


@pytest.fixture(scope="module")
def lib():
    build = importlib.import_module("3dhumangan_amd._build")
    return ctypes.CDLL(build.build_lib())


def test_h3d_ingest_refuses_bad_arguments_without_a_device(lib):
    lib.h3d_ingest.restype = ctypes.c_int
    lib.h3d_ingest.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int] * 6 + [ctypes.c_void_p]
    lib.h3d_last_error.restype = ctypes.c_char_p
    p = ctypes.c_void_p(4096)                                                   # never dereferenced: every call below is refused first
    assert lib.h3d_ingest(None, p, p, p, p, p, 1, 8, 4, 4, 2, 0, None) == -1 and b"null pointer" in lib.h3d_last_error()
    assert lib.h3d_ingest(p, p, p, p, p, None, 1, 8, 4, 4, 2, 0, None) == -1 and b"null pointer" in lib.h3d_last_error()
    for shape in ((0, 8, 4, 4, 2), (1, 0, 4, 4, 2), (1, 8, -1, 4, 2), (1, 8, 4, 0, 2), (1, 8, 4, 4, 0)):
        assert lib.h3d_ingest(p, p, p, p, p, p, *shape, 0, None) == -1 and b"bad shape" in lib.h3d_last_error(), shape
    assert lib.h3d_ingest(p, p, p, p, p, p, 1024, 1024, 1024, 4, 2, 0, None) == -1 and b"overflows int32" in lib.h3d_last_error()
    assert lib.h3d_ingest(p, p, p, p, p, p, 1024, 4, 2, 1024, 1024, 0, None) == -1 and b"overflows int32" in lib.h3d_last_error()
    assert lib.h3d_ingest(p, p, p, p, p, p, 1, 40000, 1, 40000, 1, 0, None) == -1 and b"resize coordinates" in lib.h3d_last_error()
