"""Training from a dataset on the GPU: an 8-item dataset written at 32 x 16 (synthetic.write_example_dataset), read through
DatasetTrainingSource (pinned staging, h3d_ingest, smpl_conditions) and compared with the stacked CPU items of SHHQDataset; then the
tiny real networks of tests/test_gpu_trainer.py at 16 x 8, batch 2, trained from it, and a resumed run."""
import importlib
import json
import os

import pytest
import torch

pytest.importorskip("PIL")
from test_gpu_trainer import _curriculum, _opt  # noqa: E402

pytestmark = pytest.mark.gpu
synthetic = importlib.import_module("3dhumangan_amd.synthetic")
data = importlib.import_module("3dhumangan_amd.lib.data")
pt = importlib.import_module("3dhumangan_amd.lib.trainers.phase_trainer")

LENGTH, SIZE = 8, (16, 8)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = synthetic.write_example_dataset(str(tmp_path_factory.mktemp("shhq")), length=LENGTH, height=32, width=16, seed=6)
    return data.SHHQDataset(dataroot=root, dataset_length=LENGTH, gen_height=SIZE[0], gen_width=SIZE[1], latent_dim=16,
                            joints=list(range(24)), smpl_model=os.path.join(root, "smpl_model.npz"))


def test_source_on_the_device_against_the_stacked_cpu_items(dataset):
    """images / masks: 1e-6 (the ingest's bar); segments equal; conditions: the bars tests/test_gpu_smpl.py holds smpl_conditions to --
    vertices (J + 7) 2^-24 of the largest coordinate, everything else float32 rounding of float64 matrices."""
    src = data.DatasetTrainingSource(dataset, seed=1, prefetch=2)
    try:
        for g in (0, 1, 2, 5):                                   # 1 and 2 were prefetched (pinned rows filled by the workers), 5 was not
            out = src.batches(2, g, "cuda")
            idx = src.indices(2, g)
            assert out["indices"].tolist() == idx and all(v.is_cuda for v in out.values())
            items = [dataset[i] for i in idx]
            want = {k: torch.stack([torch.as_tensor(it[k]) for it in items]) for k in items[0] if k != "indices"}
            assert set(want) | {"indices", "cam2world_matrices"} == set(out)
            for k, w in want.items():
                got = out[k].cpu()
                assert got.shape == w.shape and got.dtype == w.dtype, k
                if k == "body_segments":
                    assert torch.equal(got, w)
                elif k in ("images", "masks"):
                    e = float((got - w).abs().max())
                    print(f"g={g} {k}: {e:.2e}")
                    assert e <= 1e-6, (k, e)
                elif k == "vertices":
                    e, bar = float((got - w).abs().max()), (24 + 7) * 2.0 ** -24 * float(w.abs().max())
                    print(f"g={g} vertices: err {e:.2e} bar {bar:.2e}")
                    assert e <= bar
                elif k == "latents":
                    assert torch.equal(got, w)
                else:
                    assert torch.allclose(got, w, rtol=1e-6, atol=1e-7), k
    finally:
        src.close()


def test_prefetch_on_and_off_and_the_torch_composition_give_the_same_tensors(dataset):
    on, off = data.DatasetTrainingSource(dataset, seed=2, prefetch=2, num_workers=4), data.DatasetTrainingSource(dataset, seed=2, prefetch=0, num_workers=1)
    composed = data.DatasetTrainingSource(dataset, seed=2, prefetch=0, fused=False)
    try:
        for g in (0, 1, 2, 3, 1):
            a, b, c = on.batches(2, g, "cuda"), off.batches(2, g, "cuda"), composed.batches(2, g, "cuda")
            assert a.keys() == b.keys()
            for k in a:
                assert torch.equal(a[k], b[k]), (g, k)
            assert torch.equal(a["body_segments"], c["body_segments"]) and float((a["images"] - c["images"]).abs().max()) <= 2e-6
        slots = on._slots + [r.slot for r in on._pending.values() if r.slot is not None]      # free ones and those being filled
        assert slots and all(s.rgb.is_pinned() and s.mask.is_pinned() and s.seg.is_pinned() for s in slots)
        assert len(on._slots) <= 2 * (on.prefetch + 2)
    finally:
        for s in (on, off, composed):
            s.close()


def _trainer(out, dataset, records, **over):
    src = data.DatasetTrainingSource(dataset, seed=3, prefetch=2)
    return pt.PhaseTrainer(0, 1, "cuda", _opt(out, **over), _curriculum(), src, on_step=records.append), src


def _lines(path):
    return [json.loads(ln) for ln in open(os.path.join(path, "train_log.jsonl"))]


def test_trainer_runs_from_the_dataset_and_a_resumed_run_repeats_step_two(dataset, tmp_path):
    """The resumed run loads the saved state bit for bit and is fed bit-identical inputs (asserted); what is left between the two
    runs' scalars of step 2 is the summation order of library kernels (MIOpen's backward): 1e-4 relative, the bar
    tests/test_gpu_seg_loss_step.py holds a step to whose inputs differ in their last bits."""
    whole, first, second = [], [], []
    t, src = _trainer(tmp_path / "a", dataset, whole, max_steps=2)
    t.run()
    src.close()
    lines = _lines(tmp_path / "a")
    assert t.step == 2 and [ln["step"] for ln in lines] == [0, 1]
    for ln in lines:
        assert all(v == v and abs(v) < 1e6 for v in list(ln["d"].values()) + list(ln["g"].values())), ln
        assert ln["d"]["segmentation"] > 0
    t1, src1 = _trainer(tmp_path / "b", dataset, first, max_steps=1)
    t1.run()
    src1.close()
    t2, src2 = _trainer(tmp_path / "b", dataset, second, max_steps=2)
    assert t2.step == 1
    t2.run()
    src2.close()
    assert [r["step"] for r in second] == [1]
    for k in ("z_d", "z_g", "d_view", "g_view"):
        assert torch.equal(whole[1][k], second[0][k]), k
    a, b = lines[1], _lines(tmp_path / "b")[-1]
    assert b["step"] == 1
    for part in ("d", "g"):
        for k, v in a[part].items():
            print(f"step 2 {part}.{k}: uninterrupted {v:.9g} resumed {b[part][k]:.9g}")
            assert abs(v - b[part][k]) <= 1e-4 * abs(v) + 1e-6, (part, k, v, b[part][k])


def test_sample_app_takes_each_seeds_body_from_the_dataset(dataset, tmp_path):
    import numpy as np
    from PIL import Image
    from conftest import load_golden
    app = importlib.import_module("3dhumangan_amd.apps.sample_from_generator")
    configs = importlib.import_module("3dhumangan_amd.configs")
    cfg = dict(load_golden("gen_tiny_mixed")["meta"])
    cfg.update(neural_field_cls="COORDCONCATSIREN", name="tiny_dataset")
    configs.TINY_DATASET = cfg
    H, W = cfg["gen_height"], cfg["gen_width"]
    ckpt = str(tmp_path / "tiny_state_dict.pth")
    torch.save(load_golden("gen_tiny_mixed")["state"], ckpt)
    out_dir = app.main(["--config", "TINY_DATASET", "--checkpoint", ckpt, "--dataroot", dataset.root, "--smpl-model",
                        os.path.join(dataset.root, "smpl_model.npz"), "--dataset_length", "4", "--seeds", "1", "2", "--n_angles", "2",
                        "--save", "png", "--output_dir", str(tmp_path / "out")])
    sems = []
    for seed in (1, 2):
        frames = np.asarray(Image.open(f"{out_dir}/{seed:03d}_uncond.png")).astype(np.float64)
        sems.append(np.asarray(Image.open(f"{out_dir}/{seed:03d}_smpl.png")))
        assert frames.shape == (H, 2 * W, 3) and sems[-1].shape == (H, 2 * W, 3) and np.isfinite(frames).all()
        assert (sems[-1] != 255).any()                                          # the rasteriser drew the record's body
    assert not np.array_equal(sems[0], sems[1])                                 # two seeds, two items of the shuffled order


def test_a_batch_with_two_source_sizes_on_the_device(dataset, tmp_path):
    """items 2 and 5 at twice the size: a prefetched request then holds rows its workers staged (pinned) beside rows they could not
    (another size) -- one ingest per size, each through its own staging buffer, assembled in the batch's order"""
    import shutil
    big = synthetic.write_example_dataset(str(tmp_path / "big"), length=LENGTH, height=64, width=32, seed=6)
    mixed = str(tmp_path / "mixed")
    shutil.copytree(dataset.root, mixed)
    for d in ("images", "masks", "body_seg"):
        for name in ("000002.png", "000005.png"):
            shutil.copy(os.path.join(big, d, name), os.path.join(mixed, d, name))
    ds = data.SHHQDataset(dataroot=mixed, dataset_length=LENGTH, gen_height=SIZE[0], gen_width=SIZE[1], latent_dim=16,
                          joints=list(range(24)), smpl_model=os.path.join(mixed, "smpl_model.npz"))
    src = data.DatasetTrainingSource(ds, shuffle=False, prefetch=2)
    try:
        for g in (0, 1, 2):                                      # g = 2 wraps into the next epoch: items 0..3 again
            out = src.batches(4, g, "cuda")
            items = [ds[i % LENGTH] for i in range(4 * g, 4 * g + 4)]
            assert out["indices"].tolist() == [i % LENGTH for i in range(4 * g, 4 * g + 4)]
            assert torch.equal(out["body_segments"].cpu(), torch.stack([it["body_segments"] for it in items]))
            for k in ("images", "masks"):
                assert float((out[k].cpu() - torch.stack([it[k] for it in items])).abs().max()) <= 1e-6, (g, k)
    finally:
        src.close()
