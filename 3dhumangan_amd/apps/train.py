"""Train a generator / discriminator pair: the reference's second entry point (apps/train.py -> PhaseTrainer.run()).

    python -m 3dhumangan_amd.apps.train --config MAP3DBN --source synthetic --output_dir runs/toy --max_steps 100
    torchrun --nproc_per_node 8 -m 3dhumangan_amd.apps.train --config MAP3DBN512 --source synthetic --output_dir runs/toy

The reference's flags: --config, --output_dir, --n_epochs, --sample_interval (accepted; there is no image logging),
--model_keep_interval, --bs_factor.  Added: --seed, --save_interval, --log_interval, --max_steps, --source.  The rank comes from
LOCAL_RANK; a process group ("nccl") is initialised only when WORLD_SIZE > 1.  A run directory that holds saved steps is resumed.
`--source synthetic` trains on synthetic.SyntheticTrainingSource.  `--source shhq` (implied by --dataroot) trains on a dataset in the
reference's layout (lib/data/datasets.py) through lib/data/source.DatasetTrainingSource: --dataroot and --dataset_length default to
the config's, --smpl-model PATH.npz is the plain-array SMPL model (required), --densepose-data PATH.json optionally supplies the
part labels of its faces, --num_workers sizes the decoding thread pool.  The images are ingested at the size of the curriculum's
first stage.
Progress: <output_dir>/<config name>/train_log.jsonl, one JSON line per --log_interval steps."""
import argparse
import os

import torch

from .. import configs, synthetic
from ..lib.trainers.phase_trainer import PhaseTrainer


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", type=str, default="MAP3DBN")
    ap.add_argument("--output_dir", type=str, default="results/train")
    ap.add_argument("--n_epochs", type=int, default=3000)
    ap.add_argument("--sample_interval", type=int, default=1000, help="accepted for the reference's command lines; no image logging")
    ap.add_argument("--model_keep_interval", type=int, default=10000)
    ap.add_argument("--bs_factor", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save_interval", type=int, default=1000)
    ap.add_argument("--log_interval", type=int, default=10)
    ap.add_argument("--max_steps", type=int, default=None)
    ap.add_argument("--source", type=str, default=None, choices=["synthetic", "shhq"], help="default: shhq with --dataroot, else synthetic")
    ap.add_argument("--dataroot", type=str, default=None, help="dataset directory (default with --source shhq: the config's)")
    ap.add_argument("--dataset_length", type=int, default=None, help="items to use (default: the config's)")
    ap.add_argument("--smpl-model", type=str, default=None, help="an .npz SMPL model (the arrays of synthetic.make_smpl_model)")
    ap.add_argument("--densepose-data", type=str, default=None, help="a densepose_data.json: the part labels of the model's faces")
    ap.add_argument("--num_workers", type=int, default=4, help="decoding threads of the dataset source")
    opt = ap.parse_args(argv)
    if opt.source is None:
        opt.source = "shhq" if opt.dataroot is not None else "synthetic"
    return opt


def build_source(opt, meta, world=1):
    """the data source `opt` asks for, at the size of `meta`"""
    if opt.source == "synthetic":
        return synthetic.SyntheticTrainingSource(length=meta["batch_size"], gen_height=meta["gen_height"], gen_width=meta["gen_width"],
                                                 seed=opt.seed, label_dim=meta["label_dim"])
    if opt.smpl_model is None:
        raise ValueError("--source shhq / --dataroot needs --smpl-model PATH.npz: the SMPL model as plain arrays (v_template, "
                         "lbs_weights, faces, faces_to_labels, joints_index); the licensed model file itself cannot ship")
    from ..lib.data import DatasetTrainingSource, SHHQDataset
    kw = {k: v for k, v in meta.items() if isinstance(k, str)}
    kw["dataroot"] = opt.dataroot if opt.dataroot is not None else kw.get("dataroot")
    kw["dataset_length"] = opt.dataset_length if opt.dataset_length is not None else kw.get("dataset_length")
    if kw["dataroot"] is None or kw["dataset_length"] is None:
        raise ValueError("--source shhq: neither the flags nor the config give dataroot / dataset_length")
    dataset = SHHQDataset(**dict(kw, smpl_model=opt.smpl_model, densepose_data=opt.densepose_data))
    return DatasetTrainingSource(dataset, seed=opt.seed, stride=world, num_workers=opt.num_workers)


def main(argv=None):
    opt = parse_args(argv)
    rank, world = int(os.environ.get("LOCAL_RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    if not torch.cuda.is_available():
        raise RuntimeError("training needs a ROCm device: the generator has no CPU path")
    torch.cuda.set_device(rank)
    device = torch.device("cuda", rank)
    if world > 1:
        torch.distributed.init_process_group("nccl")
    config = configs.get_config(opt)
    opt.output_dir = os.path.join(opt.output_dir, config["name"])
    meta = configs.extract_metadata(config, 0)
    source = build_source(opt, meta, world)
    try:
        with torch.cuda.device(device):
            trainer = PhaseTrainer(rank, world, device, opt, config, source).run()
    finally:
        if hasattr(source, "close"):
            source.close()
    if world > 1:
        torch.distributed.destroy_process_group()
    print(f"rank {rank}: stopped at step {trainer.step}, epoch {trainer.epoch}; state in {opt.output_dir}")
    return trainer


if __name__ == "__main__":
    main()
