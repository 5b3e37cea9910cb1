"""Train a generator / discriminator pair: the reference's second entry point (apps/train.py -> PhaseTrainer.run()).

    python -m 3dhumangan_amd.apps.train --config MAP3DBN --source synthetic --output_dir runs/toy --max_steps 100
    torchrun --nproc_per_node 8 -m 3dhumangan_amd.apps.train --config MAP3DBN512 --source synthetic --output_dir runs/toy

The reference's flags: --config, --output_dir, --n_epochs, --sample_interval (accepted; there is no image logging),
--model_keep_interval, --bs_factor.  Added: --seed, --save_interval, --log_interval, --max_steps, --source.  The rank comes from
LOCAL_RANK; a process group ("nccl") is initialised only when WORLD_SIZE > 1.  A run directory that holds saved steps is resumed.
The SHHQ reader needs licensed assets: --dataroot raises; `--source synthetic` trains on synthetic.SyntheticTrainingSource.
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
    ap.add_argument("--source", type=str, default="synthetic", choices=["synthetic"])
    ap.add_argument("--dataroot", type=str, default=None)
    return ap.parse_args(argv)


def main(argv=None):
    opt = parse_args(argv)
    if opt.dataroot is not None:
        raise NotImplementedError("the SHHQ dataset reader / SMPL preprocessor need licensed assets and pytorch3d; "
                                  "run with the synthetic conditions")
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
    source = synthetic.SyntheticTrainingSource(length=meta["batch_size"], gen_height=meta["gen_height"],
                                               gen_width=meta["gen_width"], seed=opt.seed, label_dim=meta["label_dim"])
    with torch.cuda.device(device):
        trainer = PhaseTrainer(rank, world, device, opt, config, source).run()
    if world > 1:
        torch.distributed.destroy_process_group()
    print(f"rank {rank}: stopped at step {trainer.step}, epoch {trainer.epoch}; state in {opt.output_dir}")
    return trainer


if __name__ == "__main__":
    main()
