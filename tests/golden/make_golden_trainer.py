"""Golden fixture of the trainer's schedule from the real Python reference: trainer_schedule.json.

BUILD CONTAINER ONLY (imports /root/reference through _ref_import.py).  Stores data only.  A tiny curriculum with two int steps,
the second of which raises the render size (the sizes live in the int steps: static keys win
in extract_metadata), and an end step; for steps 0..19:
  meta         the reference's configs.extract_metadata(curriculum, step) (JSON-able keys)
  lrs          the group learning rates after the reference's PhaseTrainer.set_learning_rate (lib/trainers/phase_trainer.py:87-109),
               called unbound on real torch.optim.Adam groups
  phase        step % len(phases)                                                     (phase_trainer.py:299)
  alpha        min(1, (step - last_upsample_step) / fade_steps), last_upsample_step the reference's   (base_trainer.py:383)
  nerf_noise   max(0, 1 - step / 5000)                                                (base_trainer.py:384)
or {"ended": true} once batch_size has disappeared (base_trainer.py:342).
Run:  python tests/golden/make_golden_trainer.py
"""
import json
import os
import sys
import types
import warnings

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
warnings.filterwarnings("ignore")

import _ref_import  # noqa: E402

_ref_import.install()
for name in ("tensorboardX", "torch.utils.tensorboard"):
    if name not in sys.modules:
        m = types.ModuleType(name)
        m.SummaryWriter = object
        sys.modules[name] = m

import configs as ref_configs  # noqa: E402
import lib.trainers.phase_trainer as pt  # noqa: E402

GROUPS = ("generator", "appearance_codes", "neural_field_mapping", "synthesis_mapping", "neural_field")


def curriculum():
    phases = [dict(name="uncond", uncond=True, gen_modal="rgbs", rotate=r, do_r1=d)
              for r, d in zip((False, True, True, False), (False, False, False, True))]
    return {0: dict(batch_size=4, batch_split=1, gen_lr=1e-4, disc_lr=4e-4, render_height=8, render_width=4),
            7: dict(batch_size=4, batch_split=1, gen_lr=5e-5, disc_lr=2e-4, render_height=16, render_width=8),
            15: {},
            "phases": phases, "fade_steps": 4, "betas": (0, 0.9), "weight_decay": 0, "appearance_codes_lr_mul": 1.0,
            "mapping_net_lr_mul": 0.05, "neural_field_lr_mul": 0.25, "gen_height": 16,
            "gen_width": 8, "ada_interval": 0, "use_mixed_precision": False, "grad_clip": 1.0, "latent_dim": 8}


def main():
    cur = curriculum()
    opt_g = torch.optim.Adam([{"params": [torch.nn.Parameter(torch.zeros(1))], "name": n} for n in GROUPS], lr=1.0)
    opt_d = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    me = types.SimpleNamespace(optimizer_G=opt_g, optimizer_D=opt_d)
    steps = {}
    for step in range(20):
        meta = ref_configs.extract_metadata(cur, step)
        if "batch_size" not in meta:
            steps[str(step)] = {"ended": True}
            continue
        pt.PhaseTrainer.set_learning_rate(me, meta)
        last = ref_configs.last_upsample_step(cur, step)
        steps[str(step)] = dict(
            meta={k: (list(v) if isinstance(v, tuple) else v) for k, v in meta.items()},
            lrs={g["name"]: g["lr"] for g in opt_g.param_groups} | {"discriminator": opt_d.param_groups[0]["lr"]},
            betas=list(opt_d.param_groups[0]["betas"]), weight_decay=opt_d.param_groups[0]["weight_decay"],
            phase=step % len(meta["phases"]), last_upsample_step=last,
            alpha=min(1, (step - last) / meta["fade_steps"]),                         # base_trainer.py:383
            nerf_noise=max(0, 1. - step / 5000.))                                     # base_trainer.py:384
    cur_json = {str(k): v for k, v in cur.items()}
    cur_json["betas"] = list(cur["betas"])
    path = os.path.join(HERE, "trainer_schedule.json")
    json.dump(dict(curriculum=cur_json, int_steps=[0, 7, 15], groups=list(GROUPS), steps=steps), open(path, "w"), indent=1)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
