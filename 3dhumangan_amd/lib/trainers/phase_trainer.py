"""The training session: curriculum stepping, the phase cycle, learning-rate schedule, the shared GradScaler, checkpoints and
resume around the existing discriminator_step / generator_step.

Reference: BaseTrainer.run (lib/trainers/base_trainer.py:328-449) and PhaseTrainer (lib/trainers/phase_trainer.py:57-110,
297-341).  Per step s:
    meta  = configs.extract_metadata(config, s)            the run ends when "batch_size" disappears
    phase = meta["phases"][s % len(phases)]                rotate / do_r1 of the step
    alpha = min(1, (s - last_upsample_step) / fade_steps), nerf_noise = max(0, 1 - s / 5000)          (:383-384)
    the preprocessor runs once before each of the two steps with rotate = phase["rotate"] (:305, :329); the D step's labels are
    rasterized_segments when rotate or a draw < 0.5, else body_segments (:350-353), likewise the G step's (:533)
Every random draw of step s -- z of both steps, the views, the label choices, the generator's jitter and noise -- follows
torch.manual_seed(step_seed(opt.seed, rank, s)) at the top of the step, so a resumed run draws what the uninterrupted run drew
(the reference seeds once per run and uses Python's `random` for the label choice; both come from torch's generator here).
One GradScaler when use_mixed_precision is set, shared by both steps, updated by the G step only, and put back to 1 when it has
dropped below 1 (base_trainer.py:374-375; done on the device, no host read).

Refused by name (ValueError), because no shipped config uses them: batch_split * bs_factor > 1, a phase with uncond=False, a
phase whose gen_modal != "rgbs", ada_interval != 0, dual_discrimination.

Data source protocol: source.batches(batch, step, device) -> dict with images [B,3,H,W], body_segments [B,H,W] and the condition
entries CameraPreprocessor and the generator read; source.faces, source.faces_to_labels; source.length.  The rank-r shard of
step s is batches(batch, s * world_size + r, device).  synthetic.SyntheticTrainingSource is one; lib/data/source.DatasetTrainingSource
(a dataset in the reference's layout) is the other.
"""
import json
import os

import torch

from ... import checkpoints, configs
from ..components.ema import ExponentialMovingAverage
from . import losses
from .d_step import discriminator_step
from .g_step import generator_step, make_generator_optimizer

GROUP_LR = {"generator": lambda m: m["gen_lr"], "appearance_codes": lambda m: m["gen_lr"] * m["appearance_codes_lr_mul"],
            "neural_field_mapping": lambda m: m["gen_lr"] * m["mapping_net_lr_mul"], "synthesis_mapping": lambda m: m["gen_lr"],
            "neural_field": lambda m: m["gen_lr"] * m["neural_field_lr_mul"]}


def step_seed(seed, rank, step):
    """one seed per (run seed, rank, step), below 2^63"""
    return ((int(seed) * 1_000_003 + int(rank)) * 1_000_003 + int(step)) % (2 ** 63 - 1)


def schedule(config, step):
    """-> (meta, phase index, alpha, nerf_noise) of `step`, or None when the curriculum has ended (base_trainer.py:341-342, 383-384)"""
    meta = configs.extract_metadata(config, step)
    if "batch_size" not in meta:
        return None
    alpha = min(1, (step - configs.last_upsample_step(config, step)) / meta["fade_steps"])
    return meta, step % len(meta["phases"]), alpha, max(0, 1. - step / 5000.)


def set_learning_rate(optimizer_G, optimizer_D, meta):
    """phase_trainer.py:87-109: lr, betas and weight_decay of the five named generator groups and of the D group from `meta`"""
    for group in optimizer_G.param_groups:
        if group.get("name") not in GROUP_LR:
            raise ValueError(f"param_group not defined: {group.get('name')!r} (one of {sorted(GROUP_LR)})")
        group["lr"] = GROUP_LR[group["name"]](meta)
    for group in optimizer_D.param_groups:
        group["lr"] = meta["disc_lr"]
    for group in optimizer_G.param_groups + optimizer_D.param_groups:
        group["betas"] = tuple(float(b) for b in meta["betas"])
        group["weight_decay"] = meta["weight_decay"]


def check_supported(meta, bs_factor=1):
    """the refusals, by name"""
    if meta.get("batch_split", 1) * bs_factor > 1:
        raise ValueError(f"batch_split * bs_factor = {meta.get('batch_split', 1) * bs_factor} > 1: gradient accumulation is not provided")
    if meta.get("ada_interval", 0) != 0:
        raise ValueError("ada_interval != 0: adaptive discriminator augmentation is not provided")
    if meta.get("dual_discrimination", False):
        raise ValueError("dual_discrimination is not provided")
    for phase in meta["phases"]:
        if not phase.get("uncond", True):
            raise ValueError(f"phase {phase.get('name')!r} has uncond=False: the conditional phases are not provided")
        if phase.get("gen_modal", "rgbs") != "rgbs":
            raise ValueError(f"phase {phase.get('name')!r} has gen_modal={phase.get('gen_modal')!r}: only 'rgbs' is provided")


class PhaseTrainer:
    """PhaseTrainer(rank, world_size, device, opt, config, source).run().  opt: output_dir, n_epochs, seed, save_interval,
    model_keep_interval, log_interval, max_steps (None: no limit), bs_factor.  A directory that holds saved steps is resumed from
    the newest; rank 0 saves every save_interval steps and at the end of run().  generator / discriminator / preprocessor / d_step / g_step / seg_loss / on_step: replaceable parts (tests run the
    control plane on stand-ins); on_step(record) sees the inputs of every step."""

    def __init__(self, rank, world_size, device, opt, config, source=None, generator=None, discriminator=None, preprocessor=None,
                 d_step=None, g_step=None, seg_loss=None, on_step=None):
        self.rank, self.world_size, self.device, self.opt, self.config, self.source = rank, world_size, torch.device(device), opt, config, source
        self.output_dir = opt.output_dir
        self.d_step, self.g_step, self.on_step = d_step or discriminator_step, g_step or generator_step, on_step
        self.step = self.epoch = 0
        self.seed = int(getattr(opt, "seed", 0))
        saved = checkpoints.saved_steps(self.output_dir)
        if saved:
            self.step = saved[-1]
        meta = configs.extract_metadata(config, self.step)
        if "batch_size" not in meta:
            raise ValueError(f"the curriculum has no batch_size at step {self.step}: nothing to train")
        check_supported(meta, getattr(opt, "bs_factor", 1))
        cuda = self.device.type == "cuda"
        self.amp_dtype = torch.float16 if (meta.get("use_mixed_precision", False) and cuda) else None
        self.scaler = torch.amp.GradScaler("cuda") if self.amp_dtype is not None else None
        # the fused loss is faster than the torch composition at both measured shapes (profiles/seg_loss_bench.json)
        self.seg_loss = seg_loss if seg_loss is not None else (losses.segmentation_loss_fused if cuda else None)
        torch.manual_seed(step_seed(self.seed, 0, 0))                     # identical initial weights on every rank
        self.generator = generator if generator is not None else self._build("generator", meta)
        self.discriminator = discriminator if discriminator is not None else self._build("discriminator", meta)
        if hasattr(self.generator, "set_device"):
            self.generator.set_device(self.device)
        self.ema = ExponentialMovingAverage(self.generator.parameters(), decay=0.999).to(self.device)
        self.optimizer_G = make_generator_optimizer(self.generator, meta)
        self.optimizer_D = torch.optim.Adam(self.discriminator.parameters(), lr=meta["disc_lr"], betas=tuple(float(b) for b in meta["betas"]),
                                            weight_decay=meta["weight_decay"])
        if preprocessor is None:
            from ..data.conditions import CameraPreprocessor
            preprocessor = CameraPreprocessor(self.device, **{k: v for k, v in meta.items() if isinstance(k, str)})
            preprocessor.init_smpl(source.faces, source.faces_to_labels)
        self.preprocessor = preprocessor
        if saved:
            rec = checkpoints.load_training_state(self.output_dir, self.generator, self.discriminator, self.ema, self.optimizer_G,
                                                  self.optimizer_D, self.scaler, step=self.step, map_location=self.device)
            if rec["seed"] != self.seed:
                raise ValueError(f"{self.output_dir} was written with --seed {rec['seed']}, this run asks for {self.seed}")
            self.step, self.epoch = rec["step"], rec["epoch"]

    def _build(self, kind, meta):
        from .. import discriminators, generators, implicit_funcitions
        kw = {k: v for k, v in meta.items() if isinstance(k, str)}
        if isinstance(kw.get("neural_field_cls"), str):
            kw["neural_field_cls"] = getattr(implicit_funcitions, kw["neural_field_cls"])
        if kind == "discriminator":
            kw.pop("neural_field_cls", None)
        return getattr(generators if kind == "generator" else discriminators, meta[kind])(**kw).to(self.device)

    def save(self):
        return checkpoints.save_training_state(self.output_dir, self.step, self.generator, self.discriminator, self.ema, self.optimizer_G,
                                               self.optimizer_D, self.scaler, epoch=self.epoch, seed=self.seed,
                                               keep_interval=getattr(self.opt, "model_keep_interval", None))

    def _labels(self, data, rotate):
        """(:350-353, :533) -> (labels, which)"""
        which = "rasterized_segments" if (rotate or float(torch.rand(())) < 0.5) else "body_segments"
        return data[which], which

    def _z(self, batch, meta):
        return torch.randn(batch, meta["latent_dim"]).to(self.device)

    def train_step(self, meta, phase_idx, alpha, nerf_noise):
        """one iteration at self.step -> (D scalars, G scalars)"""
        step, phase = self.step, meta["phases"][phase_idx]
        torch.manual_seed(step_seed(self.seed, self.rank, step))
        if self.scaler is not None and getattr(self.scaler, "_scale", None) is not None:
            self.scaler._scale.clamp_(min=1.0)                              # base_trainer.py:374-375 without the host read
        meta = dict(meta, nerf_noise=nerf_noise)
        fwd = {k: v for k, v in meta.items() if isinstance(k, str)}
        batch = meta["batch_size"] // self.world_size
        self.generator.train()
        self.discriminator.train()
        data = self.source.batches(batch, step * self.world_size + self.rank, self.device)
        record = dict(step=step, phase=phase_idx, alpha=alpha, nerf_noise=nerf_noise,
                      lrs=[g["lr"] for g in self.optimizer_G.param_groups] + [g["lr"] for g in self.optimizer_D.param_groups])
        distributed = self.world_size > 1
        # ---- discriminator
        d_data = self.preprocessor(data, phase["rotate"], **fwd)
        d_labels, record["d_labels"] = self._labels(d_data, phase["rotate"])
        z_d = self._z(batch, meta)
        with torch.no_grad(), torch.autocast("cuda", dtype=self.amp_dtype or torch.float16, enabled=self.amp_dtype is not None):
            fake = self.generator(z_d, d_data, **fwd)["rgbs"].float()
        d = self.d_step(self.discriminator, self.optimizer_D, d_data["images"], fake, d_labels, meta, do_r1=phase["do_r1"],
                        distributed=distributed, grad_clip=meta["grad_clip"], amp_dtype=self.amp_dtype, scaler=self.scaler,
                        seg_loss=self.seg_loss)
        # ---- generator
        g_data = self.preprocessor(data, phase["rotate"], **fwd)
        g_labels, record["g_labels"] = self._labels(g_data, phase["rotate"])
        z_g = self._z(batch, meta)
        g = self.g_step(self.generator, self.discriminator, self.optimizer_G, z_g, g_data, meta, gt_segments=g_labels, ema=self.ema,
                        distributed=distributed, d_step_count=step, gen_modal=phase["gen_modal"], amp_dtype=self.amp_dtype,
                        scaler=self.scaler, seg_loss=self.seg_loss)
        if self.on_step is not None:
            record.update(z_d=z_d, z_g=z_g, d_view=d_data.get("cam2world_matrices"), g_view=g_data.get("cam2world_matrices"))
            self.on_step(record)
        return d, g

    def _log(self, meta, phase_idx, alpha, d, g):
        def scalars(res):
            return {k: float(v) for k, v in res.items()}                    # the only host reads of device scalars
        line = dict(step=self.step, epoch=self.epoch, phase=phase_idx, alpha=alpha,
                    lrs={g_["name"]: g_["lr"] for g_ in self.optimizer_G.param_groups} | {"discriminator": self.optimizer_D.param_groups[0]["lr"]},
                    scale=float(self.scaler.get_scale()) if self.scaler is not None else 1.0, d=scalars(d), g=scalars(g))
        with open(os.path.join(self.output_dir, "train_log.jsonl"), "a") as f:
            f.write(json.dumps(line) + "\n")

    def run(self):
        opt = self.opt
        os.makedirs(self.output_dir, exist_ok=True)
        max_steps, save_interval = getattr(opt, "max_steps", None), getattr(opt, "save_interval", 1000)
        log_interval, first = max(1, getattr(opt, "log_interval", 10)), self.step
        while self.epoch < opt.n_epochs:
            at = schedule(self.config, self.step)
            if at is None:
                break
            meta = at[0]
            check_supported(meta, getattr(opt, "bs_factor", 1))
            set_learning_rate(self.optimizer_G, self.optimizer_D, meta)
            size = (meta["batch_size"], meta["gen_height"], meta["gen_width"])
            for _ in range(max(1, getattr(self.source, "length", meta["batch_size"]) // meta["batch_size"])):
                at = schedule(self.config, self.step)
                if at is None or (at[0]["batch_size"], at[0]["gen_height"], at[0]["gen_width"]) != size:
                    break
                if max_steps is not None and self.step >= max_steps:
                    return self._finish(first)
                if self.rank == 0 and self.step % save_interval == 0 and self.step > first:
                    self.save()
                d, g = self.train_step(*at)
                if self.rank == 0 and self.step % log_interval == 0:
                    self._log(at[0], at[1], at[2], d, g)
                self.step += 1
            self.epoch += 1
        return self._finish(first)

    def _finish(self, first):
        """the state at the end of the run is saved too (the reference saves only every 1000 steps: a short run would leave nothing
        to resume from)"""
        if self.rank == 0 and self.step > first:
            self.save()
        return self
