"""Stand-ins that let the trainer's control plane run on the CPU: tiny modules with the five named parameter groups, a data
source and a preprocessor that draw from torch's generator (so seeding is observable), and step functions that move the weights."""
import json
import os
import types

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def curriculum(**over):
    d = json.load(open(os.path.join(GOLDEN, "trainer_schedule.json")))["curriculum"]
    cur = {(int(k) if k.isdigit() else k): v for k, v in d.items()}
    cur["betas"] = tuple(cur["betas"])
    cur.update(over)
    return cur


class StubG(torch.nn.Module):
    def __init__(self, latent_dim=8):
        super().__init__()
        self.synthesis = torch.nn.Linear(latent_dim, 3 * 4 * 2)
        self.latent_pool = torch.nn.Embedding(2, latent_dim)
        self.neural_field_mapping_network = torch.nn.Linear(latent_dim, 2)
        self.synthesis_mapping_network = torch.nn.Linear(latent_dim, 2)
        self.neural_field = torch.nn.Linear(2, 2)

    def forward(self, z, conditions, **kw):
        extra = self.neural_field(self.neural_field_mapping_network(z) + self.synthesis_mapping_network(z)).sum() + self.latent_pool.weight.sum()
        return {"rgbs": torch.tanh(self.synthesis(z)).view(-1, 3, 4, 2) + 0 * extra + torch.randn(z.shape[0], 3, 4, 2) * kw.get("nerf_noise", 0)}


class StubD(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 4, 1)

    def forward(self, x, conditions, alpha, **kw):
        y = self.conv(x)
        return {"prediction": y[:, :1], "segments": y[:, 1:]}


class StubSource:
    length = 8
    faces = torch.zeros(1, 3, dtype=torch.long)
    faces_to_labels = torch.zeros(1, dtype=torch.long)

    def __init__(self):
        self.asked = []

    def batches(self, batch, step, device):
        self.asked.append((batch, step))
        g = torch.Generator().manual_seed(step)
        return {"images": torch.rand(batch, 3, 4, 2, generator=g) * 2 - 1, "body_segments": torch.randint(0, 3, (batch, 4, 2), generator=g),
                "scales": torch.ones(batch)}


class StubPreprocessor:
    """draws the views like CameraPreprocessor.forward does: torch.randn on the CPU generator, only spread when `rotate`"""

    def __call__(self, data, rotate=False, **kw):
        data = dict(data)
        B = data["scales"].shape[0]
        data["cam2world_matrices"] = torch.randn(B, 2) * (1.0 if rotate else 0.0) + torch.arange(2.0)
        data["rasterized_segments"] = (data["body_segments"] + 1) % 3
        return data


def stub_opt(output_dir, **over):
    opt = types.SimpleNamespace(output_dir=str(output_dir), n_epochs=100, seed=3, save_interval=1000, model_keep_interval=1000,
                                log_interval=1, max_steps=None, bs_factor=1)
    for k, v in over.items():
        setattr(opt, k, v)
    return opt


def stub_meta_over():
    return dict(label_dim=3, gan_lambda=0, segmentation_lambda=1, r1_lambda=0.0, latent_dim=8)
