"""Golden fixtures of the generator WITHOUT the 3D render (disable_render=True: SynthesisStyleInput on the rasterised
body condition feeds the synthesis network; no neural field, no ray integration), written by the real Python reference.

BUILD CONTAINER ONLY, like make_golden.py, whose reference import, tiny config, weight conditioning and writer it reuses:
the reference modules are driven with seeded synthetic inputs and only *data* is stored.
Run:  python tests/golden/make_golden_norender.py
"""
import json

import numpy as np
import torch

import make_golden as mg        # installs the reference import shims

ref_gen, synthetic = mg.ref_gen, mg.synthetic

COND_HW = (12, 6)               # differs from the 16 x 8 image and the 8 x 4 render size: the resize is exercised


def blob_segments(batch, hw, label_dim, g):
    """Integer labels 0 .. label_dim-1 in rectangular blobs on a background of label 1; labels 0 and label_dim-1 occur."""
    H, W = hw
    seg = torch.ones(batch, H, W, dtype=torch.int64)
    for b in range(batch):
        for _ in range(10):
            y0, x0 = int(torch.randint(0, H - 1, (1,), generator=g)), int(torch.randint(0, W - 1, (1,), generator=g))
            h, w = int(torch.randint(1, 5, (1,), generator=g)), int(torch.randint(1, 4, (1,), generator=g))
            seg[b, y0:y0 + h, x0:x0 + w] = int(torch.randint(0, label_dim, (1,), generator=g))
        seg[b, 0, 0], seg[b, -1, -1] = 0, label_dim - 1
    return seg


def blob_semantics(batch, hw, g):
    """Three channels in [-1, 1]: smooth inside a body-like blob, zero (the rasteriser's background) outside."""
    H, W = hw
    sem = torch.rand(batch, 3, H, W, generator=g) * 2 - 1
    yy = torch.linspace(-1, 1, H).view(1, 1, H, 1)
    xx = torch.linspace(-1, 1, W).view(1, 1, 1, W)
    inside = (yy ** 2 + (1.4 * xx) ** 2) < 0.9
    sem = torch.where(inside, sem, torch.zeros_like(sem))
    sem[:, :, H // 2, W // 2] = torch.tensor([1.0, -1.0, 1.0])
    return sem


def fixture(name, seed, modal, map3d_mode, normalization, batch=2, n_vertices=128, **over):
    cfg = mg.tiny_cfg(spatial_normalization=normalization, map3d_mode=map3d_mode, condition_modal_gen=modal, **over)
    torch.manual_seed(seed)
    G = ref_gen.Map3DGenerator(**cfg).eval()
    G.set_device("cpu")
    mg.condition_weights(G, seed)
    sd = G.state_dict()
    for k in ("from_coords.0.bias", "network.0.bias", "network.2.bias"):
        assert float(sd["synthesis_style_input." + k].abs().max()) > 0, k      # condition_weights left them non-zero
    cond = synthetic.make_conditions(batch, n_vertices=n_vertices, seed=seed, pose_scale=0.6)
    g = torch.Generator().manual_seed(seed + 3)
    cond["rasterized_segments"] = blob_segments(batch, COND_HW, cfg["label_dim"], g)
    cond["rasterized_semantics"] = blob_semantics(batch, COND_HW, g)
    z = torch.randn(batch, cfg["latent_dim"], generator=torch.Generator().manual_seed(seed + 1))
    run = dict(cfg)
    run["disable_render"] = True

    kept = []
    hook = G.synthesis_style_input.register_forward_hook(lambda m, a, out: kept.append(out.detach().clone()))
    with torch.no_grad():
        out = G.forward(z, cond, **run)
        _, styles = G.synthesis_mapping_network(z)
        # staged_forward with truncation (draws randn(10000, L) first); the reference's depth bookkeeping runs on zeros
        torch.manual_seed(seed + 8)
        srun = dict(run)
        srun.update(truncation_psi=0.7, nerf_noise=0, last_back=cfg["eval_last_back"])
        sout = G.staged_forward(z, cond, **srun)
    hook.remove()
    assert len(kept) == 2 and kept[0].shape == (batch, cfg["feature_dim"]) + COND_HW
    assert sorted(sout) == ["depths", "rgbs", "rgbs_render", "skeletons"], sorted(sout)
    avg = dict(z=G.avg_latent[0], freq=G.avg_latent[1], phase=G.avg_latent[2], styles=G.avg_latent[3])

    meta = {k: v for k, v in cfg.items() if isinstance(v, (int, float, str, bool))}
    meta["mod_blocks"] = list(cfg["mod_blocks"])
    mg.save(name, state=sd, cond=cond, z=z, meta_json=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
            out=dict(rgbs=out["rgbs"], rgbs_render=out["rgbs_render"]),
            stage=dict(feature_maps=kept[0], styles=styles),
            staged=dict(feature_maps=kept[1], rgbs=sout["rgbs"], rgbs_render=sout["rgbs_render"], depths=sout["depths"]),
            avg=avg)


if __name__ == "__main__":
    # the SPADE variants carry six synthesis blocks instead of nine (per-pixel style in blocks 0-2, skip from block 3, ToRGB
    # from block 2): the 128-wide shared MLPs of eighteen SPADEs alone would put the file above the 1 MiB limit of a
    # committed file
    fixture("gen_tiny_norender_segments", seed=21, modal="rasterized_segments", map3d_mode="mixed", normalization="batch_norm",
            synthesis_blocks=6)
    fixture("gen_tiny_norender_semantics", seed=22, modal="rasterized_semantics", map3d_mode="isolated", normalization="batch_norm",
            synthesis_blocks=6)
    fixture("gen_tiny_norender_none", seed=23, modal="rasterized_segments", map3d_mode="mixed", normalization="none")
