"""Golden fixtures of the synthesis input variants, written by the real Python reference: the label map and / or the latent
as extra inputs of the synthesis network (2d_label_input, 2d_latent_input) and a feature_dim that differs from hidden_dim.

BUILD CONTAINER ONLY, like make_golden.py, whose reference import, tiny config, weight conditioning and writer it reuses:
the reference modules are driven with seeded synthetic inputs and only *data* is stored.
  gen_tiny_2d_*.npz, gen_tiny_*_feature.npz   eval-mode forward + staged_forward (truncation 0.7, stored avg latent)
  gen_train_2d_label_latent.npz, gen_train_narrow_feature.npz   train-mode forward + backward, as make_golden_train's
Run:  python tests/golden/make_golden_2d_inputs.py
"""
import json
import os

import numpy as np
import torch

import make_golden as mg        # installs the reference import shims
from make_golden_norender import COND_HW, blob_segments

ref_gen, synthetic = mg.ref_gen, mg.synthetic
LIMIT = 1 << 20                 # a committed file stays below 1 MiB


def _meta(cfg, **extra):
    meta = {k: v for k, v in cfg.items() if isinstance(v, (int, float, str, bool))}
    meta["mod_blocks"] = list(cfg["mod_blocks"])
    meta.update(extra)
    return np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)


def _conditions(cfg, batch, seed, norender):
    """Conditions with a label map at the image size (the label input's); labels 0 and label_dim-1 occur in every image.
    norender: the style input reads its own, smaller map under the key condition_modal_gen names."""
    cond = synthetic.make_conditions(batch, n_vertices=128, seed=seed, pose_scale=0.6)
    g = torch.Generator().manual_seed(seed + 3)
    cond["rasterized_segments"] = blob_segments(batch, (cfg["gen_height"], cfg["gen_width"]), cfg["label_dim"], g)
    if norender:
        cond[cfg["condition_modal_gen"]] = blob_segments(batch, COND_HW, cfg["label_dim"], g)
    for seg in (cond["rasterized_segments"], cond[cfg["condition_modal_gen"]]):
        assert int(seg.min()) == 0 and int(seg.max()) == cfg["label_dim"] - 1
    return cond


def _check_size(name):
    size = os.path.getsize(os.path.join(mg.HERE, name + ".npz"))
    assert size < LIMIT, (name, size)


def inference_fixture(name, seed, batch=2, nerf_noise=0.3, norender=False, **over):
    if norender:
        over["condition_modal_gen"] = "style_segments"
    cfg = mg.tiny_cfg(synthesis_blocks=4, **over)
    torch.manual_seed(seed)
    G = ref_gen.Map3DGenerator(**cfg).eval()
    G.set_device("cpu")
    mg.condition_weights(G, seed)
    cond = _conditions(cfg, batch, seed, norender)
    z = torch.randn(batch, cfg["latent_dim"], generator=torch.Generator().manual_seed(seed + 1))
    run = dict(cfg)
    run["nerf_noise"] = nerf_noise
    if norender:
        run["disable_render"] = True
    R, S = cfg["render_height"] * cfg["render_width"], cfg["num_steps"]
    rs = seed + 7
    torch.manual_seed(rs)                      # the reference's consumption order (make_golden.generator_fixture)
    jitter = torch.rand(batch, R, S, 1)
    torch.randn(batch, 1), torch.randn(batch, 1)
    noise = torch.randn(batch, R, S, 1) * nerf_noise
    torch.manual_seed(rs)
    with torch.no_grad():
        out = G.forward(z, cond, **run)
    # staged_forward with truncation (draws randn(10000, L) first)
    torch.manual_seed(rs + 1)
    torch.randn(10000, cfg["latent_dim"])
    jitter_s = torch.rand(batch, R, S, 1)
    torch.manual_seed(rs + 1)
    srun = dict(run)
    srun.update(truncation_psi=0.7, nerf_noise=0, last_back=cfg["eval_last_back"])
    with torch.no_grad():
        sout = G.staged_forward(z, cond, **srun)
    avg = dict(z=G.avg_latent[0], freq=G.avg_latent[1], phase=G.avg_latent[2], styles=G.avg_latent[3])
    mg.save(name, state=G.state_dict(), cond=cond, z=z, jitter=jitter, noise=noise, meta_json=_meta(cfg),
            out=dict(rgbs=out["rgbs"], rgbs_render=out["rgbs_render"]),
            staged=dict(jitter=jitter_s, rgbs=sout["rgbs"], rgbs_render=sout["rgbs_render"], depths=sout["depths"]), avg=avg)
    _check_size(name)


def train_fixture(name, seed, batch=3, nerf_noise=0.3, **over):
    """make_golden_train.generator_train_fixture with a label map in the conditions."""
    cfg = mg.tiny_cfg(**over)
    torch.manual_seed(seed)
    G = ref_gen.Map3DGenerator(**cfg)
    G.set_device("cpu")
    mg.condition_weights(G, seed)
    g = torch.Generator().manual_seed(seed + 3)
    with torch.no_grad():                                  # u, v off the singular vectors: the power iteration must move them
        for k, v in G.state_dict().items():
            if k.endswith("weight_u") or k.endswith("weight_v"):
                v.copy_(torch.nn.functional.normalize(v + 0.3 * torch.randn(v.shape, generator=g), dim=0))
        G.latent_pool.latents.copy_(torch.randn(G.latent_pool.latents.shape, generator=g))
    G.train()
    state0 = {k: v.clone() for k, v in G.state_dict().items()}
    cond = _conditions(cfg, batch, seed, False)
    z = torch.randn(batch, cfg["latent_dim"], generator=g).requires_grad_(True)
    run = dict(cfg)
    run["nerf_noise"] = nerf_noise
    R, S = cfg["render_height"] * cfg["render_width"], cfg["num_steps"]
    rs = seed + 7
    torch.manual_seed(rs)
    jitter = torch.rand(batch, R, S, 1)
    torch.randn(batch, 1), torch.randn(batch, 1)
    noise = torch.randn(batch, R, S, 1) * nerf_noise
    torch.manual_seed(rs)
    out = G.forward(z, cond, **run)
    p_rgb = torch.randn(out["rgbs"].shape, generator=g)
    p_render = torch.randn(out["rgbs_render"].shape, generator=g)
    loss = (out["rgbs"] * p_rgb).sum() + (out["rgbs_render"] * p_render).sum()
    loss.backward()
    grads = {n: p.grad for n, p in G.named_parameters() if p.grad is not None}
    grads["__z__"] = z.grad
    changed = {k: v for k, v in G.state_dict().items() if not torch.equal(v, state0[k])}
    mg.save(name, state=state0, cond=cond, z=z, jitter=jitter, noise=noise, p_rgb=p_rgb, p_render=p_render,
            meta_json=_meta(cfg, nerf_noise=nerf_noise),
            out=dict(rgbs=out["rgbs"], rgbs_render=out["rgbs_render"], loss=loss), grad=grads, buffers_after=changed)
    print("   parameters with gradient:", len(grads) - 1, "of", len(list(G.named_parameters())), "| buffers changed:", len(changed))
    _check_size(name)


if __name__ == "__main__":
    label, latent = {"2d_label_input": True}, {"2d_latent_input": True}
    inference_fixture("gen_tiny_2d_label", seed=51, map3d_mode="mixed", **label)
    inference_fixture("gen_tiny_2d_latent", seed=52, map3d_mode="isolated", **latent)
    inference_fixture("gen_tiny_2d_label_latent", seed=53, map3d_mode="all", **label, **latent)
    # per-pixel styles in the two plain blocks only (skip connections from block 2): a network every SPADE engine takes
    inference_fixture("gen_tiny_narrow_feature", seed=54, feature_dim=16, mod_blocks=[0, 1])
    inference_fixture("gen_tiny_wide_feature", seed=55, feature_dim=48)
    inference_fixture("gen_tiny_2d_label_norender", seed=56, norender=True, **label)
    # two synthesis blocks (block 0 plain with the wide input, block 1 with skip connection; ToRGB from both): the gradients
    # double the file
    train_fixture("gen_train_2d_label_latent", seed=61, synthesis_blocks=2, mod_blocks=[0], **label, **latent)
    train_fixture("gen_train_narrow_feature", seed=62, synthesis_blocks=3, feature_dim=16)
