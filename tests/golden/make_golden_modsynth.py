"""Golden fixtures of the generator WITHOUT spatial normalisation (spatial_normalization="none": SynthesisBlock /
SpatialStyleModLayer / nn.Linear ToRGB), written by the real Python reference.

BUILD CONTAINER ONLY, like make_golden.py, whose reference import, tiny config, weight conditioning and writer it reuses:
the reference modules are driven with seeded synthetic inputs and only *data* is stored.
Run:  python tests/golden/make_golden_modsynth.py
"""
import json

import numpy as np
import torch

import make_golden as mg        # installs the reference import shims

ref_gen, synthetic = mg.ref_gen, mg.synthetic


def fixture(name, seed, mod_blocks, map3d_mode, n_vertices=128, batch=2, nerf_noise=0.3):
    cfg = mg.tiny_cfg(spatial_normalization="none", map3d_mode=map3d_mode, mod_blocks=list(mod_blocks))
    torch.manual_seed(seed)
    G = ref_gen.Map3DGenerator(**cfg).eval()
    G.set_device("cpu")
    mg.condition_weights(G, seed)          # non-zero mod1/mod2 biases; no spectral norm or BatchNorm in this variant
    cond = synthetic.make_conditions(batch, n_vertices=n_vertices, seed=seed, pose_scale=0.6)
    z = torch.randn(batch, cfg["latent_dim"], generator=torch.Generator().manual_seed(seed + 1))
    run = dict(cfg)
    run["nerf_noise"] = nerf_noise
    R, S = cfg["render_height"] * cfg["render_width"], cfg["num_steps"]

    # whole forward, the random tensors replayed in the reference's consumption order
    rs = seed + 7
    torch.manual_seed(rs)
    jitter = torch.rand(batch, R, S, 1)
    torch.randn(batch, 1), torch.randn(batch, 1)
    noise = torch.randn(batch, R, S, 1) * nerf_noise
    torch.manual_seed(rs)
    rendered = []
    render = G.render
    G.render = lambda *a, **k: (rendered.append(render(*a, **k)), rendered[-1])[1]      # keep what fed the synthesis network
    with torch.no_grad():
        out = G.forward(z, cond, **run)
        _, styles = G.synthesis_mapping_network(z)
    G.render = render
    rgb_render, fmap = rendered[0][0], rendered[0][1]
    feats = torch.cat([(rgb_render + 1) / 2, fmap], dim=1).flatten(2).transpose(1, 2).contiguous()        # [B, R, 3 + F]

    # staged_forward with truncation (draws randn(10000, L) first)
    torch.manual_seed(rs + 1)
    torch.randn(10000, cfg["latent_dim"])
    jitter_s = torch.rand(batch, R, S, 1)
    torch.manual_seed(rs + 1)
    srun = dict(run)
    srun.update(truncation_psi=0.7, nerf_noise=0, last_back=cfg["eval_last_back"], return_internal=True)
    G.render = lambda *a, **k: (rendered.append(render(*a, **k)), rendered[-1])[1]
    with torch.no_grad():
        sout = G.staged_forward(z, cond, **srun)
    G.render = render
    feats_s = torch.cat([(rendered[1][0] + 1) / 2, rendered[1][1]], dim=1).flatten(2).transpose(1, 2).contiguous()
    avg = dict(z=G.avg_latent[0], freq=G.avg_latent[1], phase=G.avg_latent[2], styles=G.avg_latent[3])

    meta = {k: v for k, v in cfg.items() if isinstance(v, (int, float, str, bool))}
    meta["mod_blocks"] = list(cfg["mod_blocks"])
    mg.save(name, state=G.state_dict(), cond=cond, z=z, jitter=jitter, noise=noise,
            meta_json=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
            out=dict(rgbs=out["rgbs"], rgbs_render=out["rgbs_render"]),
            stage=dict(styles=styles, feats=feats),
            staged=dict(jitter=jitter_s, feats=feats_s, rgbs=sout["rgbs"], rgbs_render=sout["rgbs_render"], depths=sout["depths"],
                        m3d_2_feature_map=sout["m3d_2_feature_map"], m3d_5_rgb=sout["m3d_5_rgb"],
                        m3d_8_feature_map=sout["m3d_8_feature_map"]),
            avg=avg)


if __name__ == "__main__":
    fixture("gen_tiny_none_mixed", seed=11, mod_blocks=[0, 1, 2], map3d_mode="mixed")
    fixture("gen_tiny_none_isolated", seed=12, mod_blocks=[0, 2, 5], map3d_mode="isolated")
    fixture("gen_tiny_none_all", seed=13, mod_blocks=[0, 1, 2], map3d_mode="all")
