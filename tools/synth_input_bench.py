"""Timing of h3d_synth_input (forward and adjoint) against the torch composition it replaces -- linear + sin + cat and its autograd --
at B = 16, 512 x 256, F = L = 256, K = 3, and of gen-resolution inference of the 2d_label_input variant (layer-wise synthesis) next
to the no-flag model on the default and the fp32 synthesis engine (MAP3DBN512, B = 8).  Medians of alternating calls, device events.

    python tools/synth_input_bench.py [--json profiles/synth_input_bench.json]
"""
import argparse
import importlib
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
op = importlib.import_module("3dhumangan_amd.lib.components.ops.synth_input")
gens = importlib.import_module("3dhumangan_amd.lib.generators")
impl = importlib.import_module("3dhumangan_amd.lib.implicit_funcitions")
configs = importlib.import_module("3dhumangan_amd.configs")
synthetic = importlib.import_module("3dhumangan_amd.synthetic")
DEV = "cuda"
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12


def timed(fns, warm=3, reps=10):
    """Alternating timing of several callables with device events -> list of median ms."""
    for _ in range(warm):
        for f in fns:
            f()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    return [sorted(t)[len(t) // 2] for t in times], [(min(t), max(t)) for t in times]


def op_bench():
    B, H, W, Fd, L, K, label_dim = 16, 512, 256, 256, 256, 3, 26
    P = H * W
    g = torch.Generator().manual_seed(0)
    w = ((torch.rand(Fd, K, generator=g) * 2 - 1) * 3 ** 0.5).to(DEV).requires_grad_(True)
    b = torch.randn(Fd, generator=g).to(DEV).requires_grad_(True)
    z = torch.randn(B, L, generator=g).to(DEV).requires_grad_(True)
    seg = torch.randint(0, label_dim, (B, H, W), generator=g).to(DEV)
    p = torch.randn(B, P, Fd + L, device=DEV)

    def torch_fwd():
        ii = torch.linspace(-1, 1, H, device=DEV)[:, None].expand(H, W)
        jj = torch.linspace(-1, 1, W, device=DEV)[None, :].expand(H, W)
        c = torch.stack([ii, jj], dim=-1)[None].expand(B, H, W, 2)
        c = torch.cat([c, (seg.unsqueeze(-1) / label_dim * 2 - 1)], dim=-1).reshape(B, P, K)
        x = torch.sin(F.linear(c, w, b))
        return torch.cat([x, z[:, None].expand(B, P, L)], dim=-1)

    def hip_fwd():
        return op.synth_input(w, b, (H, W), B, seg=seg, z=z, label_dim=label_dim)

    def both(fwd):
        return lambda: torch.autograd.grad(fwd(), [w, b, z], grad_outputs=p)

    a, c = hip_fwd(), torch_fwd()
    agree = float((a - c).abs().max())
    ga, gc = both(hip_fwd)(), both(torch_fwd)()
    gagree = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(ga, gc)]
    del a, c, ga, gc
    (t_hf, t_tf, t_hb, t_tb), spread = timed([hip_fwd, torch_fwd, both(hip_fwd), both(torch_fwd)])
    bytes_pass = B * P * (Fd + L) * 4
    res = dict(shape=dict(B=B, H=H, W=W, F=Fd, L=L, K=K), bytes_per_pass=bytes_pass,
               forward_ms=dict(hip=t_hf, torch=t_tf), forward_backward_ms=dict(hip=t_hb, torch=t_tb),
               backward_ms=dict(hip=t_hb - t_hf, torch=t_tb - t_tf),
               min_max_ms=dict(hip_fwd=spread[0], torch_fwd=spread[1], hip_fwd_bwd=spread[2], torch_fwd_bwd=spread[3]),
               hip_forward_hbm_fraction=dict(of_measured_6_29=bytes_pass / (t_hf * 1e-3) / HBM_MEASURED, of_spec_8=bytes_pass / (t_hf * 1e-3) / HBM_SPEC),
               hip_backward_hbm_fraction=dict(of_measured_6_29=bytes_pass / ((t_hb - t_hf) * 1e-3) / HBM_MEASURED,
                                              of_spec_8=bytes_pass / ((t_hb - t_hf) * 1e-3) / HBM_SPEC),
               max_abs_diff_forward=agree, rel_diff_grads=gagree)
    print(json.dumps(res, indent=1))
    return res


def generator_bench():
    B = 8
    base = {k: v for k, v in configs.MAP3DBN512.items() if isinstance(k, str)}
    base.update(dataset_length=4, nerf_noise=0)
    cond = {k: v.to(DEV) for k, v in synthetic.make_conditions(B, n_vertices=6890, seed=2).items()}
    cond["rasterized_segments"] = torch.randint(0, base["label_dim"], (B, base["gen_height"], base["gen_width"]), device=DEV)
    z = torch.randn(B, base["latent_dim"], device=DEV)
    out = {}
    runs = []
    for name, over, engine in (("label_layerwise", {"2d_label_input": True}, None), ("noflag_default", {}, None), ("noflag_f32", {}, "f32")):
        cfg = dict(base, **over)
        cfg["neural_field_cls"] = impl.COORDCONCATSIREN
        torch.manual_seed(3)
        G = gens.Map3DGenerator(**cfg).to(DEV).eval()
        G.set_device(DEV)
        if engine:
            G.synthesis_plan(DEV).engine = engine
        with torch.no_grad():
            fr, ph, styles = G._mapping(z, cfg)
            _, fmap, _, _, _ = G.render(fr, ph, cond, cfg["render_width"], cfg["render_height"], cfg["ray_start"], cfg["ray_end"],
                                        cfg["num_steps"], clamp_mode=cfg["clamp_mode"])
            block0 = G._block0_inputs(z, cond, cfg)
        hw = (cfg["render_height"], cfg["render_width"])
        runs.append((name, (lambda G=G, cfg=cfg: G.forward(z, cond, **cfg)),
                     (lambda G=G, fmap=fmap, styles=styles, block0=block0: torch.no_grad()(G._synthesize)(fmap, styles, hw, block0=block0)),
                     "layerwise" if G._layerwise_synthesis() else G.synthesis_plan(DEV).engine))
    med, spread = timed([r[1] for r in runs] + [r[2] for r in runs], warm=2, reps=8)
    for i, r in enumerate(runs):
        out[r[0]] = dict(synthesis_path=r[3], batch=B, forward_ms=med[i], synthesis_ms=med[len(runs) + i],
                         forward_min_max_ms=spread[i], synthesis_min_max_ms=spread[len(runs) + i])
    print(json.dumps(out, indent=1))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", type=str, default=os.path.join(ROOT, "profiles", "synth_input_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is nothing to time on a CPU"
    res = dict(device=torch.cuda.get_device_name(0), op=op_bench())
    torch.cuda.empty_cache()
    res["generator_512x256_hidden256"] = generator_bench()
    with open(args.json, "w") as fh:
        json.dump(res, fh, indent=1)
