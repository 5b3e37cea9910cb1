"""Time the SMPL forward (csrc/smpl_lbs.hip through lib/components/smpl.SMPL.forward) against the same formulas as a torch
composition on the GPU -- what a user without the kernels does, and what smplx does: einsum blend shapes and joints, batched
Rodrigues, the parents chain as a Python loop of batched 4 x 4 products, a [B,V,J] x [B,J,16] product for the per-vertex
transforms.  V = 6890, J = 24, NB = 10, B in {1, 40, 256}; both sides warmed up, then timed in alternation (device events around
each call, the device synchronised before the medians are taken).  Also prints the bytes each side moves at the least, computed
from the shapes.

    python tools/smpl_lbs_bench.py [--calls 30] [--warmup 5] [--json profiles/smpl_lbs_bench.json]
"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
smpl = importlib.import_module("3dhumangan_amd.lib.components.smpl")

SMPL_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)


def make_model(V, J, NB, seed=0):
    g = torch.Generator().manual_seed(seed)
    reg = torch.zeros(J, V)
    reg.scatter_(1, torch.randint(0, V, (J, 16), generator=g), 1.0)
    w = torch.zeros(V, J)
    w.scatter_(1, torch.stack([torch.randperm(J, generator=g)[:4] for _ in range(V)]), torch.softmax(torch.randn(V, 4, generator=g), 1))
    return {"v_template": torch.rand(V, 3, generator=g) - 0.5, "shapedirs": torch.randn(V, 3, NB, generator=g) * 0.02,
            "posedirs": torch.randn((J - 1) * 9, V * 3, generator=g) * 0.005, "J_regressor": reg / reg.sum(1, keepdim=True),
            "parents": torch.tensor(SMPL_PARENTS[:J]), "lbs_weights": w}


def torch_lbs(betas, pose, m, parents):
    """The composition in fp32 torch ops on the device -> (A, v_shaped, verts, J, J_transformed)."""
    B, n_j = pose.shape[0], len(parents)
    v_shaped = m["v_template"][None] + torch.einsum("bl,mkl->bmk", betas, m["shapedirs"])
    J = torch.einsum("bik,ji->bjk", v_shaped, m["J_regressor"])
    R = smpl.batch_rodrigues(pose.reshape(-1, 3)).view(B, n_j, 3, 3)
    feature = (R[:, 1:] - torch.eye(3, device=pose.device)).reshape(B, -1)
    v_posed = v_shaped + torch.matmul(feature, m["posedirs"]).view(B, -1, 3)
    rel = J.clone()
    rel[:, 1:] -= J[:, parents[1:]]
    local = torch.cat([torch.nn.functional.pad(R, [0, 0, 0, 1]), torch.nn.functional.pad(rel[..., None], [0, 0, 0, 1], value=1.0)], dim=3)
    chain = [local[:, 0]]
    for i in range(1, n_j):
        chain.append(torch.matmul(chain[parents[i]], local[:, i]))
    G = torch.stack(chain, dim=1)
    A = G - torch.nn.functional.pad(torch.matmul(G, torch.nn.functional.pad(J[..., None], [0, 0, 0, 1])), [3, 0])
    T = torch.matmul(m["lbs_weights"][None].expand(B, -1, -1), A.view(B, n_j, 16)).view(B, -1, 4, 4)
    homo = torch.cat([v_posed, torch.ones_like(v_posed[..., :1])], dim=2)
    verts = torch.matmul(T, homo[..., None])[:, :, :3, 0]
    return A, v_shaped, verts, J, G[:, :, :3, 3]


def bench(B, V, J, NB, calls, warmup):
    dev = torch.device("cuda")
    model = make_model(V, J, NB)
    body = smpl.SMPL(model, device=dev)
    m = {k: v.to(dev) for k, v in model.items() if k != "parents"}
    parents = [int(p) for p in model["parents"]]
    g = torch.Generator().manual_seed(B)
    betas = torch.randn(B, NB, generator=g).to(dev)
    pose = ((torch.rand(B, J * 3, generator=g) - 0.5) * 2.0).to(dev)
    ours = lambda: body.forward(betas, pose[:, 3:], pose[:, :3])                           # noqa: E731
    theirs = lambda: torch_lbs(betas, pose, m, parents)                                    # noqa: E731
    with torch.no_grad():
        a, b = ours(), theirs()
        err = float((a["vertices"] - b[2]).abs().max())
        for _ in range(warmup):
            ours(), theirs()
        torch.cuda.synchronize()
        ev = {"hip": [], "torch": []}
        for _ in range(calls):                                                              # alternating: both see the same machine
            for name, fn in (("hip", ours), ("torch", theirs)):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                fn()
                e.record()
                ev[name].append((s, e))
        torch.cuda.synchronize()
    med = {k: sorted(s.elapsed_time(e) for s, e in v)[len(v) // 2] for k, v in ev.items()}
    P, tiles = (J - 1) * 9, (B + 7) // 8
    # least traffic of the kernels: posedirs once per tile of 8 items, shapedirs once per tile, the model's small arrays once,
    # v_shaped written and read, verts written, A / joints / feature written and read
    hip_bytes = 4 * (tiles * P * 3 * V + tiles * 3 * V * NB + 3 * V + V * J + 3 * B * 3 * V + B * (2 * J * 16 + 2 * P + 6 * J))
    # least traffic of the composition: every operand and result of every op once, the [B,V,16] transforms written and read
    torch_bytes = 4 * (P * 3 * V + 3 * V * NB + 3 * V + J * V + V * J + B * V * (3 * 2 + 3 * 3 + 16 * 2 + 4 * 2 + 3))
    return {"B": B, "V": V, "J": J, "NB": NB, "calls": calls, "hip_median_ms": med["hip"], "torch_median_ms": med["torch"],
            "speedup": med["torch"] / med["hip"], "hip_min_bytes": hip_bytes, "torch_min_bytes": torch_bytes,
            "max_abs_vertex_difference": err}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 40, 256])
    ap.add_argument("--json", type=str, default=os.path.join(ROOT, "profiles", "smpl_lbs_bench.json"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("smpl_lbs_bench needs a GPU: a CPU run says nothing about these times")
    rows = []
    for B in opt.batches:
        r = bench(B, 6890, 24, 10, opt.calls, opt.warmup)
        rows.append(r)
        print(f"B={B:3d}: HIP {r['hip_median_ms'] * 1e3:8.1f} us ({r['hip_min_bytes'] / 1e6:.1f} MB at least) | torch "
              f"{r['torch_median_ms'] * 1e3:8.1f} us ({r['torch_min_bytes'] / 1e6:.1f} MB at least) | x{r['speedup']:.2f} | "
              f"max |dv| {r['max_abs_vertex_difference']:.1e}", flush=True)
    with open(opt.json, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
