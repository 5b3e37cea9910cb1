"""A pure-torch restatement of the SMPL forward -- the reference's lbs() (lib/components/smpl.py:11-107) with smplx's published
definitions of blend_shapes, vertices2joints, batch_rodrigues and batch_rigid_transform written out -- evaluated in whatever
dtype it is called with (float64: the oracle of the GPU tests; float32: the yardstick of their tolerance).  Also the case grid
that tests/test_smpl_cpu.py and tests/test_gpu_smpl.py share."""
import itertools
import math

import torch

MODEL_KEYS = ("v_template", "shapedirs", "posedirs", "J_regressor", "parents", "lbs_weights")
SMPL_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)


def batch_rodrigues(rot_vecs):
    angle = torch.norm(rot_vecs + 1e-8, dim=1, keepdim=True)
    d = rot_vecs / angle
    zero = torch.zeros_like(d[:, 0])
    K = torch.stack([zero, -d[:, 2], d[:, 1], d[:, 2], zero, -d[:, 0], -d[:, 1], d[:, 0], zero], dim=1).view(-1, 3, 3)
    s, c = torch.sin(angle)[:, None], torch.cos(angle)[:, None]
    return torch.eye(3, dtype=rot_vecs.dtype)[None] + s * K + (1 - c) * torch.bmm(K, K)


def lbs(betas, pose, v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights, pose2rot=True, transl=None):
    """-> (A [B,J,4,4], v_shaped [B,V,3], verts [B,V,3], J [B,J,3], J_transformed [B,J,3]) in betas' dtype."""
    dt = betas.dtype
    v_template, shapedirs, posedirs, J_regressor, lbs_weights, pose = (
        t.to(dt) for t in (v_template, shapedirs, posedirs, J_regressor, lbs_weights, pose))
    B = max(betas.shape[0], pose.shape[0])
    n_j = J_regressor.shape[0]
    parents = [int(p) for p in torch.as_tensor(parents).tolist()]
    v_shaped = (v_template[None] + torch.einsum("bl,mkl->bmk", betas, shapedirs)).expand(B, -1, -1)
    J = torch.einsum("bik,ji->bjk", v_shaped, J_regressor)
    R = batch_rodrigues(pose.reshape(-1, 3)).view(B, n_j, 3, 3) if pose2rot else pose.reshape(B, n_j, 3, 3)
    pose_feature = (R[:, 1:] - torch.eye(3, dtype=dt)).reshape(B, -1)
    v_posed = v_shaped + torch.matmul(pose_feature, posedirs).view(B, -1, 3)
    G = [None] * n_j
    for i in range(n_j):
        L = torch.zeros(B, 4, 4, dtype=dt)
        L[:, :3, :3] = R[:, i]
        L[:, :3, 3] = J[:, i] - (J[:, parents[i]] if i > 0 else 0)
        L[:, 3, 3] = 1
        G[i] = L if i == 0 else torch.matmul(G[parents[i]], L)
    G = torch.stack(G, dim=1)
    J_transformed = G[:, :, :3, 3]
    A = G.clone()
    A[:, :, :3, 3] = G[:, :, :3, 3] - torch.einsum("bjrc,bjc->bjr", G[:, :, :3, :3], J)
    T = torch.matmul(lbs_weights[None].expand(B, -1, -1), A.view(B, n_j, 16)).view(B, -1, 4, 4)
    homo = torch.cat([v_posed, torch.ones(B, v_posed.shape[1], 1, dtype=dt)], dim=2)
    verts = torch.matmul(T, homo[..., None])[:, :, :3, 0]
    if transl is not None:
        verts = verts + transl.to(dt)[:, None]
    return A, v_shaped.contiguous(), verts, J, J_transformed


OUTPUTS = ("A", "v_shaped", "verts", "J", "J_transformed")
CAP = 1e-5          # no case may lose more than this (relative to each output's maximum) in the fp32 composition alone
FACTOR = 8          # a different summation order in the (J-1)*9- and J-term sums, FMA contraction, a few ulp in sin / cos


def composition_error(case):
    """-> (float64 outputs, err32): err32 = max over the five outputs of max|fp32 evaluation - float64 evaluation| / max|float64|,
    the restatement's own rounding on this case's inputs.  The bar of a GPU case is min(FACTOR * err32, CAP), and err32 <= CAP must hold."""
    m = case["model"]
    args64 = [case["betas"].double(), case["pose"].double()] + [m[k].double() if k != "parents" else m[k] for k in MODEL_KEYS]
    args32 = [a.float() if torch.is_floating_point(a) else a for a in args64]
    tr = case["transl"]
    o64 = lbs(*args64, pose2rot=case["pose2rot"], transl=None if tr is None else tr.double())
    o32 = lbs(*args32, pose2rot=case["pose2rot"], transl=None if tr is None else tr.float())
    err = max(float((a.double() - b).abs().max() / b.abs().max()) for a, b in zip(o32, o64))
    return o64, err


TREES = ("smpl", "chain", "star")


def make_parents(tree, n_j):
    if tree == "chain":
        return [-1] + list(range(n_j - 1))
    if tree == "star":
        return [-1] + [0] * (n_j - 1)
    # SMPL's tree; joints past its 24 hang off earlier ones the way SMPL-X's hands and face do (a fixed pseudo-random pattern)
    return [SMPL_PARENTS[i] if i < 24 else (i * 7 + 3) % 24 for i in range(n_j)]


def make_model(V, n_j, NB, tree, seed=0):
    """A seeded model of the given shape (float32 values): a body-sized template, shape directions of a few centimetres, pose
    directions of a few millimetres, a sparse convex joint regressor and skinning weights with four joints per vertex."""
    g = torch.Generator().manual_seed(seed * 1000 + V * 7 + n_j * 3 + NB)
    v_template = (torch.rand(V, 3, generator=g) - 0.5) * torch.tensor([0.6, 1.7, 0.3])
    shapedirs = torch.randn(V, 3, NB, generator=g) * 0.02
    posedirs = torch.randn((n_j - 1) * 9, V * 3, generator=g) * 0.005
    k = min(8, V)
    reg = torch.zeros(n_j, V)
    reg.scatter_(1, torch.stack([torch.randperm(V, generator=g)[:k] for _ in range(n_j)]),
                 torch.softmax(torch.randn(n_j, k, generator=g), dim=1))
    kw = min(4, n_j)
    w = torch.zeros(V, n_j)
    w.scatter_(1, torch.stack([torch.randperm(n_j, generator=g)[:kw] for _ in range(V)]),
               torch.softmax(torch.randn(V, kw, generator=g) * 2, dim=1))
    return {"v_template": v_template, "shapedirs": shapedirs, "posedirs": posedirs, "J_regressor": reg,
            "parents": torch.tensor(make_parents(tree, n_j)), "lbs_weights": w}


def make_case(V, B, NB, n_j, pose2rot, with_transl, tree, seed=0):
    """One case of the grid: poses with angles up to pi; item 0 carries an exactly zero pose, the last item one joint at angle
    pi - 1e-4 (both sit in the same item when B = 1: the zero pose with that one joint turned)."""
    g = torch.Generator().manual_seed(seed * 77 + V + 13 * B + 5 * NB + n_j + 2 * int(pose2rot) + int(with_transl))
    model = make_model(V, n_j, NB, tree, seed)
    axis = torch.randn(B, n_j, 3, generator=g)
    axis = axis / axis.norm(dim=-1, keepdim=True)
    pose = axis * (torch.rand(B, n_j, 1, generator=g) * math.pi)
    pose[0] = 0.0
    pose[B - 1, n_j - 1] = axis[B - 1, n_j - 1] * (math.pi - 1e-4)
    if not pose2rot:
        pose = batch_rodrigues(pose.double().reshape(-1, 3)).view(B, n_j, 3, 3).float()
    else:
        pose = pose.reshape(B, n_j * 3)
    betas = torch.randn(B, NB, generator=g)
    transl = torch.randn(B, 3, generator=g) * 0.5 if with_transl else None
    return {"model": model, "betas": betas, "pose": pose, "pose2rot": pose2rot, "transl": transl}


GRID_V, GRID_B, GRID_NB, GRID_J = (1, 67, 301), (1, 3, 9), (0, 1, 10, 17), (2, 24, 55)


def grid():
    """Every combination of the grid: (V, B, NB, J, pose2rot, transl, tree)."""
    return itertools.product(GRID_V, GRID_B, GRID_NB, GRID_J, (True, False), (False, True), TREES)
