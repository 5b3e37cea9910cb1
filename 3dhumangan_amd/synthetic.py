"""Procedural stand-in for the SHHQ/SMPL `conditions` dict (A0 schema).

The reference builds this dict from a licensed SMPL model + dataset files
(lib/data/datasets.py:117-181, lib/data/preprocessor.py:72-97) which cannot be
shipped.  This module produces tensors with the same keys, shapes, dtypes and
geometric conventions from a seeded procedural body: a 24-joint kinematic tree,
`n_vertices` points on capsules around the bones, dense LBS weights whose rows
sum to one, a random (or canonical) pose driven through forward kinematics, and
the weak-perspective camera of the fix_body coordinate mode.

Everything is computed on CPU in fp32 so the same bytes can be handed to the
oracle and to the HIP path.
"""
import math

import torch

PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)

_REST = (
    (0.00, 0.00, 0.00), (0.07, -0.09, 0.00), (-0.07, -0.09, 0.00), (0.00, 0.11, -0.01),
    (0.10, -0.47, 0.01), (-0.10, -0.47, 0.01), (0.00, 0.25, 0.00), (0.09, -0.87, -0.02),
    (-0.09, -0.87, -0.02), (0.00, 0.30, 0.01), (0.11, -0.93, 0.10), (-0.11, -0.93, 0.10),
    (0.00, 0.51, -0.02), (0.08, 0.42, -0.01), (-0.08, 0.42, -0.01), (0.00, 0.60, 0.02),
    (0.17, 0.44, -0.02), (-0.17, 0.44, -0.02), (0.43, 0.44, -0.03), (-0.43, 0.44, -0.03),
    (0.68, 0.44, -0.03), (-0.68, 0.44, -0.03), (0.76, 0.44, -0.03), (-0.76, 0.44, -0.03),
)
_RADIUS = (0.12, 0.08, 0.08, 0.12, 0.06, 0.06, 0.12, 0.045, 0.045, 0.12, 0.04, 0.04,
           0.05, 0.06, 0.06, 0.09, 0.05, 0.05, 0.04, 0.04, 0.035, 0.035, 0.03, 0.03)

FOCAL = 1.0 / math.tan(math.pi * 12 / 180 / 2)     # lib/data/datasets.py:119-120


def _axis_angle_to_matrix(aa):
    theta = aa.norm(dim=-1, keepdim=True).clamp_min(1e-8)
    k = aa / theta
    K = torch.zeros(aa.shape[0], 3, 3)
    K[:, 0, 1], K[:, 0, 2] = -k[:, 2], k[:, 1]
    K[:, 1, 0], K[:, 1, 2] = k[:, 2], -k[:, 0]
    K[:, 2, 0], K[:, 2, 1] = -k[:, 1], k[:, 0]
    s = torch.sin(theta)[..., None]
    c = torch.cos(theta)[..., None]
    return torch.eye(3)[None] + s * K + (1 - c) * (K @ K)


def _rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return torch.tensor([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=torch.float32)


def _rot_y(a):
    c, s = math.cos(a), math.sin(a)
    return torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=torch.float32)


def template_body(n_vertices=6890, seed=0):
    """-> rest joints [24,3], rest vertices [V,3], lbs weights [V,24]."""
    g = torch.Generator().manual_seed(1000 + seed)
    J = torch.tensor(_REST, dtype=torch.float32)
    rad = torch.tensor(_RADIUS, dtype=torch.float32)
    par = torch.tensor([max(p, 0) for p in PARENTS])
    a, b = J[par], J                                        # bone: parent -> joint
    blen = (b - a).norm(dim=-1)
    blen[0] = 0.10
    share = blen * rad
    bone = torch.multinomial(share / share.sum(), n_vertices, replacement=True, generator=g)
    t = torch.rand(n_vertices, generator=g)
    ang = torch.rand(n_vertices, generator=g) * 2 * math.pi
    axis = b[bone] - a[bone]
    axis[bone == 0] = torch.tensor([0.0, 0.10, 0.0])
    axis_n = axis / axis.norm(dim=-1, keepdim=True)
    helper = torch.where(axis_n[:, 1:2].abs() < 0.9, torch.tensor([[0.0, 1.0, 0.0]]), torch.tensor([[1.0, 0.0, 0.0]]))
    u = torch.cross(axis_n, helper.expand_as(axis_n), dim=-1)
    u = u / u.norm(dim=-1, keepdim=True)
    w = torch.cross(axis_n, u, dim=-1)
    r = rad[bone] * (0.85 + 0.3 * torch.rand(n_vertices, generator=g))
    V = a[bone] + axis * t[:, None] + r[:, None] * (torch.cos(ang)[:, None] * u + torch.sin(ang)[:, None] * w)
    # dense LBS weights: softmax over the 4 nearest joints, zero elsewhere
    d2 = torch.cdist(V, J).square()
    near = torch.topk(d2, 4, dim=1, largest=False)
    wts = torch.zeros(n_vertices, 24)
    wts.scatter_(1, near.indices, torch.softmax(-near.values / 0.01, dim=1))
    return J, V.contiguous(), wts.contiguous()


def forward_kinematics(J, rot):
    """rot [24,3,3] local rotations -> (A [24,4,4] rest->posed transforms, posed joints [24,3])."""
    G = [None] * 24
    for j in range(24):
        T = torch.eye(4)
        T[:3, :3] = rot[j]
        T[:3, 3] = J[j] - (J[PARENTS[j]] if PARENTS[j] >= 0 else torch.zeros(3))
        G[j] = T if PARENTS[j] < 0 else G[PARENTS[j]] @ T
    G = torch.stack(G)
    posed = G[:, :3, 3].clone()
    A = G.clone()
    A[:, :3, 3] = G[:, :3, 3] - torch.einsum("jab,jb->ja", G[:, :3, :3], J)
    return A, posed


def make_conditions(batch, n_vertices=6890, seed=0, pose_scale=0.5, scale=0.8, h_angle=0.0, v_angle=0.0):
    """Synthetic `conditions` dict (CPU fp32).  pose_scale=0 gives the canonical pose.

    Keys/shapes follow the consumer at lib/generators/map3d_generator.py:388-395."""
    J, V, W = template_body(n_vertices, seed)
    flip = torch.eye(4)
    flip[:3, :3] = _rot_x(math.pi)                          # cano_rotation, datasets.py:141
    out = {k: [] for k in ("skeletons_xyz", "vertices", "fk_matrices", "cam2world_matrices")}
    g = torch.Generator().manual_seed(2000 + seed)
    for b in range(batch):
        aa = (torch.rand(24, 3, generator=g) - 0.5) * 2 * pose_scale
        aa[0] = 0
        A, posed = forward_kinematics(J, _axis_angle_to_matrix(aa) if pose_scale > 0 else torch.eye(3).repeat(24, 1, 1))
        A = flip[None] @ A
        VA = torch.einsum("vj,jab->vab", W, A)
        verts = torch.einsum("vab,vb->va", VA, torch.cat([V, torch.ones(n_vertices, 1)], 1))[:, :3]
        joints = posed @ flip[:3, :3].T
        hb = h_angle if isinstance(h_angle, float) else float(h_angle[b])
        vb = v_angle if isinstance(v_angle, float) else float(v_angle[b])
        body_rot = torch.eye(4)
        body_rot[:3, :3] = _rot_x(math.pi - vb) @ _rot_y(-hb)   # preprocessor.py:82-88 with identity root
        T = torch.eye(4)
        T[2, 3] = FOCAL / scale
        out["skeletons_xyz"].append(joints)
        out["vertices"].append(verts)
        out["fk_matrices"].append(A)
        out["cam2world_matrices"].append(torch.inverse(T @ body_rot))
    cond = {k: torch.stack(v).float().contiguous() for k, v in out.items()}
    tp = V.clone()
    tp[:, 1] += 0.35                                        # datasets.py:159-160
    cond["tpose_vertices"] = tp[None].repeat(batch, 1, 1).contiguous()
    cond["lbs_weights"] = W[None].repeat(batch, 1, 1).contiguous()
    K = torch.eye(4)
    K[0, 0] = K[1, 1] = FOCAL
    cond["intrinsics"] = K[None].repeat(batch, 1, 1).contiguous()
    cond["scales"] = torch.full((batch,), float(scale))
    # camera pieces the reference's preprocessor consumes (datasets.py:127-139, preprocessor.py:80-93)
    T = torch.eye(4)
    T[2, 3] = FOCAL / scale
    cond["R"] = torch.eye(4)[None].repeat(batch, 1, 1)
    cond["T"] = T[None].repeat(batch, 1, 1)
    cond["full_pose"] = torch.eye(3)[None, None].repeat(batch, 24, 1, 1)
    return cond


# The camera front-end lives in lib/data/conditions.py (pinned to the reference's preprocessor); the old names stay importable.
from .lib.data.conditions import CameraPreprocessor as SyntheticPreprocessor, euler_xyz_to_matrix  # noqa: E402,F401


# --- a triangulated stand-in for the SMPL mesh (the rasteriser's input) -----------------------------------------------------

TUBE_SEGMENTS = 12          # vertices per ring
TUBE_RINGS = 574            # rings over the 24 bones: 24 * 574 = 13 776 faces (SMPL's count), 12 * 574 + 48 = 6 936 vertices


def tube_body():
    """A closed triangulated tube around each of the 24 bones of `template_body` (bone j runs from its parent joint to joint j;
    the root's is a 0.10 stub upwards), capped by a pole at each end.  -> rest joints [24,3], rest vertices [V,3], LBS weights
    [V,24] (the same rule as template_body: softmax over the 4 nearest joints), faces int64 [F,3], per-face part labels int64
    [F] (the bone index 0..23).  F = 13 776 and V = 6 936: SMPL-sized, deterministic, no licensed asset."""
    J = torch.tensor(_REST, dtype=torch.float64)
    rad = torch.tensor(_RADIUS, dtype=torch.float64)
    par = [max(p, 0) for p in PARENTS]
    blen = (J - J[par]).norm(dim=-1)
    blen[0] = 0.10
    rings = (blen / blen.sum() * (TUBE_RINGS - 3 * 24)).floor().long() + 3
    order = torch.argsort(blen, descending=True)
    for i in range(TUBE_RINGS - int(rings.sum())):
        rings[order[i % 24]] += 1
    k = TUBE_SEGMENTS
    ang = torch.arange(k, dtype=torch.float64) * (2 * math.pi / k)
    verts, faces, labels = [], [], []
    n_v = 0
    for j in range(24):
        a = J[par[j]]
        axis = J[j] - a if j > 0 else torch.tensor([0.0, 0.10, 0.0], dtype=torch.float64)
        axis_n = axis / axis.norm()
        helper = torch.tensor([0.0, 1.0, 0.0] if abs(float(axis_n[1])) < 0.9 else [1.0, 0.0, 0.0], dtype=torch.float64)
        u = torch.linalg.cross(axis_n, helper)
        u = u / u.norm()
        w = torch.linalg.cross(axis_n, u)
        n = int(rings[j])
        t = torch.linspace(0, 1, n, dtype=torch.float64)
        ring = a + t[:, None, None] * axis + rad[j] * (torch.cos(ang)[None, :, None] * u + torch.sin(ang)[None, :, None] * w)
        poles = torch.stack([a - 0.5 * rad[j] * axis_n, a + axis + 0.5 * rad[j] * axis_n])
        verts += [ring.reshape(-1, 3), poles]
        idx = lambda i, m: n_v + i * k + (m % k)                                          # noqa: E731
        pa, pb = n_v + n * k, n_v + n * k + 1
        tri = []
        for i in range(n - 1):
            for m in range(k):
                tri += [(idx(i, m), idx(i, m + 1), idx(i + 1, m + 1)), (idx(i, m), idx(i + 1, m + 1), idx(i + 1, m))]
        for m in range(k):
            tri += [(pa, idx(0, m + 1), idx(0, m)), (pb, idx(n - 1, m), idx(n - 1, m + 1))]
        faces.append(torch.tensor(tri, dtype=torch.int64))
        labels.append(torch.full((len(tri),), j, dtype=torch.int64))
        n_v += n * k + 2
    V = torch.cat(verts).float()
    Jf = J.float()
    d2 = torch.cdist(V, Jf).square()
    near = torch.topk(d2, 4, dim=1, largest=False)
    W = torch.zeros(V.shape[0], 24)
    W.scatter_(1, near.indices, torch.softmax(-near.values / 0.01, dim=1))
    return Jf, V.contiguous(), W.contiguous(), torch.cat(faces).contiguous(), torch.cat(labels).contiguous()


def _random_pose(J, g, pose_scale):
    aa = (torch.rand(24, 3, generator=g) - 0.5) * 2 * pose_scale
    aa[0] = 0
    return forward_kinematics(J, _axis_angle_to_matrix(aa) if pose_scale > 0 else torch.eye(3).repeat(24, 1, 1))


def make_mesh_conditions(batch, seed=0, pose_scale=0.5, scale=0.8):
    """`conditions` of make_conditions' schema on the tube_body mesh (random pose per item, drawn as make_conditions draws
    them), and the mesh topology: -> (cond, faces [F,3] int64, faces_to_labels [F] int64).  The cameras are those of the
    canonical view; CameraPreprocessor.forward_with_rotation sets per-item views."""
    J, V, W, faces, labels = tube_body()
    n = V.shape[0]
    flip = torch.eye(4)
    flip[:3, :3] = _rot_x(math.pi)
    g = torch.Generator().manual_seed(2000 + seed)
    verts, fks, joints = [], [], []
    for _ in range(batch):
        A, posed = _random_pose(J, g, pose_scale)
        A = flip[None] @ A
        VA = torch.einsum("vj,jab->vab", W, A)
        verts.append(torch.einsum("vab,vb->va", VA, torch.cat([V, torch.ones(n, 1)], 1))[:, :3])
        fks.append(A)
        joints.append(posed @ flip[:3, :3].T)
    T = torch.eye(4)
    T[2, 3] = FOCAL / scale
    body_rot = torch.eye(4)
    body_rot[:3, :3] = _rot_x(math.pi)
    tp = V.clone()
    tp[:, 1] += 0.35
    K = torch.eye(4)
    K[0, 0] = K[1, 1] = FOCAL
    rep = lambda t: t[None].repeat(batch, *([1] * t.dim())).contiguous()                  # noqa: E731
    cond = {"skeletons_xyz": torch.stack(joints).contiguous(), "vertices": torch.stack(verts).contiguous(),
            "fk_matrices": torch.stack(fks).contiguous(), "cam2world_matrices": rep(torch.inverse(T @ body_rot)),
            "tpose_vertices": rep(tp), "lbs_weights": rep(W), "intrinsics": rep(K), "scales": torch.full((batch,), float(scale)),
            "R": rep(torch.eye(4)), "T": rep(T), "full_pose": torch.eye(3)[None, None].repeat(batch, 24, 1, 1)}
    return cond, faces, labels


def make_smpl_model(seed=0, num_betas=10):
    """A procedural SMPL-shaped body model on the tube_body mesh, what lib/components/smpl.SMPL is built from (and what
    `--smpl-model` of the sample app loads from an .npz): v_template [V,3], parents [24], lbs_weights [V,24], a sparse convex
    J_regressor [24,V] (each joint is the softmax-weighted mean of its 32 nearest vertices, rows sum to 1 -- so the regressed
    joints sit near, not on, the tube's rest joints), small seeded shapedirs [V,3,num_betas] (smooth in space: centimetres per
    unit beta) and posedirs [207, 3V] (millimetres), plus faces, faces_to_labels and joints_index for the front-end.  A dict
    of numpy arrays."""
    J, V, W, faces, labels = tube_body()
    n, g = V.shape[0], torch.Generator().manual_seed(3000 + seed)
    near = torch.topk(torch.cdist(J, V).square(), 32, dim=1, largest=False)
    reg = torch.zeros(24, n)
    reg.scatter_(1, near.indices, torch.softmax(-near.values / 0.005, dim=1))
    # shape directions: low-frequency fields of the rest position, so that neighbouring vertices move together
    freq = torch.randn(num_betas, 3, 3, generator=g) * 2.0
    phase = torch.rand(num_betas, 3, generator=g) * 2 * math.pi
    shapedirs = 0.02 * torch.sin(torch.einsum("lkc,vc->vkl", freq, V) + phase.T[None])
    posedirs = 0.002 * torch.randn(23 * 9, n * 3, generator=g)
    return {"v_template": V.numpy(), "shapedirs": shapedirs.contiguous().numpy(), "posedirs": posedirs.numpy(),
            "J_regressor": reg.numpy(), "parents": torch.tensor(PARENTS).numpy(), "lbs_weights": W.numpy(),
            "faces": faces.numpy(), "faces_to_labels": labels.numpy(), "joints_index": torch.arange(24).numpy()}


def make_pose_sequence(n, seed=0, num_betas=10, pose_scale=0.5, scale=0.8):
    """A smooth seeded motion of `n` frames for a 24-joint body: poses [n,24,3] axis-angle (every joint swings sinusoidally about
    a seeded axis with a seeded amplitude <= pose_scale, period and phase; the root stays upright), betas [1,num_betas] and
    orig_cam [n,4] (the weak-perspective camera of make_conditions) -- the arrays `--pose-sequence` of the sample app loads from
    an .npz.  Frames with equal time (n = 1 aside, frame i sits at t = i / n) are equal."""
    g = torch.Generator().manual_seed(4000 + seed)
    axis = torch.randn(24, 3, generator=g)
    axis = axis / axis.norm(dim=-1, keepdim=True)
    amp = torch.rand(24, 1, generator=g) * pose_scale
    cycles = torch.randint(1, 3, (24, 1), generator=g).float()
    phase = torch.rand(24, 1, generator=g) * 2 * math.pi
    t = torch.arange(n).float()[:, None, None] / max(n, 1)
    poses = axis[None] * amp[None] * torch.sin(2 * math.pi * cycles[None] * t + phase[None])
    poses[:, 0] = 0
    cam = torch.tensor([[2 * scale, 2 * scale, 0.0, 0.0]]).repeat(n, 1)
    return {"poses": poses.contiguous().numpy(), "betas": (0.5 * torch.randn(1, num_betas, generator=g)).numpy(), "orig_cam": cam.numpy()}


def make_smpl_record(seed=0, pose_scale=0.5, scale=0.8):
    """One SMPL regression record of the shape lib/data/conditions.preprocess_smpl_fix_body reads, on the tube_body mesh, plus
    the assets the front-end needs beside it (joints_index, smpl_tpose_vertices, faces, faces_to_labels): a dict of numpy
    arrays, what `--smpl-record` of the sample app loads from an .npz."""
    J, V, W, faces, labels = tube_body()
    g = torch.Generator().manual_seed(2000 + seed)
    A, posed = _random_pose(J, g, pose_scale)
    return {"orig_cam": torch.tensor([[2 * scale, 2 * scale, 0.0, 0.0]]).numpy(), "joints": posed[None].numpy(),
            "full_pose": torch.eye(3)[None, None].repeat(1, 24, 1, 1).numpy(), "tpose_vertices": V[None].numpy(),
            "fk_matrices": A[None].numpy(), "lbs_weights": W.numpy(), "betas": torch.zeros(1, 10).numpy(),
            "joints_index": torch.arange(24).numpy(), "smpl_tpose_vertices": V.numpy(), "faces": faces.numpy(),
            "faces_to_labels": labels.numpy()}


class SyntheticTrainingSource:
    """A learnable toy task that needs no assets, in the trainer's data-source protocol (lib/trainers/phase_trainer.py):
    `length` posed tube bodies (make_mesh_conditions); the "photograph" of a body is a fixed palette applied to its UNROTATED
    rasterisation plus a little seeded noise, and `body_segments` is that rasterisation.

        batches(batch, step, device) -> dict: images [B,3,H,W] in [-1, 1], body_segments [B,H,W] int64, indices [B] and the
                                              condition entries CameraPreprocessor and the generator read
        faces [F,3], faces_to_labels [F]      the topology CameraPreprocessor.init_smpl takes
    Item i of step s is (s * batch + i) % length.  The rasterisation runs on the device (HIP), once per item and size."""

    def __init__(self, length=8, gen_height=256, gen_width=128, seed=0, noise=0.02, label_dim=26):
        self.length, self.size, self.seed, self.noise = int(length), (int(gen_height), int(gen_width)), int(seed), float(noise)
        self.conditions, self.faces, self.faces_to_labels = make_mesh_conditions(self.length, seed=seed)
        g = torch.Generator().manual_seed(4000 + seed)
        self.palette = torch.rand(label_dim + 2, 3, generator=g) * 2 - 1
        self.palette[:2] = 1.0                                               # labels 0 / 1: the white background
        self._cache = {}

    def _rasterised(self, device):
        key = str(device)
        if key not in self._cache:
            pre = SyntheticPreprocessor(device)
            pre.init_smpl(self.faces, self.faces_to_labels)
            cond = {k: v.to(device) for k, v in self.conditions.items()}
            zero = torch.zeros(self.length)
            seg = pre.forward_with_rotation(cond, zero, zero, zero, gen_height=self.size[0], gen_width=self.size[1])["rasterized_segments"]
            self._cache[key] = (cond, seg.long(), self.palette.to(device)[seg.long().clamp(0, self.palette.shape[0] - 1)].permute(0, 3, 1, 2))
        return self._cache[key]

    def batches(self, batch, step, device):
        cond, seg, rgb = self._rasterised(device)
        idx = (torch.arange(batch) + int(step) * batch) % self.length
        g = torch.Generator().manual_seed(self.seed * 7919 + int(step))
        noise = (torch.randn(batch, 3, *self.size, generator=g) * self.noise).to(device)
        idx_d = idx.to(device)
        out = {k: v[idx_d].contiguous() for k, v in cond.items()}
        out.update(images=(rgb[idx_d] + noise).clamp(-1, 1).contiguous(), body_segments=seg[idx_d].contiguous(), indices=idx_d)
        return out


RECORD_ASSETS = ("joints_index", "smpl_tpose_vertices", "faces", "faces_to_labels")


def write_example_dataset(root, length=8, height=64, width=32, seed=0, records="npz"):
    """Write a procedural dataset of `length` items in the layout lib/data/datasets.SHHQDataset reads (CPU only, no licensed
    asset): images/ (seeded smooth colours), masks/ (an ellipse, 255 inside), body_seg/ (label bands 0..24 inside the ellipse, as a
    3-channel PNG whose channel 0 counts), inversions/*.npy (seeded latents [512]), smpl/ (make_smpl_record's records without the
    assets, as plain-array .npz, or joblib .pkl with records="pkl") and smpl_model.npz (make_smpl_model).  -> root."""
    import os

    import numpy as np
    from PIL import Image
    if records not in ("npz", "pkl"):
        raise ValueError(f"records must be 'npz' or 'pkl', got {records!r}")
    for d in ("images", "masks", "body_seg", "inversions", "smpl"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    np.savez(os.path.join(root, "smpl_model.npz"), **make_smpl_model(seed))
    yy, xx = np.meshgrid(np.linspace(-1, 1, height), np.linspace(-1, 1, width), indexing="ij")
    for i in range(length):
        rng = np.random.default_rng(seed * 100_003 + i)
        name = f"{i + 1:06d}"
        freq, phase = rng.uniform(0.5, 3.0, (3, 2)), rng.uniform(0, 2 * math.pi, 3)
        rgb = np.stack([0.5 + 0.5 * np.sin(freq[c, 0] * yy * math.pi + freq[c, 1] * xx * math.pi + phase[c]) for c in range(3)], -1)
        cy, cx, ry, rx = rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.6, 0.9), rng.uniform(0.5, 0.8)
        inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
        band = np.clip(((yy - cy + ry) / (2 * ry) * 25).astype(np.int64), 0, 24)
        seg = np.where(inside, band, 0).astype(np.uint8)
        Image.fromarray((rgb * 255).round().astype(np.uint8)).save(os.path.join(root, "images", name + ".png"))
        Image.fromarray(np.where(inside, 255, 0).astype(np.uint8)).save(os.path.join(root, "masks", name + ".png"))
        Image.fromarray(np.stack([seg, seg, seg], -1)).save(os.path.join(root, "body_seg", name + ".png"))
        np.save(os.path.join(root, "inversions", name + ".npy"), rng.standard_normal(512).astype(np.float32))
        rec = {k: v for k, v in make_smpl_record(seed=seed * 100_003 + i).items() if k not in RECORD_ASSETS}
        if records == "npz":
            np.savez(os.path.join(root, "smpl", name + ".npz"), **rec)
        else:
            import joblib
            joblib.dump(rec, os.path.join(root, "smpl", name + ".pkl"))
    return root
