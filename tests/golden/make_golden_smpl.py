"""Golden fixture of the SMPL forward: the reference's own lbs() (lib/components/smpl.py:11-107) on a tiny seeded model.

BUILD CONTAINER ONLY, like make_golden.py: the reference module is imported through _ref_import, driven with seeded inputs, and
only *data* is stored.  The four smplx functions lbs() calls (pinned smplx, not installed) are replaced in that module's namespace
by the functional stand-ins below, which follow smplx's published definitions -- as the kNN stand-in does for pytorch3d.  So the
fixture pins the reference's own glue (array layouts, the order of the pose feature, the return order, the skinning), and the
smplx boundary itself stays unpinned.
Run:  python tests/golden/make_golden_smpl.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import  # noqa: E402

_ref_import.install()
import lib.components.smpl as ref_smpl  # noqa: E402
import _smpl_reference as SR  # noqa: E402


def blend_shapes(betas, shape_disps):
    return torch.einsum("bl,mkl->bmk", [betas, shape_disps])


def vertices2joints(J_regressor, vertices):
    return torch.einsum("bik,ji->bjk", [vertices, J_regressor])


def batch_rodrigues(rot_vecs, epsilon=1e-8):
    n = rot_vecs.shape[0]
    angle = torch.norm(rot_vecs + epsilon, dim=1, keepdim=True)
    rot_dir = rot_vecs / angle
    cos, sin = torch.cos(angle)[:, None], torch.sin(angle)[:, None]
    rx, ry, rz = torch.split(rot_dir, 1, dim=1)
    zeros = torch.zeros((n, 1), dtype=rot_vecs.dtype)
    K = torch.cat([zeros, -rz, ry, rz, zeros, -rx, -ry, rx, zeros], dim=1).view((n, 3, 3))
    return torch.eye(3, dtype=rot_vecs.dtype)[None] + sin * K + (1 - cos) * torch.bmm(K, K)


def batch_rigid_transform(rot_mats, joints, parents, dtype=torch.float32):
    joints = joints.unsqueeze(-1)
    rel = joints.clone()
    rel[:, 1:] -= joints[:, parents[1:]]
    local = torch.cat([F.pad(rot_mats.reshape(-1, 3, 3), [0, 0, 0, 1]), F.pad(rel.reshape(-1, 3, 1), [0, 0, 0, 1], value=1)],
                      dim=2).reshape(-1, joints.shape[1], 4, 4)
    chain = [local[:, 0]]
    for i in range(1, parents.shape[0]):
        chain.append(torch.matmul(chain[parents[i]], local[:, i]))
    transforms = torch.stack(chain, dim=1)
    posed = transforms[:, :, :3, 3]
    rel_transforms = transforms - F.pad(torch.matmul(transforms, F.pad(joints, [0, 0, 0, 1])), [3, 0, 0, 0, 0, 0, 0, 0])
    return posed, rel_transforms


def main():
    for name, fn in (("blend_shapes", blend_shapes), ("vertices2joints", vertices2joints), ("batch_rodrigues", batch_rodrigues),
                     ("batch_rigid_transform", batch_rigid_transform)):
        setattr(ref_smpl, name, fn)
    V, n_j, NB, B = 67, 24, 10, 3
    out = {}
    for pose2rot in (True, False):
        case = SR.make_case(V, B, NB, n_j, pose2rot, False, "smpl", seed=11)
        m = case["model"]
        tag = "aa" if pose2rot else "mat"
        if pose2rot:
            for k in SR.MODEL_KEYS:
                out["model/" + k] = m[k].numpy()
        out[f"{tag}/betas"], out[f"{tag}/pose"] = case["betas"].numpy(), case["pose"].numpy()
        # the reference evaluated in float64 on the float32 inputs: the fixture carries no rounding of its own
        res = ref_smpl.lbs(case["betas"].double(), case["pose"].double(), m["v_template"].double(), m["shapedirs"].double(),
                           m["posedirs"].double(), m["J_regressor"].double(), m["parents"].long(), m["lbs_weights"].double(),
                           pose2rot=pose2rot)
        for k, v in zip(SR.OUTPUTS, res):
            out[f"{tag}/{k}"] = v.numpy()
    path = os.path.join(HERE, "smpl_lbs_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
