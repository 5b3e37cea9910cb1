"""The condition front-end of the generator, in plain torch -- no pytorch3d / smplx / dataset files:

  preprocess_smpl_fix_body   one SMPL prediction record -> the `conditions` entries the generator consumes
                             (reference: SHHQDataset._preprocess_smpl_fix_body, lib/data/datasets.py:117-181)
  CameraPreprocessor         the camera matrices for a requested view (reference: SHHQPreprocessor.forward /
                             forward_with_rotation / _forward_fix_body, lib/data/preprocessor.py:45-97)

Both are pinned to the reference's own methods by tests/golden/frontend.npz.  The preprocessor's mesh rasteriser (:138-176,
pytorch3d in the reference) runs on the HIP kernel of lib/components/raster.py once `init_smpl` has handed it the SMPL faces and
their part labels: forward_with_rotation then returns `rasterized_segments` (the segmentation target of the trainer) and the real
`rasterized_semantics`; without `init_smpl` the semantics are an all-zero map and there are no segments.  Third-party boundary: pytorch3d.transforms.euler_angles_to_matrix
(pinned 0.6.2, not installed): euler_xyz_to_matrix follows its published definition, Rx(a) @ Ry(b) @ Rz(c) for "XYZ".
"""
import math

import torch

from ..components import raster
from ..components import smpl as smpl_ops

FOV = math.pi * 12 / 180
FOCAL = 1.0 / math.tan(FOV / 2)                      # 9.5144: intrinsics[0,0] of every sample
FOCAL_RASTER = 1.0 / math.tan(math.pi / 360)         # 114.59: the rasteriser's 1-degree camera (preprocessor.py:145-146)


def euler_xyz_to_matrix(euler):
    """euler [B,3] (radians) -> [B,3,3] = Rx(e0) @ Ry(e1) @ Rz(e2)."""
    a, b, c = euler[:, 0], euler[:, 1], euler[:, 2]
    one, zero = torch.ones_like(a), torch.zeros_like(a)
    rx = torch.stack([one, zero, zero, zero, a.cos(), -a.sin(), zero, a.sin(), a.cos()], -1).view(-1, 3, 3)
    ry = torch.stack([b.cos(), zero, b.sin(), zero, one, zero, -b.sin(), zero, b.cos()], -1).view(-1, 3, 3)
    rz = torch.stack([c.cos(), -c.sin(), zero, c.sin(), c.cos(), zero, zero, zero, one], -1).view(-1, 3, 3)
    return rx @ ry @ rz


def preprocess_smpl_fix_body(pred, joints_index, smpl_tpose_vertices, inference=False):
    """pred: one SMPL regression record (arrays with a leading batch dim of 1, as the dataset stores them): orig_cam [1,4]
    (sx, sy, tx, ty), joints [1,Jall,3], full_pose [1,24,3,3], tpose_vertices [1,V,3], fk_matrices [1,24,4,4], lbs_weights
    [V,24] (, betas [1,10]).  -> dict of float32 tensors: scales, skeletons_xyz [24,3], intrinsics [4,4], vertices [V,3],
    tpose_vertices [V,3] (the TEMPLATE mesh raised by 0.35 in y), full_pose, fk_matrices, lbs_weights, cano_matrices, R, T.

    "fix body": the body is put into a canonical frame -- root rotation undone, then turned upside-up by Rx(pi) -- and the
    camera carries the view."""
    f64 = lambda x: torch.as_tensor(x, dtype=torch.float64)
    sx, _, tx, ty = [float(v) for v in torch.as_tensor(pred["orig_cam"]).reshape(-1)[:4].float()]     # stored as float32
    sx = sx / 2.0
    skeleton = f64(pred["joints"])[0].float().double()[list(joints_index)]
    K = torch.diag(torch.tensor([FOCAL, FOCAL, 1.0, 1.0], dtype=torch.float64))
    T = torch.eye(4, dtype=torch.float64)
    T[0, 3], T[1, 3], T[2, 3] = tx, ty, FOCAL / sx
    pose = f64(pred["full_pose"])[0]
    cano = torch.eye(4, dtype=torch.float64)
    rx_pi = torch.tensor([[1.0, 0, 0], [0, math.cos(math.pi), -math.sin(math.pi)], [0, math.sin(math.pi), math.cos(math.pi)]],
                         dtype=torch.float64)
    cano[:3, :3] = rx_pi @ torch.linalg.inv(pose[0])
    fk = torch.einsum("ij,bjk->bik", cano, f64(pred["fk_matrices"])[0])
    lbs = f64(pred["lbs_weights"])
    per_vertex = torch.einsum("bi,ijk->bjk", lbs, fk)
    tpose_shaped = f64(pred["tpose_vertices"])[0]
    homo = torch.cat([tpose_shaped, torch.ones_like(tpose_shaped[:, :1])], dim=1)
    vertices = torch.einsum("bij,bj->bi", per_vertex, homo)[:, :3]
    sk_h = torch.cat([skeleton, torch.ones_like(skeleton[:, :1])], dim=1)
    skeleton = torch.einsum("ij,bj->bi", cano, sk_h)[:, :3]
    template = torch.as_tensor(smpl_tpose_vertices).float().clone()
    template[..., 1] += 0.35
    out = {"scales": torch.tensor(sx, dtype=torch.float32), "skeletons_xyz": skeleton.float(), "intrinsics": K.float(),
           "vertices": vertices.float(), "tpose_vertices": template, "full_pose": pose.float(), "fk_matrices": fk.float(),
           "lbs_weights": lbs.float(), "cano_matrices": cano.float(), "R": torch.eye(4), "T": T.float()}
    if inference:
        out["body_shape"] = f64(pred["betas"])[0].float()
    return out


def smpl_conditions_math(fk_matrices, joints, full_pose, orig_cam, joints_index):
    """The small matrices of preprocess_smpl_fix_body for a batch, in float64 on the inputs' device (plain torch, CPU or GPU):
    fk_matrices [B,J,4,4], joints [B,Jall,3], full_pose [B,J,3,3], orig_cam [B,4] -> dict of float64 tensors scales [B],
    intrinsics, T, cano_matrices [B,4,4], fk_matrices [B,J,4,4] (= cano . A), skeletons_xyz [B,len(joints_index),3]."""
    dev = fk_matrices.device
    B = fk_matrices.shape[0]
    cam = orig_cam.reshape(B, -1)[:, :4].float().double()                                  # stored as float32
    sx = cam[:, 0] / 2.0
    K = torch.diag(torch.tensor([FOCAL, FOCAL, 1.0, 1.0], dtype=torch.float64, device=dev)).expand(B, 4, 4).clone()
    T = torch.eye(4, dtype=torch.float64, device=dev).repeat(B, 1, 1)
    T[:, 0, 3], T[:, 1, 3], T[:, 2, 3] = cam[:, 2], cam[:, 3], FOCAL / sx
    rx_pi = torch.tensor([[1.0, 0, 0], [0, math.cos(math.pi), -math.sin(math.pi)], [0, math.sin(math.pi), math.cos(math.pi)]],
                         dtype=torch.float64, device=dev)
    cano = torch.eye(4, dtype=torch.float64, device=dev).repeat(B, 1, 1)
    cano[:, :3, :3] = rx_pi @ torch.linalg.inv(full_pose[:, 0].double())                    # a true inverse, as the dataset code takes
    fk = cano[:, None] @ fk_matrices.double()
    sk = joints.float().double()[:, list(joints_index)]
    sk = sk @ cano[:, :3, :3].transpose(1, 2) + cano[:, None, :3, 3]
    return {"scales": sx, "intrinsics": K, "T": T, "cano_matrices": cano, "fk_matrices": fk, "skeletons_xyz": sk}


@torch.no_grad()
def smpl_conditions(smpl_out, orig_cam, joints_index, smpl_tpose_vertices):
    """The batched, on-device counterpart of preprocess_smpl_fix_body: `smpl_out` is the dict of components.smpl.SMPL.forward
    for B bodies (device tensors), orig_cam [B,4] (sx, sy, tx, ty), smpl_tpose_vertices [V,3] the model's template.  -> what
    preprocess_smpl_fix_body returns per record, stacked over the batch (float32, on the device): scales [B], skeletons_xyz,
    intrinsics, vertices, tpose_vertices, full_pose [B,J,3,3], fk_matrices, lbs_weights [B,V,J], cano_matrices, R, T.

    The root rotation comes from smpl_out["full_pose"] when that holds matrices, else from global_orient / body_pose (axis-angle
    goes through batch_rodrigues).  The vertices are the shaped template skinned with cano . A by the HIP skinning kernel -- no
    pose offsets, as the dataset code applies none; the small matrices are float64 torch ops on the device."""
    A = smpl_out["fk_matrices"]
    B, J = A.shape[:2]
    dev = A.device
    pose = smpl_out.get("full_pose")
    if pose is None or pose.shape[-2:] != (3, 3) or pose.dim() != 4:
        go, bp = smpl_out["global_orient"], smpl_out["body_pose"]
        if go.shape[-2:] == (3, 3) and go.dim() >= 3:
            pose = torch.cat([go.reshape(B, -1, 3, 3), bp.reshape(B, -1, 3, 3)], dim=1)
        else:
            aa = torch.cat([go.reshape(B, -1), bp.reshape(B, -1)], dim=1).reshape(-1, 3)
            pose = smpl_ops.batch_rodrigues(aa.float()).view(B, J, 3, 3)
    pose = pose.to(dev)
    m = smpl_conditions_math(A, smpl_out["joints"], pose, torch.as_tensor(orig_cam).to(dev), joints_index)
    vertices = smpl_ops.skin_vertices(smpl_out["tpose_vertices"], A, smpl_out["lbs_weights"], rigid=m["cano_matrices"].float())
    template = torch.as_tensor(smpl_tpose_vertices).float().to(dev).clone()
    template[..., 1] += 0.35
    return {"scales": m["scales"].float(), "skeletons_xyz": m["skeletons_xyz"].float(), "intrinsics": m["intrinsics"].float(),
            "vertices": vertices, "tpose_vertices": template[None].repeat(B, 1, 1), "full_pose": pose.float(),
            "fk_matrices": m["fk_matrices"].float(), "lbs_weights": smpl_out["lbs_weights"].float()[None].repeat(B, 1, 1),
            "cano_matrices": m["cano_matrices"].float(), "R": torch.eye(4, device=dev).repeat(B, 1, 1), "T": m["T"].float()}


def raster_translation(data):
    """T of the rasteriser's camera, [B,3] (preprocessor.py:147-148): the record's x/y offsets, depth f_r / (2 scales).  With
    R = data["raster_rotation"] and focal -f_r the mesh lands where the generator's camera sees it (the 0.5 assumes H = 2 W, the
    shape of every shipped config)."""
    T_raster = data["T"][:, :3, -1].clone()
    T_raster[:, -1] = FOCAL_RASTER / data["scales"].reshape(-1) * 0.5
    return T_raster


class CameraPreprocessor:
    """coordinate_mode "fix_body": world2cam = R @ T @ [root_rotation @ Rx(pi - v) Ry(-h) Rz(-r)], cam2world its inverse.
    Same call surface as the reference's SHHQPreprocessor (forward / forward_with_rotation / to)."""

    def __init__(self, device="cpu", **kwargs):
        self.device = device
        if kwargs.get("coordinate_mode", "fix_body") != "fix_body":
            raise NotImplementedError("only coordinate_mode='fix_body' (every shipped config) is provided")
        self.smpl_faces = None
        self.smpl_faces_to_labels = None

    @torch.no_grad()
    def init_smpl(self, smpl_faces, smpl_faces_to_labels):
        """The SMPL topology [F,3] and the per-face part labels [F] (preprocessor.py:38-42); enables the rasteriser."""
        self.smpl_faces = torch.as_tensor(smpl_faces).long().clone()
        self.smpl_faces_to_labels = torch.as_tensor(smpl_faces_to_labels).long().clone()
        if self.smpl_faces.dim() != 2 or self.smpl_faces.shape[1] != 3 or self.smpl_faces_to_labels.shape != self.smpl_faces.shape[:1]:
            raise ValueError(f"init_smpl: faces [F,3] and labels [F] expected, got {tuple(self.smpl_faces.shape)}, "
                             f"{tuple(self.smpl_faces_to_labels.shape)}")

    def to(self, device):
        self.device = device
        return self

    @torch.no_grad()
    def forward(self, data, rotate=False, **kwargs):
        """Random view: h, v ~ N(mean, stddev) when `rotate`, else the means (preprocessor.py:45-55; draws on the CPU RNG
        like the reference)."""
        B = data["scales"].shape[0]
        h = torch.randn(B) * (kwargs["h_stddev"] if rotate else 0) + kwargs["h_mean"]
        v = torch.randn(B) * (kwargs["v_stddev"] if rotate else 0) + kwargs["v_mean"]
        return self.forward_with_rotation(data, h, v, torch.zeros_like(h), **kwargs)

    __call__ = forward

    @torch.no_grad()
    def forward_with_rotation(self, data, h_rotation, v_rotation, r_rotation, **kwargs):
        data = dict(data)
        B = data["scales"].shape[0]
        dev = data["scales"].device
        euler = torch.zeros([B, 3], device=dev)
        euler[:, 1] = -h_rotation.reshape(B).to(dev)
        euler[:, 0] = math.pi - v_rotation.reshape(B).to(dev)
        euler[:, 2] = -r_rotation.reshape(B).to(dev)
        R = data["full_pose"][:, 0] @ euler_xyz_to_matrix(euler)
        body = torch.zeros(B, 4, 4, device=dev)
        body[:, :3, :3] = R
        body[:, 3, 3] = 1.0
        world2cam = torch.bmm(torch.bmm(data["R"], data["T"]), body)
        data["cam2world_matrices"] = torch.inverse(world2cam.float())
        data["raster_rotation"] = torch.inverse(R)                  # R_raster of the reference (feeds its rasteriser)
        h, w = kwargs.get("gen_height", 1), kwargs.get("gen_width", 1)
        if self.smpl_faces is None:
            data["rasterized_semantics"] = torch.zeros(B, 3, h, w, device=dev)
            return data
        return self._forward_rasterize(data, data["raster_rotation"], h, w)

    def _forward_rasterize(self, data, R_raster, h, w):
        """preprocessor.py:138-176: the posed SMPL mesh at the sampled view, a 1-degree camera at distance f_r / (2 scales)."""
        dev = data["scales"].device
        T_raster = raster_translation(data)
        faces, labels = self.smpl_faces.to(dev), self.smpl_faces_to_labels.to(dev)
        seg, sem = raster.rasterize_segments_semantics(data["vertices"], faces, R_raster, T_raster, -FOCAL_RASTER, (h, w), labels,
                                                       data["tpose_vertices"][0])
        data["rasterized_semantics"] = sem
        data["rasterized_segments"] = seg
        return data
