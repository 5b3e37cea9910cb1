"""The SHHQ dataset reader (reference: SHHQDataset, lib/data/datasets.py:27-320), without torchvision, cv2, scipy or pickled
models: the images are decoded with PIL, the item transform is lib/data/ingest.py, the SMPL model is a plain-array .npz.

Layout under `dataroot` (item i is file NNNNNN = i + 1, six digits):
    images/NNNNNN.png     RGB photograph                       masks/NNNNNN.png    foreground mask (read as "L")
    body_seg/NNNNNN.png   part labels in channel 0             inversions/NNNNNN.npy   optional latent [>= latent_dim]
    smpl/NNNNNN.npz       the SMPL regression record as plain arrays (tried first), or smpl/NNNNNN.pkl, the reference's joblib
                          record: orig_cam [1,4], joints [1,Jall,3], full_pose [1,24,3,3], fk_matrices [1,24,4,4],
                          tpose_vertices [1,V,3], lbs_weights [V,24] (, betas [1,10])

raw(i) is what the host does per item (decode, copy bytes); __getitem__(i) is the reference's item, built from ingest_torch and
conditions.preprocess_smpl_fix_body on the CPU.  lib/data/source.DatasetTrainingSource feeds raw() items to the fused GPU ingest.
"""
import json
import os

import numpy as np
import torch

from . import conditions
from .ingest import ingest_torch

RECORD_KEYS = ("orig_cam", "joints", "full_pose", "fk_matrices", "tpose_vertices")
MODEL_KEYS = ("v_template", "lbs_weights", "faces")


def load_smpl_model(smpl_model):
    """a path to an .npz or a dict of arrays with the keys of synthetic.make_smpl_model -> dict of numpy arrays"""
    if smpl_model is None:
        raise ValueError("SHHQDataset needs smpl_model=: a path to an .npz or a dict of arrays (synthetic.make_smpl_model's keys)")
    if isinstance(smpl_model, (str, os.PathLike)):
        if not os.path.exists(smpl_model):
            raise FileNotFoundError(f"SMPL model not found: {smpl_model}")
        smpl_model = dict(np.load(smpl_model))
    model = {k: np.asarray(v) for k, v in smpl_model.items()}
    missing = [k for k in MODEL_KEYS if k not in model]
    if missing:
        raise ValueError(f"smpl_model lacks {missing} (has {sorted(model)})")
    return model


def densepose_faces_to_labels(path, n_faces):
    """reference get_preprocessor (lib/data/preprocessor.py:187-192): densepose_faces_to_labels[smpl_faces_to_densepose_faces[f]]"""
    if not os.path.exists(path):
        raise FileNotFoundError(f"densepose data not found: {path}")
    data = json.load(open(path))
    to_dp = np.asarray(data["smpl_faces_to_densepose_faces"], dtype=np.int64)[np.arange(n_faces)]
    return np.asarray(data["densepose_faces_to_labels"], dtype=np.int64)[to_dp]


def _open(path):
    if not os.path.exists(path):
        raise FileNotFoundError(f"dataset file not found: {path}")
    from PIL import Image
    return Image.open(path)


class SHHQDataset(torch.utils.data.Dataset):
    """SHHQDataset(dataroot=, dataset_length=, gen_height=, gen_width=, latent_dim=, joints=[], coordinate_mode="fix_body",
    inference=False, image_only=False, geo_only=False, condition_only=False, smpl_model=, densepose_data=None); vertex_downsample
    is accepted and ignored."""

    corrupted = [118464]

    def __init__(self, **kwargs):
        super().__init__()
        self.coordinate_mode = kwargs.get("coordinate_mode", "fix_body")
        if self.coordinate_mode != "fix_body":
            raise NotImplementedError("only coordinate_mode='fix_body' (every shipped config) is provided")
        self.root = kwargs["dataroot"]
        self.length = int(kwargs["dataset_length"])
        self.height, self.width = int(kwargs["gen_height"]), int(kwargs["gen_width"])
        self.joints = list(kwargs.get("joints", []))
        self.latent_dim = int(kwargs["latent_dim"])
        self.inference = bool(kwargs.get("inference", False))
        self.image_only = bool(kwargs.get("image_only", False))
        self.geo_only = bool(kwargs.get("geo_only", False))
        self.condition_only = bool(kwargs.get("condition_only", False))
        model = load_smpl_model(kwargs.get("smpl_model"))
        self.template = torch.as_tensor(model["v_template"]).float()
        self.lbs_weights = torch.as_tensor(model["lbs_weights"]).float()
        self.faces = torch.as_tensor(model["faces"].astype(np.int64))
        if kwargs.get("densepose_data") is not None:
            labels = densepose_faces_to_labels(kwargs["densepose_data"], self.faces.shape[0])
        elif "faces_to_labels" in model:
            labels = model["faces_to_labels"]
        else:
            raise ValueError("the SMPL model has no faces_to_labels: give densepose_data= (a densepose_data.json)")
        self.faces_to_labels = torch.as_tensor(np.asarray(labels).astype(np.int64))
        if not self.joints and "joints_index" in model:
            self.joints = [int(j) for j in model["joints_index"]]

    def __len__(self):
        return self.length

    def resolve(self, index):
        """the reference's skip of the corrupted items (:276-277)"""
        index = int(index)
        while index in self.corrupted:
            index = (index + 1) % len(self)
        return index

    def path(self, kind, index, ext):
        return os.path.join(self.root, kind, f"{index + 1:06d}.{ext}")

    def record(self, index):
        """the SMPL regression record of item `index` as numpy arrays; smpl/NNNNNN.npz first, then the joblib .pkl"""
        npz, pkl = self.path("smpl", index, "npz"), self.path("smpl", index, "pkl")
        if os.path.exists(npz):
            rec = dict(np.load(npz))
        elif os.path.exists(pkl):
            import joblib
            rec = joblib.load(pkl)
        else:
            raise FileNotFoundError(f"dataset file not found: {npz} (nor {pkl})")
        if "lbs_weights" in rec:
            w = np.asarray(rec["lbs_weights"])
            if w.shape != tuple(self.lbs_weights.shape) or not np.array_equal(w.astype(np.float32), self.lbs_weights.numpy()):
                raise ValueError(f"the record of item {index} carries lbs_weights that differ from the SMPL model's")
        keys = RECORD_KEYS + (("betas",) if self.inference else ())
        missing = [k for k in keys if k not in rec]
        if missing:
            raise ValueError(f"the record of item {index} lacks {missing}")
        return {k: np.asarray(rec[k]) for k in keys}

    def raw(self, index):
        """-> numpy: rgb [Hs,Ws,3], mask [Hs,Ws], seg [Hs,Ws] uint8, index, latent [latent_dim] fp32 when the dataset has
        inversions, and the record's small arrays.  Decoding and byte copies only."""
        index = self.resolve(index)
        out = {"index": index}
        out["rgb"] = np.ascontiguousarray(np.asarray(_open(self.path("images", index, "png")).convert("RGB"), dtype=np.uint8))
        out["mask"] = np.ascontiguousarray(np.asarray(_open(self.path("masks", index, "png")).convert("L"), dtype=np.uint8))
        seg = np.asarray(_open(self.path("body_seg", index, "png")), dtype=np.uint8)
        out["seg"] = np.ascontiguousarray(seg[:, :, 0] if seg.ndim == 3 else seg)
        if out["mask"].shape != out["rgb"].shape[:2] or out["seg"].shape != out["rgb"].shape[:2]:
            raise ValueError(f"item {index}: image {out['rgb'].shape[:2]}, mask {out['mask'].shape} and labels {out['seg'].shape} differ")
        latent = self.path("inversions", index, "npy")
        if os.path.exists(latent):
            out["latent"] = (2 * np.load(latent)[:self.latent_dim]).astype(np.float32)
        out.update(self.record(index))
        return out

    def _conditions(self, rec):
        pred = dict(rec, lbs_weights=self.lbs_weights.numpy())
        return conditions.preprocess_smpl_fix_body(pred, self.joints, self.template, inference=self.inference)

    def _images(self, index, with_segments):
        rgb = np.array(_open(self.path("images", index, "png")).convert("RGB"), dtype=np.uint8)
        mask = np.array(_open(self.path("masks", index, "png")).convert("L"), dtype=np.uint8)
        if with_segments:
            seg = np.array(_open(self.path("body_seg", index, "png")), dtype=np.uint8)
            seg = seg[:, :, 0] if seg.ndim == 3 else seg
        else:
            seg = np.zeros_like(mask)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))[None]                      # noqa: E731
        out = ingest_torch(t(rgb), t(mask), t(seg), (self.height, self.width), self.geo_only)
        return {k: v[0] for k, v in out.items()}

    def __getitem__(self, index):
        index = self.resolve(index)
        if self.image_only:
            im = self._images(index, False)
            return {"images": im["images"], "masks": im["masks"]}
        if self.condition_only:
            return self._conditions(self.record(index))
        data = {"indices": index}
        latent = self.path("inversions", index, "npy")
        if os.path.exists(latent):                                                 # the reference requires them; optional here
            data["latents"] = torch.from_numpy((2 * np.load(latent)[:self.latent_dim]).astype(np.float32))
        data.update(self._images(index, True))
        if len(self.joints) > 0:
            data.update(self._conditions(self.record(index)))
        return data
