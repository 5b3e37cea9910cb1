from .conditions import CameraPreprocessor, euler_xyz_to_matrix, preprocess_smpl_fix_body, smpl_conditions  # noqa: F401
from .datasets import SHHQDataset, densepose_faces_to_labels, load_smpl_model  # noqa: F401
from .ingest import ingest, ingest_torch  # noqa: F401
from .source import DatasetTrainingSource  # noqa: F401


def get_preprocessor(device, smpl_model, densepose_data=None, **meta):
    """The reference's get_preprocessor (lib/data/preprocessor.py:179-196) on a plain-array SMPL model: a CameraPreprocessor on
    `device` with init_smpl done.  smpl_model: a path to an .npz or a dict of arrays; the part labels are the model's
    faces_to_labels, or come from `densepose_data` (a densepose_data.json) when that is given."""
    import torch
    model = load_smpl_model(smpl_model)
    if densepose_data is not None:
        labels = densepose_faces_to_labels(densepose_data, model["faces"].shape[0])
    elif "faces_to_labels" in model:
        labels = model["faces_to_labels"]
    else:
        raise ValueError("the SMPL model has no faces_to_labels: give densepose_data (a densepose_data.json)")
    pre = CameraPreprocessor(device, **meta)
    pre.init_smpl(torch.as_tensor(model["faces"].astype("int64")), torch.as_tensor(labels.astype("int64")))
    return pre
