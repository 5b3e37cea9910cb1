"""Mesh rasterisation on the HIP kernel of csrc/mesh_raster.hip (h3d_mesh_rasterize): the SMPL mesh at a camera, in place of the
pytorch3d 0.6.2 MeshRasterizer the reference's preprocessor uses (lib/data/preprocessor.py:138-176; faces_per_pixel=1,
blur_radius=0, PerspectiveCameras(in_ndc=True), perspective-corrected barycentrics).  Forward only, no gradients.

Conventions (include/h3d.h): view X = v @ R + T with row vectors; NDC x = focal * X / Z, y = focal * Y / Z; pixel (r, c) at
(W/s - (2c+1)/s, H/s - (2r+1)/s), s = min(H, W) (+x left, +y up).  Rules at the boundary, as pytorch3d 0.6.2's rasterize_meshes
reads: a face is skipped when its NDC area is <= 1e-8 in magnitude or a vertex has Z <= 0 (pytorch3d clips per pixel; a body in
front of the camera never meets that case); a pixel is covered when all three perspective-corrected barycentrics are > 0, in either
winding; the smallest depth wins and exact ties go to the lower face index.  These rules only decide pixels within float rounding
of an edge or of a depth tie.
"""
import collections

import torch

from ... import _lib

Fragments = collections.namedtuple("Fragments", ["pix_to_face", "zbuf", "bary_coords"])


def _launch(vertices, faces, R, T, focal, image_size, face_labels=None, sem_table=None, want_fragments=True):
    _lib.need_cuda(vertices, faces, R, T, face_labels, sem_table)
    H, W = (int(image_size), int(image_size)) if isinstance(image_size, int) else (int(image_size[0]), int(image_size[1]))
    if vertices.dim() != 3 or vertices.shape[2] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"rasterize: vertices [B,V,3] and faces [F,3] expected, got {tuple(vertices.shape)}, {tuple(faces.shape)}")
    B, V, F = vertices.shape[0], vertices.shape[1], faces.shape[0]
    if R.shape != (B, 3, 3) or T.shape != (B, 3):
        raise ValueError(f"rasterize: R [B,3,3] and T [B,3] expected, got {tuple(R.shape)}, {tuple(T.shape)}")
    dev = vertices.device
    vertices = vertices.detach().float().contiguous()
    faces = faces.detach().to(torch.int32).contiguous()
    R = R.detach().float().contiguous()
    T = T.detach().float().contiguous()
    if face_labels is not None:
        face_labels = face_labels.detach().to(torch.int32).contiguous()
        if face_labels.shape != (F,):
            raise ValueError(f"rasterize: face_labels [F] expected, got {tuple(face_labels.shape)}")
    if sem_table is not None:
        sem_table = sem_table.detach().float().contiguous()
        if sem_table.shape != (V, 3):
            raise ValueError(f"rasterize: sem_table [V,3] expected, got {tuple(sem_table.shape)}")
    lib = _lib.load()
    ws = torch.empty(int(lib.h3d_mesh_raster_bytes(B, F)), dtype=torch.uint8, device=dev)
    pix = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    zbuf = torch.empty(B, H, W, device=dev) if want_fragments else None
    bary = torch.empty(B, H, W, 3, device=dev) if want_fragments else None
    seg = torch.empty(B, H, W, dtype=torch.int64, device=dev) if face_labels is not None else None
    sem = torch.empty(B, 3, H, W, device=dev) if sem_table is not None else None
    rc = lib.h3d_mesh_rasterize(_lib.ptr(vertices), _lib.ptr(faces), _lib.ptr(R), _lib.ptr(T), float(focal), _lib.ptr(face_labels),
                                _lib.ptr(sem_table), _lib.ptr(pix), _lib.ptr(zbuf), _lib.ptr(bary), _lib.ptr(seg), _lib.ptr(sem),
                                _lib.ptr(ws), B, V, F, H, W, _lib.stream_handle())
    _lib.check(rc, "h3d_mesh_rasterize")
    return pix, zbuf, bary, seg, sem


@torch.no_grad()
def rasterize_meshes(vertices, faces, R, T, focal, image_size):
    """vertices [B,V,3], faces [F,3] (shared by the batch), R [B,3,3], T [B,3], focal: the camera's focal_length (a float; the
    reference passes -1/tan(pi/360)), image_size: (H, W) or an int.  -> Fragments of pytorch3d's shapes for faces_per_pixel=1:
    pix_to_face int64 [B,H,W,1] (the per-image face index -- what the reference gets after its `% F` -- or -1), zbuf [B,H,W,1]
    (-1 on background), bary_coords [B,H,W,1,3] (-1 on background)."""
    pix, zbuf, bary, _, _ = _launch(vertices, faces, R, T, focal, image_size)
    return Fragments(pix.long().unsqueeze(-1), zbuf.unsqueeze(-1), bary.unsqueeze(-2))


@torch.no_grad()
def rasterize_segments_semantics(vertices, faces, R, T, focal, image_size, face_labels, sem_table):
    """The reference's two derived maps (preprocessor.py:156-174) from one launch: segments int64 [B,H,W] = face_labels[f] + 2
    (1 on background), semantics [B,3,H,W] = sem_table[faces[f][argmax bary]] (0 on background)."""
    _, _, _, seg, sem = _launch(vertices, faces, R, T, focal, image_size, face_labels, sem_table, want_fragments=False)
    return seg, sem
