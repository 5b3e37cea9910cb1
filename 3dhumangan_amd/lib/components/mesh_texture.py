"""A texture atlas for a mesh, baked from rendered views on the device (csrc/mesh_attributes.hip; the layout and the per-texel
definition are in include/h3d.h, h3d_mesh_bake_texture).

    atlas_layout(T, size) -> (cell, per_row)
    atlas_uvs(T, size) -> float32 numpy [T,3,2]
    bake_texture(vertices, faces, normals, images, depths, focals, scales, cam2world, depth_tolerance, size, normal_power=2, fill=0.0,
                 eps=1e-3) -> (texture fp32 [S,S,3], coverage fp32 [S,S])
    texture_bytes(texture) -> uint8 numpy [S,S,3]

No unwrapping: every triangle owns half of a square cell of the texture, so the appearance has the resolution the texture is given,
whatever the mesh's.  A texel's colour is project_colors' colour (lib/components/mesh_color.py) at the point of the triangle the texel
stands for; a gutter of three diagonals between the two triangles of a cell keeps a viewer's bilinear filter inside one triangle.
"""
import math

import numpy as np
import torch

from ... import _lib
from .mesh_color import camera_table, check_views
from .mesh_io import color_bytes

MAX_SIZE = 8192


def atlas_layout(T, size):
    """-> (cell, per_row): the cell edge c = size // R in texels and the cells per row R = ceil(sqrt(ceil(T / 2))), in integers.
    ValueError where size is outside 2..8192 or a cell would have fewer than 4 texels a side (it names the size that works)."""
    T, size = int(T), int(size)
    if T < 0:
        raise ValueError(f"atlas_layout: T={T} triangles")
    if not 2 <= size <= MAX_SIZE:
        raise ValueError(f"atlas_layout: size={size} outside 2..{MAX_SIZE}")
    cells = (T + 1) // 2
    per_row = math.isqrt(cells - 1) + 1 if cells > 0 else 1
    cell = size // per_row
    if cell < 4:
        raise ValueError(f"atlas_layout: {T} triangles need {per_row} x {per_row} cells of at least 4 texels: the smallest size is "
                         f"{4 * per_row}, got {size}")
    return cell, per_row


def atlas_uvs(T, size):
    """-> float32 [T,3,2]: (u, v) of every triangle's corners, v = 0 at the top row of the texture"""
    c, R = atlas_layout(T, size)
    t = np.arange(int(T), dtype=np.int64)
    cell = t // 2
    x0, y0 = ((cell % R) * c).astype(np.float64)[:, None], ((cell // R) * c).astype(np.float64)[:, None]
    m = c - 3
    lower = np.stack([x0 + [0.5, m + 0.5, 0.5], y0 + [0.5, 0.5, m + 0.5]], axis=-1)
    upper = np.stack([x0 + [c - 0.5, 2.5, c - 0.5], y0 + [c - 0.5, c - 0.5, 2.5]], axis=-1)
    return (np.where((t % 2 == 1)[:, None, None], upper, lower) / int(size)).astype(np.float32)


def bake_texture(vertices, faces, normals, images, depths, focals, scales, cam2world, depth_tolerance, size, normal_power=2, fill=0.0,
                 eps=1e-3):
    """vertices, normals fp32 [V,3]; faces int32 [T,3]; the views and constants as project_colors takes them; size: the texture's
    edge S.  -> (texture [S,S,3] in the images' [-1, 1], coverage [S,S]); a texel no triangle owns has colour `fill` and coverage 0.
    Face indices outside [0, V) are clamped on the device: a wrong texel, never a load out of range."""
    named = dict(vertices=vertices, faces=faces, normals=normals, images=images, depths=depths, focals=focals, scales=scales,
                 cam2world=cam2world)
    K, depth_tolerance, fill, eps = check_views("bake_texture", named, depth_tolerance, normal_power, fill, eps)
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"bake_texture: faces must be int32 [T,3], got {faces.dtype} {tuple(faces.shape)}")
    V, T = vertices.shape[0], faces.shape[0]
    if T > 0 and V == 0:
        raise ValueError(f"bake_texture: {T} triangles without a vertex")
    if int(size) != size:
        raise ValueError(f"bake_texture: size={size} must be an integer")
    S = int(size)
    atlas_layout(T, S)
    _lib.need_cuda(vertices, faces, normals, images, depths)
    dev = vertices.device
    texture = torch.empty(S, S, 3, dtype=torch.float32, device=dev)
    coverage = torch.empty(S, S, dtype=torch.float32, device=dev)
    table = torch.from_numpy(camera_table(focals, cam2world)).to(dev)
    vertices, faces, normals, images, depths = (t.contiguous() for t in (vertices, faces, normals, images, depths))
    (H, W), (h, w) = images.shape[2:], depths.shape[1:]
    _lib.check(_lib.load().h3d_mesh_bake_texture(_lib.ptr(vertices), _lib.ptr(normals), V, _lib.ptr(faces), T, S, _lib.ptr(images), K, H,
                                                 W, _lib.ptr(depths), h, w, _lib.ptr(table), depth_tolerance, int(normal_power), fill,
                                                 eps, _lib.ptr(texture), _lib.ptr(coverage), _lib.stream_handle()),
               "h3d_mesh_bake_texture")
    return texture, coverage


def texture_bytes(texture):
    """texture [S,S,3] in [-1, 1] (tensor or array) -> uint8 numpy [S,S,3], converted as write_ply converts colours: *0.5+0.5, *255,
    clamp, truncate; NaN gives 0"""
    t = np.asarray(texture.detach().cpu().numpy() if hasattr(texture, "detach") else texture)
    if t.ndim != 3 or t.shape[2] != 3:
        raise ValueError(f"texture_bytes: texture must be [S,S,3], got {t.shape}")
    return color_bytes(t)
