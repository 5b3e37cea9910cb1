"""Colours of rendered views carried onto the vertices of a mesh, on the device (csrc/mesh_attributes.hip; the definition -- camera,
weights, sampling conventions -- is in include/h3d.h, h3d_mesh_project_colors).

    project_colors(vertices, normals, images, depths, focals, scales, cam2world, depth_tolerance, normal_power=2, fill=0.0, eps=1e-3)
        -> (colors fp32 [V,3], coverage fp32 [V])

A view counts at a vertex by how squarely the vertex faces it, how far inside the image it projects and how well its distance from
the camera agrees with the view's depth map there (a tent of half-width `depth_tolerance`): all continuous, no threshold.  One
launch; the one host step is the float64 inversion of the K camera matrices into a [K,16] table.
"""
import numpy as np
import torch

from ... import _lib


def camera_table(focals, cam2world):
    """-> float32 numpy [K,16]: rows 0..2 of world2cam (cam2world inverted in float64), the camera origin, the focal."""
    c2w = cam2world.detach().double().cpu().numpy()
    w2c = np.linalg.inv(c2w)
    table = np.concatenate([w2c[:, :3, :].reshape(-1, 12), c2w[:, :3, 3], focals.detach().double().cpu().numpy().reshape(-1, 1)], axis=1)
    return table.astype(np.float32)


def check_views(who, named, depth_tolerance, normal_power, fill, eps):
    """The argument checks project_colors and mesh_texture.bake_texture share, before any device is asked for: `named` holds the
    tensors by name (vertices, normals, images, depths, focals, scales, cam2world and whatever else must be a tensor)
    -> (K, depth_tolerance, fill, eps) as python numbers"""
    for name, t in named.items():
        if not torch.is_tensor(t):
            raise TypeError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
    vertices, normals, images, depths = (named[k] for k in ("vertices", "normals", "images", "depths"))
    for name in ("vertices", "normals"):
        t = named[name]
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{who}: {name} must be float32 [V,3], got {t.dtype} {tuple(t.shape)}")
    if normals.shape[0] != vertices.shape[0]:
        raise ValueError(f"{who}: {normals.shape[0]} normals for {vertices.shape[0]} vertices")
    if images.dtype != torch.float32 or images.dim() != 4 or images.shape[1] != 3 or min(images.shape[2:]) < 2:
        raise ValueError(f"{who}: images must be float32 [K,3,H,W] with H, W >= 2, got {images.dtype} {tuple(images.shape)}")
    if depths.dtype != torch.float32 or depths.dim() != 3 or min(depths.shape[1:]) < 2:
        raise ValueError(f"{who}: depths must be float32 [K,h,w] with h, w >= 2, got {depths.dtype} {tuple(depths.shape)}")
    K = images.shape[0]
    if K < 1:
        raise ValueError(f"{who}: at least one view is needed (K >= 1)")
    for name, want in (("depths", (K,) + tuple(depths.shape[1:])), ("focals", (K,)), ("scales", (K,)), ("cam2world", (K, 4, 4))):
        if tuple(named[name].shape) != want:
            raise ValueError(f"{who}: {name} has shape {tuple(named[name].shape)}, the {K} views of images need {want}")
    depth_tolerance, fill, eps = float(depth_tolerance), float(fill), float(eps)
    if not 0.0 < depth_tolerance < float("inf"):
        raise ValueError(f"{who}: depth_tolerance={depth_tolerance} must be positive")
    if not 0.0 < eps < float("inf"):
        raise ValueError(f"{who}: eps={eps} must be positive")
    if int(normal_power) != normal_power or not 1 <= int(normal_power) <= 8:
        raise ValueError(f"{who}: normal_power={normal_power} must be an integer 1..8")
    return K, depth_tolerance, fill, eps


def project_colors(vertices, normals, images, depths, focals, scales, cam2world, depth_tolerance, normal_power=2, fill=0.0, eps=1e-3):
    """vertices, normals fp32 [V,3]; images fp32 [K,3,H,W] in [-1, 1]; depths fp32 [K,h,w], the renderer's ray distances in world
    units on its render grid; focals, scales [K] and cam2world [K,4,4] as the renderer took them.  `scales` only places the
    renderer's depth range along the ray (focal / scale), which `depths` already contains: it is checked and not read.
    -> (colors [V,3], coverage [V]): coverage = sum_k w_k, colors = (sum_k w_k c_k + eps fill) / (coverage + eps)."""
    named = dict(vertices=vertices, normals=normals, images=images, depths=depths, focals=focals, scales=scales, cam2world=cam2world)
    K, depth_tolerance, fill, eps = check_views("project_colors", named, depth_tolerance, normal_power, fill, eps)
    _lib.need_cuda(vertices, normals, images, depths)
    dev, V = vertices.device, vertices.shape[0]
    colors = torch.empty(V, 3, dtype=torch.float32, device=dev)
    coverage = torch.empty(V, dtype=torch.float32, device=dev)
    if V == 0:
        return colors, coverage
    table = torch.from_numpy(camera_table(focals, cam2world)).to(dev)
    vertices, normals, images, depths = (t.contiguous() for t in (vertices, normals, images, depths))
    (H, W), (h, w) = images.shape[2:], depths.shape[1:]
    _lib.check(_lib.load().h3d_mesh_project_colors(_lib.ptr(vertices), _lib.ptr(normals), V, _lib.ptr(images), K, H, W, _lib.ptr(depths),
                                                   h, w, _lib.ptr(table), depth_tolerance, int(normal_power), fill, eps,
                                                   _lib.ptr(colors), _lib.ptr(coverage), _lib.stream_handle()),
               "h3d_mesh_project_colors")
    return colors, coverage
