"""The geometry export as stages: settings -> density_grid -> surfaces -> view_frame per view -> colour -> rig.
Map3DGenerator.extract_mesh / extract_textured_mesh / extract_avatar and apps/sample_from_generator.py run the same functions; a
generator, where a stage needs one, is an argument.  No stage enters a device context: the caller holds that block."""
import math
from collections import namedtuple

import torch

from ..components import mesh_rig
from ..components.isosurface import marching_tetrahedra, vertex_normals
from ..components.mesh_color import project_colors
from ..components.mesh_simplify import simplify as simplify_mesh
from ..components.mesh_texture import atlas_uvs, bake_texture


Settings = namedtuple("Settings", "level depth_tolerance normal_power simplify texture_size")      # simplify, texture_size: or None


def default_depth_tolerance(config):
    """two coarse integration steps of the render, in world units"""
    return 2.0 * (config["ray_end"] - config["ray_start"]) / config.get("num_steps", 24)


def settings(who, config, n_views=0, level=None, depth_tolerance=None, normal_power=2, texture_size=None, simplify=None):
    """The arguments of the public method `who` (Map3DGenerator.extract_* document them) checked and their defaults resolved,
    before a generator or a device is touched -> Settings"""
    if config.get("clamp_mode", "relu") != "relu":
        raise NotImplementedError(f"{who}: clamp_mode={config['clamp_mode']!r} is not supported: only with 'relu' is the raw output "
                                  "of the density head the density the renderer integrates (above zero)")
    if int(normal_power) != normal_power or not 1 <= int(normal_power) <= 8:
        raise ValueError(f"{who}: normal_power={normal_power} must be an integer 1..8")
    if texture_size is not None and not n_views:
        raise ValueError(f"{who}: texture_size needs at least one view to bake the texture from")
    level = math.log(2.0) * config.get("num_steps", 24) / (config["ray_end"] - config["ray_start"]) if level is None else level
    depth_tolerance = default_depth_tolerance(config) if depth_tolerance is None else depth_tolerance
    if not 0.0 < float(depth_tolerance) < math.inf:
        raise ValueError(f"{who}: depth_tolerance={depth_tolerance} must be positive")
    if simplify is not None and (isinstance(simplify, bool) or not isinstance(simplify, (int, float)) or not 0.0 < simplify < math.inf):
        raise ValueError(f"{who}: simplify={simplify!r} must be a positive number (the cluster cell in voxels) or None")
    return Settings(level, float(depth_tolerance), int(normal_power), None if simplify is None else float(simplify), texture_size)


def surfaces(sigma, origin, spacing, level, simplify, normals):
    """density_grid's (sigma [B,Nx,Ny,Nz], origin, spacing) -> one dict(vertices, faces, normals, colors=None, coverage=None) per
    item: marching_tetrahedra at `level`; simplify=K clusters it on cells of K (cubic) voxels over the grid's own box, counts
    floor((N - 1) / K) + 1 per axis; `normals`: vertex_normals of the same grid at the final vertices, else None and no launch."""
    meshes = []
    for b, (o, s) in enumerate(zip(origin.tolist(), spacing.tolist())):
        vertices, faces = marching_tetrahedra(sigma[b], level, o, s)
        if simplify is not None:
            counts = [int(math.floor((n - 1) / simplify)) + 1 for n in sigma.shape[1:]]
            vertices, faces = simplify_mesh(vertices, faces, simplify * s[0], origin=o, counts=counts)[:2]
        meshes.append(dict(vertices=vertices, faces=faces, normals=vertex_normals(sigma[b], vertices, o, s) if normals else None,
                           colors=None, coverage=None))
    return meshes


def view_frame(generator, latent, view, config):
    """One view of the colour stage: generator.staged_forward(latent, view, keep_depth_on_device=True, **config) -> (rgbs fp32
    [B,3,H,W] clamped to [-1, 1] as the apps clamp a frame, the distance along each ray fp32 [B,h,w] in world units: the normalised
    depth map taken back, depth_map * depth_length / 2 + focal / scale; it saturates where the map was clamped)."""
    out = generator.staged_forward(latent, view, **dict(config, keep_depth_on_device=True))
    zc = view["intrinsics"][:, 0, 0] / view["scales"].float()
    return out["rgbs"].float().clamp(-1, 1), out["depths"][:, 0].float() * (config["depth_length"] / 2.0) + zc.view(-1, 1, 1)


def colour(meshes, views, frames, depth_tolerance, normal_power, texture_size):
    """Carries the frames onto the meshes, in place -> meshes.  Mesh b takes item b of every view (conditions dicts) and of its
    view_frame, stacked: project_colors sets colors and coverage; with texture_size=S bake_texture of the same tensors then adds
    uvs [T,3,2], texture [S,S,3] and texture_coverage [S,S]."""
    for b, mesh in enumerate(meshes):
        seen = (torch.stack([im[b] for im, _ in frames]), torch.stack([d[b] for _, d in frames]),
                torch.stack([v["intrinsics"][b, 0, 0] for v in views]).float(), torch.stack([v["scales"][b] for v in views]).float(),
                torch.stack([v["cam2world_matrices"][b] for v in views]).float())
        mesh["colors"], mesh["coverage"] = project_colors(mesh["vertices"], mesh["normals"], *seen, depth_tolerance, normal_power)
        if texture_size is not None:
            texture, coverage = bake_texture(mesh["vertices"], mesh["faces"], mesh["normals"], *seen, depth_tolerance, texture_size,
                                             normal_power)
            uvs = torch.from_numpy(atlas_uvs(mesh["faces"].shape[0], texture_size)).to(texture.device)
            mesh.update(uvs=uvs, texture=texture, texture_coverage=coverage)
    return meshes


def rig(meshes, conditions, k):
    """Adds mesh_rig.bind's entries (rest_vertices, rest_normals, joints, weights, det) to mesh b from item b of the body of
    `conditions` (lbs_weights [B,V,J] or [V,J]), in place -> meshes"""
    lbs = conditions["lbs_weights"]
    for b, mesh in enumerate(meshes):
        mesh.update(mesh_rig.bind(mesh["vertices"], conditions["vertices"][b], lbs[b] if lbs.dim() == 3 else lbs,
                                  conditions["fk_matrices"][b], normals=mesh["normals"], k=k))
    return meshes
