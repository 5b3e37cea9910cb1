"""The stages of lib/generators/geometry_export.py without a device: the component calls are replaced on the module by recorders that
return small CPU tensors, so what is held here is the plumbing -- which component runs when, on which item's tensors -- and the
settings every public extract_* method resolves.  The numbers are held by the GPU tier, bit for bit against the parts."""
import importlib
import math
import re

import numpy as np
import pytest
import torch

ge = importlib.import_module("3dhumangan_amd.lib.generators.geometry_export")
mesh_texture = importlib.import_module("3dhumangan_amd.lib.components.mesh_texture")
CALLERS = ("extract_mesh", "extract_textured_mesh", "extract_avatar")
CFG = dict(ray_start=-1.0, ray_end=1.0, num_steps=8)
B, GRID, K = 2, (3, 4, 5), 2


# ------------------------------------------------------------------------------------------------------------------ settings
@pytest.mark.parametrize("who", CALLERS)
def test_settings_refusals_carry_the_callers_name(who):
    with pytest.raises(NotImplementedError, match=re.escape(f"{who}: clamp_mode='softplus' is not supported: only with 'relu' is the "
                                                            "raw output of the density head the density the renderer integrates")):
        ge.settings(who, dict(CFG, clamp_mode="softplus"))
    for power in (0, 9, 1.5):
        with pytest.raises(ValueError, match=re.escape(f"{who}: normal_power={power} must be an integer 1..8")):
            ge.settings(who, CFG, normal_power=power)
    for tolerance in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match=re.escape(f"{who}: depth_tolerance={tolerance} must be positive")):
            ge.settings(who, CFG, depth_tolerance=tolerance)
    with pytest.raises(ValueError, match=re.escape(f"{who}: texture_size needs at least one view to bake the texture from")):
        ge.settings(who, CFG, 0, texture_size=64)
    for simplify in (True, 0, math.inf, -2.0, "2"):
        with pytest.raises(ValueError, match=re.escape(f"{who}: simplify={simplify!r} must be a positive number (the cluster cell in "
                                                       "voxels) or None")):
            ge.settings(who, CFG, simplify=simplify)


def test_settings_refuse_the_clamp_mode_first():
    with pytest.raises(NotImplementedError, match="clamp_mode"):
        ge.settings("extract_avatar", dict(clamp_mode="softplus"), normal_power=0, simplify=True)      # no ray_start needed either


def test_settings_defaults():
    rays = dict(ray_start=0.5, ray_end=2.0)
    assert ge.settings("extract_mesh", rays).level == math.log(2.0) * 24 / 1.5
    assert ge.settings("extract_mesh", dict(rays, num_steps=12)).level == math.log(2.0) * 12 / 1.5
    assert ge.settings("extract_mesh", rays, level=-2.5).level == -2.5
    s = ge.settings("extract_textured_mesh", CFG)
    assert s.depth_tolerance == ge.default_depth_tolerance(CFG) == 0.5
    assert (s.normal_power, s.simplify, s.texture_size) == (2, None, None)
    assert ge.settings("extract_mesh", rays).depth_tolerance == 2.0 * 1.5 / 24
    s = ge.settings("extract_avatar", CFG, 1, depth_tolerance=0.25, normal_power=8, texture_size=64, simplify=3)
    assert s == (math.log(2.0) * 8 / 2.0, 0.25, 8, 3.0, 64) and type(s.simplify) is float
    assert ge.settings("extract_mesh", CFG, simplify=0.5).simplify == 0.5


# ------------------------------------------------------------------------------------------------------------------ surfaces
class Recorder:
    """stands in for the component functions of the module: every call is logged as (name, args, kwargs) in one list"""

    def __init__(self, monkeypatch):
        self.calls = []
        self.marched = [(torch.full((4 + b, 3), float(b)), torch.full((2 + b, 3), b, dtype=torch.int32)) for b in range(B)]
        self.clustered = [(torch.full((3, 3), 10.0 + b), torch.full((1 + b, 3), 10 + b, dtype=torch.int32), "cluster ids") for b in range(B)]
        for name in ("marching_tetrahedra", "simplify_mesh", "vertex_normals", "project_colors", "bake_texture"):
            monkeypatch.setattr(ge, name, lambda *a, _name=name, **kw: self.call(_name, a, kw))
        monkeypatch.setattr(ge.mesh_rig, "bind", lambda *a, **kw: self.call("bind", a, kw))

    def call(self, name, args, kwargs):
        n = sum(c[0] == name for c in self.calls)                      # the n-th call of this component
        self.calls.append((name, args, kwargs))
        if name == "marching_tetrahedra":
            return self.marched[n]
        if name == "simplify_mesh":
            return self.clustered[n]
        if name == "vertex_normals":
            return -args[1]
        if name == "project_colors":
            return torch.full((len(args[0]), 3), 0.5 + n), torch.full((len(args[0]),), 1.0 + n)
        if name == "bake_texture":
            size = args[9]
            return torch.full((size, size, 3), 0.25 + n), torch.full((size, size), 2.0 + n)
        return {key: f"{key} {n}" for key in ("rest_vertices", "rest_normals", "joints", "weights", "det")}

    def names(self):
        return [c[0] for c in self.calls]


def grid():
    sigma = torch.arange(B * 3 * 4 * 5, dtype=torch.float32).reshape(B, *GRID)
    return sigma, torch.tensor([[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]]), torch.tensor([[0.5] * 3, [0.25] * 3])


def test_surfaces_march_then_cluster_then_normals_per_item(monkeypatch):
    rec = Recorder(monkeypatch)
    sigma, origin, spacing = grid()
    meshes = ge.surfaces(sigma, origin, spacing, 1.5, 2.0, True)
    assert rec.names() == ["marching_tetrahedra", "simplify_mesh", "vertex_normals"] * B
    for b, mesh in enumerate(meshes):
        o, s = origin[b].tolist(), spacing[b].tolist()
        (_, march, kw0), (_, cluster, kw1), (_, normals, kw2) = rec.calls[3 * b:3 * b + 3]
        assert torch.equal(march[0], sigma[b]) and march[1:] == (1.5, o, s) and not kw0
        assert cluster[0] is rec.marched[b][0] and cluster[1] is rec.marched[b][1]
        assert cluster[2:] == (2.0 * s[0],) and kw1 == dict(origin=o, counts=[2, 2, 3])         # floor((N - 1) / 2) + 1 of 3, 4, 5
        assert torch.equal(normals[0], sigma[b]) and normals[1] is rec.clustered[b][0] and normals[2:] == (o, s) and not kw2
        assert list(mesh) == ["vertices", "faces", "normals", "colors", "coverage"]
        assert mesh["vertices"] is rec.clustered[b][0] and mesh["faces"] is rec.clustered[b][1]
        assert torch.equal(mesh["normals"], -rec.clustered[b][0]) and mesh["colors"] is None and mesh["coverage"] is None
    rec.calls.clear()
    ge.surfaces(sigma, origin, spacing, 1.5, 1.5, True)
    assert rec.calls[1][1][2] == 1.5 * 0.5 and rec.calls[1][2]["counts"] == [2, 3, 3]           # floor(2 / 1.5), (3 / 1.5), (4 / 1.5) + 1


def test_surfaces_launch_nothing_that_was_not_asked_for(monkeypatch):
    rec = Recorder(monkeypatch)
    sigma, origin, spacing = grid()
    meshes = ge.surfaces(sigma, origin, spacing, 1.5, None, False)                              # extract_mesh without simplify
    assert rec.names() == ["marching_tetrahedra"] * B
    assert all(m["vertices"] is rec.marched[b][0] and m["faces"] is rec.marched[b][1] and m["normals"] is None for b, m in enumerate(meshes))
    rec.calls.clear()
    ge.surfaces(sigma, origin, spacing, 1.5, 2.0, False)
    assert rec.names() == ["marching_tetrahedra", "simplify_mesh"] * B
    rec.calls.clear()
    meshes = ge.surfaces(sigma, origin, spacing, 1.5, None, True)
    assert rec.names() == ["marching_tetrahedra", "vertex_normals"] * B
    assert rec.calls[3][1][1] is rec.marched[1][0]                                              # normals at the unclustered vertices


# ---------------------------------------------------------------------------------------------------------------- view frame
def test_view_frame_is_one_staged_forward_with_the_depth_taken_back():
    class Generator:
        def staged_forward(self, latent, view, **config):
            self.seen = (latent, view, config)
            return dict(rgbs=torch.tensor([-3.0, 0.25, 3.0]).expand(B, 3, 4, 3), depths=torch.linspace(-1, 1, B * 6).reshape(B, 1, 2, 3))

    G = Generator()
    view = dict(intrinsics=torch.tensor([[[2.0]], [[3.0]]]), scales=torch.tensor([4.0, 2.0], dtype=torch.float64))
    config = dict(depth_length=0.5, generator="Map3DGenerator")            # the configs name the generator's class
    image, depth = ge.view_frame(G, "z", view, config)
    assert G.seen[0] == "z" and G.seen[1] is view and G.seen[2] == dict(config, keep_depth_on_device=True)
    assert "keep_depth_on_device" not in config
    assert image.shape == (B, 3, 4, 3) and torch.equal(image[0, 0, 0], torch.tensor([-1.0, 0.25, 1.0]))
    want = torch.linspace(-1, 1, B * 6).reshape(B, 2, 3) * 0.25 + torch.tensor([0.5, 1.5]).view(B, 1, 1)      # + focal / scale
    assert depth.dtype == torch.float32 and torch.equal(depth, want)


# -------------------------------------------------------------------------------------------------------------------- colour
def views_and_frames():
    gen = torch.Generator().manual_seed(3)
    views = [dict(intrinsics=torch.rand(B, 3, 3, generator=gen, dtype=torch.float64), scales=torch.rand(B, generator=gen, dtype=torch.float64),
                  cam2world_matrices=torch.rand(B, 4, 4, generator=gen, dtype=torch.float64)) for _ in range(K)]
    frames = [(torch.rand(B, 3, 4, 6, generator=gen), torch.rand(B, 2, 3, generator=gen)) for _ in range(K)]
    return views, frames


def plain_meshes():
    return [dict(vertices=torch.full((4 + b, 3), float(b)), faces=torch.zeros((6 + b, 3), dtype=torch.int32),
                 normals=torch.full((4 + b, 3), -float(b)), colors=None, coverage=None) for b in range(B)]


def assert_stacked(args, b, views, frames):
    """args = (images, depths, focals, scales, cam2world): item b of each view, in the order of the views, float32"""
    want = (torch.stack([frames[k][0][b] for k in range(K)]), torch.stack([frames[k][1][b] for k in range(K)]),
            torch.stack([views[k]["intrinsics"][b, 0, 0] for k in range(K)]).float(),
            torch.stack([views[k]["scales"][b] for k in range(K)]).float(),
            torch.stack([views[k]["cam2world_matrices"][b] for k in range(K)]).float())
    assert [tuple(t.shape) for t in args] == [(K, 3, 4, 6), (K, 2, 3), (K,), (K,), (K, 4, 4)]
    assert all(a.dtype == torch.float32 and torch.equal(a, w) for a, w in zip(args, want))


def test_colour_projects_item_b_of_every_view(monkeypatch):
    rec = Recorder(monkeypatch)
    views, frames = views_and_frames()
    meshes = plain_meshes()
    assert ge.colour(meshes, views, frames, 0.5, 2, None) is meshes
    assert rec.names() == ["project_colors"] * B                                                # no bake without a texture size
    for b, (mesh, (_, args, kwargs)) in enumerate(zip(meshes, rec.calls)):
        assert args[0] is mesh["vertices"] and args[1] is mesh["normals"] and args[7:] == (0.5, 2) and not kwargs
        assert_stacked(args[2:7], b, views, frames)
        assert list(mesh) == ["vertices", "faces", "normals", "colors", "coverage"]
        assert torch.equal(mesh["colors"], torch.full((4 + b, 3), 0.5 + b)) and torch.equal(mesh["coverage"], torch.full((4 + b,), 1.0 + b))


def test_colour_bakes_after_it_projects(monkeypatch):
    rec = Recorder(monkeypatch)
    views, frames = views_and_frames()
    meshes = ge.colour(plain_meshes(), views, frames, 0.25, 3, 16)
    assert rec.names() == ["project_colors", "bake_texture"] * B
    for b, mesh in enumerate(meshes):
        (_, project, _), (_, bake, kwargs) = rec.calls[2 * b:2 * b + 2]
        assert bake[0] is mesh["vertices"] and bake[1] is mesh["faces"] and bake[2] is mesh["normals"] and bake[8:] == (0.25, 16, 3)
        assert not kwargs and project[7:] == (0.25, 3)
        assert_stacked(bake[3:8], b, views, frames)
        assert all(p is q for p, q in zip(project[2:7], bake[3:8]))                             # stacked once, used by both
        assert list(mesh) == ["vertices", "faces", "normals", "colors", "coverage", "uvs", "texture", "texture_coverage"]
        assert np.array_equal(mesh["uvs"].numpy(), mesh_texture.atlas_uvs(6 + b, 16)) and mesh["uvs"].shape == (6 + b, 3, 2)
        assert torch.equal(mesh["texture"], torch.full((16, 16, 3), 0.25 + b))
        assert torch.equal(mesh["texture_coverage"], torch.full((16, 16), 2.0 + b))
        assert torch.equal(mesh["colors"], torch.full((4 + b, 3), 0.5 + b))                    # what they are without the texture


# ----------------------------------------------------------------------------------------------------------------------- rig
@pytest.mark.parametrize("shared_weights", (False, True))
def test_rig_binds_item_b_to_its_body(monkeypatch, shared_weights):
    rec = Recorder(monkeypatch)
    gen = torch.Generator().manual_seed(5)
    body = dict(vertices=torch.rand(B, 7, 3, generator=gen), fk_matrices=torch.rand(B, 4, 4, 4, generator=gen),
                lbs_weights=torch.rand(7, 4, generator=gen) if shared_weights else torch.rand(B, 7, 4, generator=gen))
    meshes = plain_meshes()
    assert ge.rig(meshes, body, 3) is meshes
    assert rec.names() == ["bind"] * B
    for b, (mesh, (_, args, kwargs)) in enumerate(zip(meshes, rec.calls)):
        assert args[0] is mesh["vertices"] and torch.equal(args[1], body["vertices"][b]) and torch.equal(args[3], body["fk_matrices"][b])
        assert torch.equal(args[2], body["lbs_weights"] if shared_weights else body["lbs_weights"][b]) and args[2].shape == (7, 4)
        assert len(args) == 4 and set(kwargs) == {"normals", "k"} and kwargs["normals"] is mesh["normals"] and kwargs["k"] == 3
        assert list(mesh)[5:] == ["rest_vertices", "rest_normals", "joints", "weights", "det"]
        assert all(mesh[key] == f"{key} {b}" for key in list(mesh)[5:])
