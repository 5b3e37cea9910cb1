"""The texture atlas without a GPU: the layout of lib/components/mesh_texture.py against the restatement
(tests/_texture_bake_reference.py) and its two properties, what the texture is for (a bilinear atlas lookup is closer to the frames
than interpolated vertex colours), the PNG / glTF writers, and bake_texture's refusals."""
import importlib
import struct
import zlib

import numpy as np
import pytest
import torch

import _mesh_rig_reference as RIG
import _texture_bake_reference as R
from _mesh_attributes_reference import project_colors

mesh_texture = importlib.import_module("3dhumangan_amd.lib.components.mesh_texture")
mesh_io = importlib.import_module("3dhumangan_amd.lib.components.mesh_io")
f32, f64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("T,S", R.LAYOUT_CASES)
def test_layout_is_the_restatement_and_has_its_two_properties(T, S):
    c, per_row = R.layout(T, S)
    assert mesh_texture.atlas_layout(T, S) == (c, per_row) and c >= 4
    uv = mesh_texture.atlas_uvs(T, S)
    assert uv.dtype == f32 and uv.shape == (T, 3, 2) and np.array_equal(uv, R.uvs(T, S).astype(f32))
    owner, bary = R.ownership(T, S, f32)
    # 1. the texel under each corner belongs to the triangle and carries the one-hot barycentrics of that corner
    centre = R.uvs(T, S) * S - 0.5
    assert np.abs(centre - np.round(centre)).max() < 1e-9    # a corner lies on a texel centre (S need not be a power of two)
    q, r = np.round(centre[..., 0]).astype(int), np.round(centre[..., 1]).astype(int)
    assert np.array_equal(owner[r, q], np.repeat(np.arange(T)[:, None], 3, axis=1))
    assert np.array_equal(bary[r, q], np.broadcast_to(np.eye(3, dtype=f32), (T, 3, 3)))
    # 2. the bilinear footprint of any point of a UV triangle (corners, edges, inside) touches that triangle's texels only; on a
    #    corner or an edge the rounding of the point's own coordinates may give a neighbour a weight of the order of 1e-16
    rng = np.random.default_rng(T + S)
    inside = rng.dirichlet(np.ones(3), size=(T, 200))
    edges = np.concatenate([np.eye(3), [[.5, .5, 0], [0, .5, .5], [.5, 0, .5], [.999, .001, 0], [0, .001, .999], [.001, 0, .999]]])
    b = np.concatenate([inside, np.broadcast_to(edges, (T,) + edges.shape)], axis=1)                 # [T,n,3]
    points = np.einsum("tnk,tkc->tnc", b, R.uvs(T, S))
    rows, cols, w = R.lookup_taps(points.reshape(-1, 2), S)
    wants = np.repeat(np.arange(T), b.shape[1])[:, None]
    assert (w >= 0).all() and np.abs(w.sum(axis=1) - 1).max() < 1e-12
    assert ((owner[rows, cols] == wants) | (w < 1e-12)).all()
    assert (owner >= 0).sum() >= T * 6                      # every triangle owns at least its six texels


def test_layout_refusals():
    with pytest.raises(ValueError, match="smallest size is 32"):
        mesh_texture.atlas_layout(128, 31)                   # R = 8: cells of 3
    assert mesh_texture.atlas_layout(128, 32) == (4, 8)
    with pytest.raises(ValueError, match="smallest size is 4"):
        mesh_texture.atlas_uvs(2, 3)
    for size in (1, 8193, 0, -4):
        with pytest.raises(ValueError, match="outside 2..8192"):
            mesh_texture.atlas_layout(2, size)
    assert mesh_texture.atlas_layout(0, 4) == (4, 1) and mesh_texture.atlas_uvs(0, 4).shape == (0, 3, 2)
    assert mesh_texture.atlas_layout(2 * 2048 * 2048, 8192) == (4, 2048)


# ----------------------------------------------------------------------------------------------------------------- purpose
@pytest.mark.parametrize("n,S", [(2, 64), (2, 128), (3, 256)])
def test_a_texture_lookup_is_closer_to_the_frames_than_vertex_colours(n, S):
    """20 000 random surface points that the views see (reference coverage >= 0.1): the RMS error of the viewer's bilinear atlas lookup
    against the direct evaluation of the definition there is at most half that of barycentric interpolation of the vertex colours.
    Measured here: 0.047 / 0.316 (n = 2, S = 64; 39 % of the points seen), 0.015 / 0.316 (2, 128; 40 %) and 0.011 / 0.120 (3, 256; 76 %);
    the factor 2 leaves room for another random draw."""
    K, tolerance, power = 5, 0.05, 2
    s = R.detailed_scene(K, 64, 64, 128, 128)
    vertices, normals, faces = R.octa_sphere(n, s["centre"], s["radius"])
    views = (s["images"], s["depths"], s["focals"], s["scales"], s["cam2world"], tolerance, power)
    texture, _, _ = R.bake(vertices, faces, normals, s, tolerance, S, power)
    vertex_colors, _ = project_colors(vertices, normals, *views)
    triangles, bary = R.mesh_points(vertices, faces, 60000, seed=n + S)
    x, nrm = R.surface_point(vertices, normals, faces, triangles, bary, f64)
    direct, coverage = R.colour_at(x, nrm, s["images"], s["depths"], s["focals"], s["cam2world"], tolerance, power, 0.0, 1e-3, f64)
    seen = np.flatnonzero(coverage >= 0.1)
    share = len(seen) / len(coverage)
    seen = seen[:20000]
    assert len(seen) == 20000
    uv = np.einsum("nk,nkc->nc", bary, R.uvs(len(faces), S)[triangles])
    from_texture = R.lookup(texture, uv)
    from_vertices = np.einsum("nk,nkc->nc", bary, vertex_colors[faces[triangles]])
    rms_texture = float(np.sqrt(((from_texture - direct)[seen] ** 2).mean()))
    rms_vertices = float(np.sqrt(((from_vertices - direct)[seen] ** 2).mean()))
    print(f"n={n} ({len(faces)} triangles) S={S}: texture RMS {rms_texture:.4f}, vertex colours RMS {rms_vertices:.4f}, seen {100 * share:.0f} %")
    assert rms_texture <= 0.5 * rms_vertices


# --------------------------------------------------------------------------------------------------------------- PNG / GLB
def decode_png(data):
    """a reader for what encode_png promises: 8-bit RGB, filter 0 on every row, no interlace -> uint8 [H,W,3]"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        chunks.append((kind, body))
        at += 12 + n
    assert [k for k, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"") and at == len(data)
    W, H, depth, colour, compression, filtering, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, compression, filtering, interlace) == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(b"".join(b for k, b in chunks if k == b"IDAT")), dtype=np.uint8).reshape(H, 1 + 3 * W)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(H, W, 3)


@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (64, 64), (7, 130)])
def test_png_round_trip(shape):
    rgb = np.random.default_rng(sum(shape)).integers(0, 256, size=shape + (3,), dtype=np.uint8)
    assert np.array_equal(decode_png(mesh_io.encode_png(rgb)), rgb)
    with pytest.raises(ValueError, match="uint8"):
        mesh_io.encode_png(rgb.astype(np.float32))


def glb_image(glb):
    """the one embedded image of a file read by the Glb reader -> uint8 [S,S,3], asserting the material / texture / sampler chain"""
    j = glb.json
    assert j["meshes"][0]["primitives"][0]["material"] == 0 and len(j["materials"]) == 1
    assert j["materials"][0] == {"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicFactor": 0, "roughnessFactor": 1}}
    assert j["textures"] == [{"sampler": 0, "source": 0}]
    assert j["samplers"] == [{"magFilter": 9729, "minFilter": 9729, "wrapS": 33071, "wrapT": 33071}]
    (image,) = j["images"]
    assert image["mimeType"] == "image/png"
    view = j["bufferViews"][image["bufferView"]]
    assert view["byteOffset"] % 4 == 0 and "target" not in view
    return decode_png(glb.bin[view["byteOffset"]:view["byteOffset"] + view["byteLength"]])


def test_texture_bytes_are_the_ply_conversion():
    t = np.array([[[-1.0, 0.0, 1.0], [np.nan, 2.0, -3.0]], [[0.999, -0.999, 0.5], [1e-3, np.inf, -np.inf]]], dtype=f32)
    want = np.nan_to_num(np.clip((t * f32(0.5) + f32(0.5)) * f32(255), 0, 255), nan=0.0).astype("u1")
    assert np.array_equal(mesh_texture.texture_bytes(t), want) and np.array_equal(mesh_texture.texture_bytes(torch.as_tensor(t)), want)
    assert want[0, 0].tolist() == [0, 127, 255] and want[0, 1].tolist() == [0, 255, 0]


def test_glb_with_a_texture_skinned_and_static(tmp_path):
    rig = RIG.make_rig(40, 5, seed=3, n_poses=2)
    rng = np.random.default_rng(0)
    V, T, S = 40, 21, 16
    vertices = rig["rest"].astype(f32)
    faces = rng.integers(0, V, size=(T, 3)).astype(np.int32)
    normals = rng.normal(size=(V, 3)).astype(f32)
    joints = rng.integers(0, 5, size=(V, 4))
    weights = rng.dirichlet(np.ones(4), size=V).astype(f32)
    texture = rng.uniform(-1.1, 1.1, size=(S, S, 3)).astype(f32)
    uvs = mesh_texture.atlas_uvs(T, S)
    corner = faces.reshape(-1)

    def check(glb, skinned):
        assert np.array_equal(glb.faces(), np.arange(3 * T).reshape(T, 3))
        assert np.array_equal(glb.attribute("POSITION"), vertices[corner]) and np.array_equal(glb.attribute("NORMAL"), normals[corner])
        assert np.array_equal(glb.attribute("TEXCOORD_0"), uvs.reshape(-1, 2))
        assert "COLOR_0" not in glb.json["meshes"][0]["primitives"][0]["attributes"]
        assert np.array_equal(glb_image(glb), mesh_texture.texture_bytes(texture))
        if skinned:
            assert np.array_equal(glb.attribute("JOINTS_0"), joints[corner]) and np.array_equal(glb.attribute("WEIGHTS_0"), weights[corner])
        else:
            assert set(glb.json["meshes"][0]["primitives"][0]["attributes"]) == {"POSITION", "NORMAL", "TEXCOORD_0"}
            assert "skins" not in glb.json and "animations" not in glb.json
            assert glb.json["nodes"] == [{"name": "mesh", "mesh": 0}] and glb.json["scenes"] == [{"nodes": [0]}]

    path = str(tmp_path / "skinned.glb")
    mesh_io.write_glb(path, vertices, faces, joints, weights, rig["rest_joints"], rig["parents"], normals=normals, frames=rig["A"],
                      uvs=uvs, texture=texture)
    glb = RIG.Glb(path)
    check(glb, True)
    posed = (np.einsum("vk,vkab->vab", weights.astype(f64), rig["A"][1].astype(f64)[joints]))
    want = (posed[:, :3, :3] @ vertices.astype(f64)[:, :, None])[..., 0] + posed[:, :3, 3]
    assert np.abs(glb.skinned(1) - want[corner]).max() <= RIG.evaluator_bar(rig["parents"], want)
    path = str(tmp_path / "static.glb")
    mesh_io.write_glb(path, torch.as_tensor(vertices), torch.as_tensor(faces), normals=normals, uvs=torch.as_tensor(uvs),
                      texture=torch.as_tensor(texture))
    check(RIG.Glb(path), False)
    # uint8 textures are taken as they are; a static mesh without a texture keeps its index list and may carry colours
    mesh_io.write_glb(path, vertices, faces, uvs=uvs, texture=mesh_texture.texture_bytes(texture))
    assert np.array_equal(glb_image(RIG.Glb(path)), mesh_texture.texture_bytes(texture))
    mesh_io.write_glb(path, vertices, faces, colors=normals)
    plain = RIG.Glb(path)
    assert np.array_equal(plain.faces(), faces) and "images" not in plain.json and plain.attribute("COLOR_0").shape == (V, 4)
    with pytest.raises(ValueError, match="colors and texture"):
        mesh_io.write_glb(path, vertices, faces, joints, weights, rig["rest_joints"], rig["parents"], colors=normals, uvs=uvs, texture=texture)
    with pytest.raises(ValueError, match="uvs and texture go together"):
        mesh_io.write_glb(path, vertices, faces, uvs=uvs)
    with pytest.raises(ValueError, match="go together"):
        mesh_io.write_glb(path, vertices, faces, joints, weights)
    with pytest.raises(ValueError, match="frames need a skeleton"):
        mesh_io.write_glb(path, vertices, faces, frames=rig["A"])
    with pytest.raises(ValueError, match="uvs must be"):
        mesh_io.write_glb(path, vertices, faces, uvs=uvs[:-1], texture=texture)


def test_glb_without_the_new_arguments_is_unchanged(tmp_path):
    """the skinned, coloured file of the rig tests: the same bytes whether the new keywords are left out or passed as None"""
    rig = RIG.make_rig(30, 4, seed=5, n_poses=2)
    rng = np.random.default_rng(1)
    args = (rig["rest"].astype(f32), rng.integers(0, 30, size=(11, 3)), rng.integers(0, 4, size=(30, 4)),
            rng.dirichlet(np.ones(4), size=30).astype(f32), rig["rest_joints"], rig["parents"])
    colors = rng.uniform(-1, 1, size=(30, 3)).astype(f32)
    a, b = str(tmp_path / "a.glb"), str(tmp_path / "b.glb")
    mesh_io.write_glb(a, *args, colors=colors, frames=rig["A"])
    mesh_io.write_glb(b, *args, colors=colors, frames=rig["A"], uvs=None, texture=None)
    assert open(a, "rb").read() == open(b, "rb").read()
    glb = RIG.Glb(a)
    assert list(glb.json) == ["asset", "scene", "scenes", "nodes", "meshes", "skins", "animations", "buffers", "bufferViews", "accessors"]
    assert list(glb.json["meshes"][0]["primitives"][0]["attributes"]) == ["POSITION", "COLOR_0", "JOINTS_0", "WEIGHTS_0"]
    assert list(glb.json["meshes"][0]["primitives"][0]) == ["attributes", "indices", "mode"]


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_bake_texture_refuses_bad_arguments_without_a_gpu():
    _lib = importlib.import_module("3dhumangan_amd._lib")
    K, V, T = 2, 9, 4
    good = dict(vertices=torch.zeros(V, 3), faces=torch.zeros(T, 3, dtype=torch.int32), normals=torch.zeros(V, 3),
                images=torch.zeros(K, 3, 4, 4), depths=torch.zeros(K, 2, 2), focals=torch.ones(K), scales=torch.ones(K),
                cam2world=torch.eye(4).repeat(K, 1, 1), depth_tolerance=0.1, size=8)

    def refused(match, error=ValueError, **change):
        with pytest.raises(error, match=match):
            mesh_texture.bake_texture(**dict(good, **change))

    refused("vertices must be a tensor", TypeError, vertices=np.zeros((V, 3), dtype=f32))
    refused("vertices must be float32", vertices=torch.zeros(V, 3, dtype=torch.float64))
    refused("normals must be float32", normals=torch.zeros(V, 4))
    refused("8 normals for 9 vertices", normals=torch.zeros(8, 3))
    refused("faces must be int32", faces=torch.zeros(T, 3, dtype=torch.int64))
    refused("faces must be int32", faces=torch.zeros(T, 4, dtype=torch.int32))
    refused("triangles without a vertex", vertices=torch.zeros(0, 3), normals=torch.zeros(0, 3))
    refused("images must be float32", images=torch.zeros(K, 4, 4, 4))
    refused("depths must be float32", depths=torch.zeros(K, 1, 2))
    refused("at least one view", images=torch.zeros(0, 3, 4, 4), depths=torch.zeros(0, 2, 2))
    refused("focals has shape", focals=torch.ones(K + 1))
    refused("cam2world has shape", cam2world=torch.eye(4).repeat(K, 1, 1)[:, :3])
    refused("depth_tolerance=0.0", depth_tolerance=0.0)
    refused("eps=", eps=float("inf"))
    refused("normal_power=9", normal_power=9)
    refused("smallest size is 8", size=7)                    # 4 triangles: 2 x 2 cells
    refused("outside 2..8192", size=8193)
    refused("must be an integer", size=8.5)
    refused("ROCm device only", _lib.H3DError)               # every argument is fine: the CPU tensors are what is refused


def test_the_library_refuses_bad_arguments_before_any_device_call():
    """h3d_mesh_bake_texture's own checks (the layout is computed a second time there, in C): no GPU is touched by a refused call"""
    import os
    import re
    _lib = importlib.import_module("3dhumangan_amd._lib")
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "h3d.h")).read(), flags=re.S)
    declared = re.search(r"h3d_mesh_bake_texture\s*\(([^)]*)\)", header).group(1).split(",")
    assert len(declared) == len(_lib._SIGNATURES["h3d_mesh_bake_texture"][1]) == 21

    def call(V=9, T=4, S=8, K=2, H=4, W=4, h=2, w=2, tolerance=0.1, power=2, eps=1e-3):
        rc = lib.h3d_mesh_bake_texture(None, None, V, None, T, S, None, K, H, W, None, h, w, None, tolerance, power, 0.0, eps, None, None, None)
        return rc, lib.h3d_last_error().decode()

    for kwargs, message in ((dict(S=7), "at least 8 texels"), (dict(S=1), "S=1 outside 2..8192"), (dict(S=8193), "outside 2..8192"),
                            (dict(T=-1), "T=-1 out of range"), (dict(T=128, S=31), "at least 32 texels"), (dict(K=0), "K=0 views"),
                            (dict(h=1), "need at least 2x2"), (dict(tolerance=0.0), "depth_tolerance=0 must be positive"),
                            (dict(eps=float("nan")), "eps=nan must be positive"), (dict(power=9), "normal_power=9 outside 1..8"),
                            (dict(V=0), "4 triangles without a vertex"), (dict(), "null pointer"), (dict(T=0), "null pointer")):
        rc, said = call(**kwargs)
        assert rc == -1 and message in said, (kwargs, rc, said)
