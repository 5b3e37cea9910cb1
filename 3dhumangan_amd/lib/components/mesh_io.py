"""Mesh files.  write_ply: an indexed triangle mesh as binary little-endian PLY (float x y z, optionally float nx ny nz and uchar red
green blue per vertex, then uchar-int face lists).  write_glb: a mesh -- static, or skinned with its skeleton and, optionally, one
animation -- with vertex colours or a texture, as a binary glTF 2.0 file.  encode_png: an 8-bit RGB image as PNG bytes.  json, struct,
zlib and numpy only."""
import json
import struct
import zlib

import numpy as np


def color_bytes(c):
    """floats in [-1, 1] -> uint8 of the same shape, as the apps convert images: *0.5+0.5, *255, clamp, truncate; NaN gives 0"""
    c = np.asarray(c, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.nan_to_num(np.clip((c * np.float32(0.5) + np.float32(0.5)) * np.float32(255), 0, 255), nan=0.0).astype("u1")


def encode_png(rgb):
    """rgb uint8 [H,W,3] -> the bytes of a PNG file: 8-bit RGB (colour type 2), every row with filter 0, no interlace; the chunks
    IHDR, IDAT (one zlib stream) and IEND, each with its CRC"""
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        raise ValueError(f"encode_png: rgb must be uint8 [H,W,3], got {rgb.dtype} {rgb.shape}")
    H, W = rgb.shape[:2]
    rows = np.zeros((H, 1 + 3 * W), dtype=np.uint8)          # column 0: the filter type of the row
    rows[:, 1:] = rgb.reshape(H, 3 * W)

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


def _as_array(a, dtype, what):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"write_ply: {what} must be [n,3], got {a.shape}")
    return np.ascontiguousarray(a, dtype=dtype)


def write_ply(path, vertices, faces, normals=None, colors=None):
    """vertices [V,3] (floating), faces [T,3] (integer indices into vertices); tensors or arrays.  normals [V,3] (floating) add
    `float nx ny nz`; colors [V,3] in [-1, 1] add `uchar red green blue`, converted as the apps convert images (*0.5+0.5, *255, clamp,
    truncate; NaN gives 0).  With both omitted the file is positions and faces only."""
    v = _as_array(vertices, "<f4", "vertices")
    f = _as_array(faces, "<i4", "faces")
    columns, fields = [("xyz", "<f4", (3,))], {"xyz": v}
    props = "property float x\nproperty float y\nproperty float z\n"
    if normals is not None:
        fields["n"] = _as_array(normals, "<f4", "normals")
        columns.append(("n", "<f4", (3,)))
        props += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors is not None:
        fields["rgb"] = color_bytes(_as_array(colors, "<f4", "colors"))
        columns.append(("rgb", "u1", (3,)))
        props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    for name, a in fields.items():
        if len(a) != len(v):
            raise ValueError(f"write_ply: {len(a)} rows of {'normals' if name == 'n' else 'colors'} for {len(v)} vertices")
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"write_ply: face index outside [0, {len(v)})")
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {len(v)}\n{props}"
              f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
    rows = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    rows["n"] = 3
    rows["i"] = f
    with open(path, "wb") as out:
        out.write(header.encode("ascii"))
        if len(columns) == 1:
            out.write(v.tobytes())
        else:
            table = np.empty(len(v), dtype=columns)            # packed: 12, 24, 15 or 27 bytes per vertex
            for name, a in fields.items():
                table[name] = a
            out.write(table.tobytes())
        out.write(rows.tobytes())


# --- binary glTF 2.0 ----------------------------------------------------------------------------------------------------------
_FLOAT, _UBYTE, _UINT = 5126, 5121, 5125
_ARRAY_BUFFER, _ELEMENT_ARRAY_BUFFER = 34962, 34963
RIGID_TOLERANCE = 1e-4


def _numpy(a):
    return np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a)


def _table(a, shape, dtype, what):
    a = _numpy(a)
    if a.ndim != len(shape) or any(want is not None and have != want for have, want in zip(a.shape, shape)):
        raise ValueError(f"write_glb: {what} must be [{','.join('n' if s is None else str(s) for s in shape)}], got {a.shape}")
    return np.ascontiguousarray(a, dtype=dtype)


def _quaternions(R):
    """rotation matrices [n,3,3] float64 -> unit quaternions (x, y, z, w) [n,4]: per matrix the largest of the four candidates is the
    pivot (Shepperd), so no division by a small number"""
    m = R
    t = np.stack([1 + m[:, 0, 0] - m[:, 1, 1] - m[:, 2, 2], 1 - m[:, 0, 0] + m[:, 1, 1] - m[:, 2, 2],
                  1 - m[:, 0, 0] - m[:, 1, 1] + m[:, 2, 2], 1 + m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2]], axis=1)
    q = np.empty((len(m), 4))
    pivot = t.argmax(axis=1)
    for p in range(4):
        s = pivot == p
        if not s.any():
            continue
        a = m[s]
        if p == 0:
            v = [t[s, 0], a[:, 0, 1] + a[:, 1, 0], a[:, 0, 2] + a[:, 2, 0], a[:, 2, 1] - a[:, 1, 2]]
        elif p == 1:
            v = [a[:, 0, 1] + a[:, 1, 0], t[s, 1], a[:, 1, 2] + a[:, 2, 1], a[:, 0, 2] - a[:, 2, 0]]
        elif p == 2:
            v = [a[:, 0, 2] + a[:, 2, 0], a[:, 1, 2] + a[:, 2, 1], t[s, 2], a[:, 1, 0] - a[:, 0, 1]]
        else:
            v = [a[:, 2, 1] - a[:, 1, 2], a[:, 0, 2] - a[:, 2, 0], a[:, 1, 0] - a[:, 0, 1], t[s, 3]]
        q[s] = np.stack(v, axis=1)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _local_transforms(frames, rest_joints, parents):
    """frames [n,J,4,4] (rest -> posed bone transforms) -> per joint the transform relative to its parent, float64 [n,J,4,4]:
    global_j = A_j . translate(J_j), local_j = global_parent^-1 . global_j (the root's parent is the world)"""
    G = frames.astype(np.float64).copy()
    G[:, :, :3, 3] += np.einsum("njab,jb->nja", G[:, :, :3, :3], rest_joints)
    local = G.copy()
    for j, p in enumerate(parents):
        if p >= 0:
            local[:, j] = np.linalg.inv(G[:, p]) @ G[:, j]
    return local


def write_glb(path, vertices, faces, joints=None, weights=None, rest_joints=None, parents=None, normals=None, colors=None, frames=None,
              fps=20, uvs=None, texture=None):
    """One binary glTF 2.0 file: the REST-pose mesh (vertices [M,3], faces [T,3], normals [M,3] optional, colors [M,3] in [-1, 1]
    optional: COLOR_0 as normalised bytes, converted as write_ply converts them), its skin (joints [M,4] integer, weights [M,4]:
    JOINTS_0 as unsigned bytes, WEIGHTS_0 as floats) and skeleton (rest_joints [J,3] the joint positions at rest, parents [J] with
    -1 for a root and parents[j] < j): one node per joint, translation J_j - J_parent, inverse bind matrices translate(-J_j).
    frames [n,J,4,4]: bone transforms (rest -> posed, conditions["fk_matrices"]) of n poses, written as one animation with keys at
    i / fps -- a rotation channel per joint (unit quaternions, the sign of each key chosen so that consecutive keys have a
    non-negative dot product) and a translation channel for every root.  A local transform that is not a rotation (within 1e-4), or
    that moves a joint against its parent, cannot be stored this way: ValueError naming joint and frame.
    joints = weights = rest_joints = parents = None: a static mesh -- one node, no skin, no animation (frames must be None).
    uvs [T,3,2] (per face corner, v = 0 at the top row) with texture [S,S,3] (floats in [-1, 1], converted as colours are, or uint8
    as it is): the primitive is de-indexed -- 3T vertices in face order, POSITION / NORMAL / JOINTS_0 / WEIGHTS_0 gathered per
    corner, indices 0..3T-1, TEXCOORD_0 = uvs -- and the texture is embedded as a PNG behind one material (baseColorTexture,
    metallicFactor 0, roughnessFactor 1) with one sampler (LINEAR / LINEAR, CLAMP_TO_EDGE: the atlas has no mipmaps).  colors and
    texture together: ValueError, glTF would multiply them."""
    v = _table(vertices, (None, 3), "<f4", "vertices")
    M = len(v)
    if M == 0:
        raise ValueError("write_glb: vertices is empty: glTF has no empty accessor")
    f = _table(faces, (None, 3), "<i8", "faces")
    if len(f) == 0:
        raise ValueError("write_glb: faces is empty: glTF has no empty accessor")
    if f.min() < 0 or f.max() >= M:
        raise ValueError(f"write_glb: face index outside [0, {M})")
    f = f.astype("<u4")
    rig = [a is not None for a in (joints, weights, rest_joints, parents)]
    if any(rig) and not all(rig):
        raise ValueError("write_glb: joints, weights, rest_joints and parents go together (all None: a static mesh)")
    skinned = all(rig)
    if not skinned and frames is not None:
        raise ValueError("write_glb: frames need a skeleton (joints, weights, rest_joints, parents)")
    if (uvs is None) != (texture is None):
        raise ValueError("write_glb: uvs and texture go together")
    if texture is not None and colors is not None:
        raise ValueError("write_glb: colors and texture together: glTF multiplies COLOR_0 into the base colour, pass one of them")
    if skinned:
        rest = _table(rest_joints, (None, 3), "<f8", "rest_joints")
        J = len(rest)
        if not 1 <= J <= 256:
            raise ValueError(f"write_glb: {J} joints; JOINTS_0 is written as unsigned bytes (1..256 joints)")
        par = [int(p) for p in _numpy(parents).reshape(-1)]
        if len(par) != J:
            raise ValueError(f"write_glb: parents must have {J} entries, got {len(par)}")
        for j, p in enumerate(par):
            if not -1 <= p < j:
                raise ValueError(f"write_glb: parents[{j}] = {p} is not -1 or in [0, {j}): a joint must follow its parent")
        jt = _table(joints, (M, 4), "<i8", "joints")
        if jt.min() < 0 or jt.max() >= J:
            raise ValueError(f"write_glb: joints outside [0, {J})")
        wt = _table(weights, (M, 4), "<f4", "weights")
        if not np.isfinite(wt).all():
            raise ValueError("write_glb: vertices and weights must be finite")
    if not np.isfinite(v).all():
        raise ValueError("write_glb: vertices and weights must be finite")
    if not float(fps) > 0:
        raise ValueError(f"write_glb: fps={fps} must be positive")
    nrm = None if normals is None else _table(normals, (M, 3), "<f4", "normals")
    if texture is not None:
        uv = _table(uvs, (len(f), 3, 2), "<f4", "uvs").reshape(-1, 2)
        image = _numpy(texture)
        if image.ndim != 3 or image.shape[2] != 3:
            raise ValueError(f"write_glb: texture must be [S,S,3], got {image.shape}")
        image = image if image.dtype == np.uint8 else color_bytes(image)
        corner = f.reshape(-1).astype(np.int64)               # de-indexed: a vertex per face corner, in face order
        v, nrm = v[corner], None if nrm is None else nrm[corner]
        if skinned:
            jt, wt = jt[corner], wt[corner]
        f = np.arange(len(corner), dtype="<u4").reshape(-1, 3)
        M = len(v)

    blob, views, accessors = bytearray(), [], []

    def accessor(array, component, kind, target=None, bounds=False, normalized=False):
        raw = np.ascontiguousarray(array).tobytes()
        views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": len(raw)})
        if target is not None:
            views[-1]["target"] = target
        blob.extend(raw)
        blob.extend(b"\0" * (-len(blob) % 4))
        acc = {"bufferView": len(views) - 1, "componentType": component, "count": len(array), "type": kind}
        if normalized:
            acc["normalized"] = True
        if bounds:
            flat = np.asarray(array, dtype=np.float64).reshape(len(array), -1)
            acc["min"], acc["max"] = [float(x) for x in flat.min(axis=0)], [float(x) for x in flat.max(axis=0)]
        accessors.append(acc)
        return len(accessors) - 1

    attributes = {"POSITION": accessor(v, _FLOAT, "VEC3", _ARRAY_BUFFER, bounds=True)}
    if nrm is not None:
        attributes["NORMAL"] = accessor(nrm, _FLOAT, "VEC3", _ARRAY_BUFFER)
    if texture is not None:
        attributes["TEXCOORD_0"] = accessor(uv, _FLOAT, "VEC2", _ARRAY_BUFFER)
    if colors is not None:
        rgba = np.full((M, 4), 255, dtype="u1")
        rgba[:, :3] = color_bytes(_table(colors, (M, 3), "<f4", "colors"))
        attributes["COLOR_0"] = accessor(rgba, _UBYTE, "VEC4", _ARRAY_BUFFER, normalized=True)
    if skinned:
        attributes["JOINTS_0"] = accessor(jt.astype("u1"), _UBYTE, "VEC4", _ARRAY_BUFFER)
        attributes["WEIGHTS_0"] = accessor(wt, _FLOAT, "VEC4", _ARRAY_BUFFER)
    indices = accessor(f.reshape(-1), _UINT, "SCALAR", _ELEMENT_ARRAY_BUFFER)
    primitive = {"attributes": attributes, "indices": indices, "mode": 4}
    gltf = {"asset": {"version": "2.0", "generator": "3dhumangan_amd"}, "scene": 0}
    if texture is not None:
        png = encode_png(image)
        views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": len(png)})
        blob.extend(png)
        blob.extend(b"\0" * (-len(blob) % 4))
        primitive["material"] = 0
        gltf["materials"] = [{"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicFactor": 0, "roughnessFactor": 1}}]
        gltf["textures"] = [{"sampler": 0, "source": 0}]
        gltf["samplers"] = [{"magFilter": 9729, "minFilter": 9729, "wrapS": 33071, "wrapT": 33071}]
        gltf["images"] = [{"bufferView": len(views) - 1, "mimeType": "image/png"}]
    if not skinned:
        gltf.update(scenes=[{"nodes": [0]}], nodes=[{"name": "mesh", "mesh": 0}], meshes=[{"primitives": [primitive]}])
        return _write_container(path, gltf, blob, views, accessors)

    inverse_bind = np.tile(np.eye(4, dtype="<f4").reshape(1, 16), (J, 1))      # column-major: the translation is entries 12..14
    inverse_bind[:, 12:15] = -rest
    offsets = rest - np.where(np.array(par)[:, None] >= 0, rest[np.maximum(par, 0)], 0.0)
    nodes = [{"name": f"joint_{j}", "translation": [float(x) for x in offsets[j].astype(np.float32)]} for j in range(J)]
    for j, p in enumerate(par):
        if p >= 0:
            nodes[p].setdefault("children", []).append(j)
    roots = [j for j, p in enumerate(par) if p < 0]
    nodes.append({"name": "avatar", "mesh": 0, "skin": 0})
    gltf.update(scenes=[{"nodes": roots + [J]}], nodes=nodes, meshes=[{"primitives": [primitive]}],
                skins=[{"joints": list(range(J)), "skeleton": roots[0],
                        "inverseBindMatrices": accessor(inverse_bind.reshape(J, 16), _FLOAT, "MAT4")}])

    if frames is not None:
        fr = _table(frames, (None, J, 4, 4), "<f8", "frames")
        n = len(fr)
        if n == 0:
            raise ValueError("write_glb: frames is empty: pass None for a file without an animation")
        local = _local_transforms(fr, rest, par)
        R, t = local[:, :, :3, :3], local[:, :, :3, 3]
        off = np.abs(np.swapaxes(R, -1, -2) @ R - np.eye(3)).max(axis=(-1, -2))
        off = np.maximum(off, np.abs(local[:, :, 3] - np.array([0.0, 0, 0, 1])).max(axis=-1))
        off = np.where(np.linalg.det(R) > 0, off, np.inf)                       # a reflection is no rotation
        moved = np.abs(t - offsets[None]).max(axis=-1)
        moved[:, roots] = 0.0                                                   # a root has a translation channel
        bad = np.argwhere(~(np.maximum(off, moved) <= RIGID_TOLERANCE))
        if len(bad):
            i, j = (int(x) for x in bad[0])
            raise ValueError(f"write_glb: the local transform of joint {j} in frame {i} is not a rotation about its rest offset "
                             f"within {RIGID_TOLERANCE:g} (off a rotation by {off[i, j]:.3g}, off the offset by {moved[i, j]:.3g})")
        times = accessor((np.arange(n) / float(fps)).astype("<f4"), _FLOAT, "SCALAR", bounds=True)
        samplers, channels = [], []
        for j in range(J):
            q = _quaternions(R[:, j])
            for i in range(1, n):
                if np.dot(q[i], q[i - 1]) < 0:
                    q[i] = -q[i]
            samplers.append({"input": times, "output": accessor(q.astype("<f4"), _FLOAT, "VEC4"), "interpolation": "LINEAR"})
            channels.append({"sampler": len(samplers) - 1, "target": {"node": j, "path": "rotation"}})
        for j in roots:
            samplers.append({"input": times, "output": accessor(t[:, j].astype("<f4"), _FLOAT, "VEC3"), "interpolation": "LINEAR"})
            channels.append({"sampler": len(samplers) - 1, "target": {"node": j, "path": "translation"}})
        gltf["animations"] = [{"name": "poses", "samplers": samplers, "channels": channels}]

    _write_container(path, gltf, blob, views, accessors)


def _write_container(path, gltf, blob, views, accessors):
    gltf["buffers"] = [{"byteLength": len(blob)}]
    gltf["bufferViews"], gltf["accessors"] = views, accessors
    text = json.dumps(gltf, separators=(",", ":")).encode("ascii")
    text += b" " * (-len(text) % 4)
    with open(path, "wb") as out:
        out.write(struct.pack("<III", 0x46546C67, 2, 12 + 8 + len(text) + 8 + len(blob)))
        out.write(struct.pack("<II", len(text), 0x4E4F534A))
        out.write(text)
        out.write(struct.pack("<II", len(blob), 0x004E4942))
        out.write(bytes(blob))
