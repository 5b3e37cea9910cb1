"""Mesh files.  write_ply: an indexed triangle mesh as binary little-endian PLY (float x y z, optionally float nx ny nz and uchar red
green blue per vertex, then uchar-int face lists)."""
import numpy as np


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
        c = _as_array(colors, "<f4", "colors")
        with np.errstate(invalid="ignore"):
            fields["rgb"] = np.nan_to_num(np.clip((c * np.float32(0.5) + np.float32(0.5)) * np.float32(255), 0, 255), nan=0.0).astype("u1")
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
