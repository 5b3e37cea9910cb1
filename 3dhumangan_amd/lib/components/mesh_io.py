"""Mesh files.  write_ply: an indexed triangle mesh as binary little-endian PLY (float x y z, then uchar-int face lists)."""
import numpy as np


def _as_array(a, dtype, what):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"write_ply: {what} must be [n,3], got {a.shape}")
    return np.ascontiguousarray(a, dtype=dtype)


def write_ply(path, vertices, faces):
    """vertices [V,3] (floating), faces [T,3] (integer indices into vertices); tensors or arrays."""
    v = _as_array(vertices, "<f4", "vertices")
    f = _as_array(faces, "<i4", "faces")
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"write_ply: face index outside [0, {len(v)})")
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
    rows = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    rows["n"] = 3
    rows["i"] = f
    with open(path, "wb") as out:
        out.write(header.encode("ascii"))
        out.write(v.tobytes())
        out.write(rows.tobytes())
