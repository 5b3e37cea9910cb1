"""Iso-surface of a density volume as an indexed triangle mesh, on the device (csrc/isosurface.hip; the definition -- ids,
orientation, output order -- is in include/h3d.h).

    marching_tetrahedra(volume, level, origin=(0, 0, 0), spacing=(1, 1, 1)) -> (vertices fp32 [V,3], faces int32 [T,3])

Two launches.  Between them the prefix sums of the per-node vertex counts and the per-cell triangle counts are torch.cumsum, and
their totals (V, T) are read once on the host to size the outputs: the one synchronisation, inherent to a ragged result.
"""
import ctypes as C

import torch

from ... import _lib


def marching_tetrahedra(volume, level, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """volume: fp32 [Nx,Ny,Nz] on the current ROCm device (a non-contiguous view is copied).  A node is inside iff its value is above
    `level`; the normals point towards lower values.  Vertex i lies at origin + spacing * (grid coordinates).  An empty surface
    gives tensors shaped [0,3]."""
    if not torch.is_tensor(volume):
        raise TypeError(f"marching_tetrahedra: volume must be a tensor, got {type(volume).__name__}")
    _lib.need_cuda(volume)
    if volume.dtype != torch.float32 or volume.dim() != 3:
        raise ValueError(f"marching_tetrahedra: volume must be float32 [Nx,Ny,Nz], got {volume.dtype} {tuple(volume.shape)}")
    origin, spacing = [float(v) for v in origin], [float(v) for v in spacing]
    if len(origin) != 3 or len(spacing) != 3:
        raise ValueError("marching_tetrahedra: origin and spacing take three numbers each")
    volume = volume.contiguous()
    Nx, Ny, Nz = volume.shape
    dev, lib, level = volume.device, _lib.load(), float(level)
    # counts behind one leading zero: the inclusive cumsum of the buffer is the exclusive prefix sum, its last element the total
    nodes, cells = Nx * Ny * Nz, max(Nx - 1, 0) * max(Ny - 1, 0) * max(Nz - 1, 0)
    vcount = torch.zeros(nodes + 1, dtype=torch.int32, device=dev)
    tcount = torch.zeros(cells + 1, dtype=torch.int32, device=dev)
    behind_zero = lambda t: C.c_void_p(t.data_ptr() + t.element_size())
    _lib.check(lib.h3d_isosurface_count(_lib.ptr(volume), Nx, Ny, Nz, level, behind_zero(vcount), behind_zero(tcount),
                                        _lib.stream_handle()), "h3d_isosurface_count")
    voff = torch.cumsum(vcount, 0, dtype=torch.int32)           # < 7 Nx Ny Nz < 2^31
    toff = torch.cumsum(tcount, 0)
    V, T = torch.stack([voff[-1].long(), toff[-1]]).tolist()     # the one host read
    vertices = torch.empty(V, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(T, 3, dtype=torch.int32, device=dev)
    if V == 0 or T == 0:
        return vertices[:0], faces[:0]
    _lib.check(lib.h3d_isosurface_emit(_lib.ptr(volume), Nx, Ny, Nz, level, (C.c_float * 3)(*origin), (C.c_float * 3)(*spacing),
                                       _lib.ptr(voff), _lib.ptr(toff), _lib.ptr(vertices), V, _lib.ptr(faces), T,
                                       _lib.stream_handle()), "h3d_isosurface_emit")
    return vertices, faces
