"""Iso-surface of a density volume as an indexed triangle mesh, on the device (csrc/isosurface.hip; the definition -- ids,
orientation, output order -- is in include/h3d.h).

    marching_tetrahedra(volume, level, origin=(0, 0, 0), spacing=(1, 1, 1)) -> (vertices fp32 [V,3], faces int32 [T,3])

Two launches.  Between them the prefix sums of the per-node vertex counts and the per-cell triangle counts are torch.cumsum, and
their totals (V, T) are read once on the host to size the outputs: the one synchronisation, inherent to a ragged result.

    vertex_normals(volume, vertices, origin=(0, 0, 0), spacing=(1, 1, 1), return_gradient=False) -> normals fp32 [V,3]

The normalised gradient of the volume at each vertex (csrc/mesh_attributes.hip, h3d_isosurface_normals): one launch, no host read.
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


def vertex_normals(volume, vertices, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), return_gradient=False):
    """The normal of the density `volume` (fp32 [Nx,Ny,Nz], a non-contiguous view is copied) at each of `vertices` (fp32 [V,3], in the
    frame origin + spacing * grid coordinates) -> normals fp32 [V,3], and the un-normalised gradient fp32 [V,3] when asked.

    The gradient is the trilinear interpolation of the nodes' central differences (one-sided at the border planes), the normal
    -gradient / |gradient|: towards lower values, as marching_tetrahedra orients its faces; (0,0,0) where the gradient is zero or not
    finite, and at a vertex with a non-finite coordinate.  One launch, no synchronisation (include/h3d.h has the definition)."""
    for name, t in (("volume", volume), ("vertices", vertices)):
        if not torch.is_tensor(t):
            raise TypeError(f"vertex_normals: {name} must be a tensor, got {type(t).__name__}")
    if volume.dtype != torch.float32 or volume.dim() != 3:
        raise ValueError(f"vertex_normals: volume must be float32 [Nx,Ny,Nz], got {volume.dtype} {tuple(volume.shape)}")
    if min(volume.shape) < 2:
        raise ValueError(f"vertex_normals: every axis of volume needs at least 2 nodes, got {tuple(volume.shape)}")
    if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"vertex_normals: vertices must be float32 [V,3], got {vertices.dtype} {tuple(vertices.shape)}")
    origin, spacing = [float(v) for v in origin], [float(v) for v in spacing]
    if len(origin) != 3 or len(spacing) != 3:
        raise ValueError("vertex_normals: origin and spacing take three numbers each")
    if not all(0.0 < s < float("inf") for s in spacing):
        raise ValueError(f"vertex_normals: spacing must be positive and finite, got {tuple(spacing)}")
    _lib.need_cuda(volume, vertices)
    V = vertices.shape[0]
    normals = torch.empty(V, 3, dtype=torch.float32, device=vertices.device)
    gradient = torch.empty(V, 3, dtype=torch.float32, device=vertices.device) if return_gradient else None
    if V:
        volume, vertices = volume.contiguous(), vertices.contiguous()
        Nx, Ny, Nz = volume.shape
        _lib.check(_lib.load().h3d_isosurface_normals(_lib.ptr(volume), Nx, Ny, Nz, (C.c_float * 3)(*origin), (C.c_float * 3)(*spacing),
                                                      _lib.ptr(vertices), V, _lib.ptr(normals), _lib.ptr(gradient),
                                                      _lib.stream_handle()), "h3d_isosurface_normals")
    return (normals, gradient) if return_gradient else normals
