"""The rig of an extracted mesh (csrc/mesh_rig.hip; the definitions are in include/h3d.h, h3d_mesh_bind / h3d_mesh_pose).

bind carries the SMPL body's skin onto a surface that was extracted in a pose -- distance-weighted over the K nearest SMPL vertices,
cut to four joints -- and takes the surface to the rest pose by inverting each vertex's blended bone transform; pose puts the rest
mesh into any pose of the same skeleton.  One launch each, no host read, not differentiable."""
import torch

from ... import _lib
from .smpl import MAX_JOINTS, _f32, _refuse_grad

MAX_K = 8


def _shape(t):
    return tuple(int(n) for n in t.shape)


def bind(vertices, smpl_vertices, lbs_weights, fk_matrices, normals=None, k=4, eps=1e-8):
    """vertices [M,3] (posed space), smpl_vertices [V,3] (the posed body), lbs_weights [V,J], fk_matrices [J,4,4] (rest -> posed),
    normals [M,3] unit or None; k in 1..8 neighbours, V >= k + 1, J <= 64 -> dict(rest_vertices [M,3], rest_normals [M,3] or None,
    joints int32 [M,4], weights [M,4] (descending, summing to 1, a zero slot carries joint 0), det [M] (the determinant of each
    vertex's blended transform: near 0 the rest position is not to be trusted))."""
    _lib.need_cuda(vertices, smpl_vertices, lbs_weights, fk_matrices, normals)
    _refuse_grad("mesh_rig.bind", vertices, smpl_vertices, lbs_weights, fk_matrices, normals)
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"bind: vertices must be [M,3], got {_shape(vertices)}")
    if int(k) != k or not 1 <= int(k) <= MAX_K:
        raise ValueError(f"bind: k={k} must be an integer 1..{MAX_K}")
    k, M = int(k), vertices.shape[0]
    if smpl_vertices.dim() != 2 or smpl_vertices.shape[1] != 3:
        raise ValueError(f"bind: smpl_vertices must be [V,3], got {_shape(smpl_vertices)}")
    V = smpl_vertices.shape[0]
    if V < k + 1:
        raise ValueError(f"bind: smpl_vertices has {V} rows, k={k} needs at least {k + 1}")
    if lbs_weights.dim() != 2 or lbs_weights.shape[0] != V or not 1 <= lbs_weights.shape[1] <= MAX_JOINTS:
        raise ValueError(f"bind: lbs_weights must be [{V},J] with 1 <= J <= {MAX_JOINTS}, got {_shape(lbs_weights)}")
    J = lbs_weights.shape[1]
    if _shape(fk_matrices) != (J, 4, 4):
        raise ValueError(f"bind: fk_matrices must be [{J},4,4], got {_shape(fk_matrices)}")
    if normals is not None and _shape(normals) != (M, 3):
        raise ValueError(f"bind: normals must be [{M},3], got {_shape(normals)}")
    if not 0.0 < float(eps) < float("inf"):
        raise ValueError(f"bind: eps={eps} must be positive")
    # bound to locals until the launch: ptr() keeps only the address
    x, p, w, fk = _f32(vertices), _f32(smpl_vertices), _f32(lbs_weights), _f32(fk_matrices)
    nr = None if normals is None else _f32(normals)
    new = lambda *s, dtype=torch.float32: torch.empty(s, device=x.device, dtype=dtype)    # noqa: E731
    rest, joints, weights, det = new(M, 3), new(M, 4, dtype=torch.int32), new(M, 4), new(M)
    rest_normals = None if nr is None else new(M, 3)
    rc = _lib.load().h3d_mesh_bind(_lib.ptr(x), _lib.ptr(nr), M, _lib.ptr(p), _lib.ptr(w), _lib.ptr(fk), V, J, k, float(eps),
                                   _lib.ptr(rest), _lib.ptr(rest_normals), _lib.ptr(joints), _lib.ptr(weights), _lib.ptr(det),
                                   _lib.stream_handle())
    _lib.check(rc, "h3d_mesh_bind")
    return {"rest_vertices": rest, "rest_normals": rest_normals, "joints": joints, "weights": weights, "det": det}


def pose(rest_vertices, joints, weights, fk_matrices, rest_normals=None):
    """rest_vertices [M,3], joints int [M,4], weights [M,4], fk_matrices [n,J,4,4] (n poses), rest_normals [M,3] or None
    -> (vertices [n,M,3], normals [n,M,3] or None)."""
    _lib.need_cuda(rest_vertices, joints, weights, fk_matrices, rest_normals)
    _refuse_grad("mesh_rig.pose", rest_vertices, weights, fk_matrices, rest_normals)
    if rest_vertices.dim() != 2 or rest_vertices.shape[1] != 3:
        raise ValueError(f"pose: rest_vertices must be [M,3], got {_shape(rest_vertices)}")
    M = rest_vertices.shape[0]
    if _shape(joints) != (M, 4) or joints.dtype.is_floating_point:
        raise ValueError(f"pose: joints must be integer [{M},4], got {joints.dtype} {_shape(joints)}")
    if _shape(weights) != (M, 4):
        raise ValueError(f"pose: weights must be [{M},4], got {_shape(weights)}")
    fk = fk_matrices
    if fk.dim() != 4 or _shape(fk)[2:] != (4, 4) or not 1 <= fk.shape[1] <= MAX_JOINTS or fk.shape[0] > 65535:
        raise ValueError(f"pose: fk_matrices must be [n,J,4,4] with 1 <= J <= {MAX_JOINTS} and n <= 65535, got {_shape(fk_matrices)}")
    if rest_normals is not None and _shape(rest_normals) != (M, 3):
        raise ValueError(f"pose: rest_normals must be [{M},3], got {_shape(rest_normals)}")
    n, J = fk.shape[:2]
    xr, jt, wt, fk = _f32(rest_vertices), joints.detach().contiguous().to(torch.int32), _f32(weights), _f32(fk)
    nr = None if rest_normals is None else _f32(rest_normals)
    vertices = torch.empty((n, M, 3), device=xr.device, dtype=torch.float32)
    normals = None if nr is None else torch.empty((n, M, 3), device=xr.device, dtype=torch.float32)
    rc = _lib.load().h3d_mesh_pose(_lib.ptr(xr), _lib.ptr(nr), _lib.ptr(jt), _lib.ptr(wt), M, _lib.ptr(fk), n, J, _lib.ptr(vertices),
                                   _lib.ptr(normals), _lib.stream_handle())
    _lib.check(rc, "h3d_mesh_pose")
    return vertices, normals


def dense_weights(joints, weights, J):
    """joints [M,4], weights [M,4] -> [M,J]: the skin as a dense matrix, what smpl.skin_vertices takes (zero slots add nothing)."""
    if joints.dim() != 2 or joints.shape[1] != 4 or _shape(weights) != _shape(joints):
        raise ValueError(f"dense_weights: joints and weights must both be [M,4], got {_shape(joints)} and {_shape(weights)}")
    dense = torch.zeros((joints.shape[0], int(J)), device=weights.device, dtype=weights.dtype)
    return dense.scatter_add_(1, joints.long(), weights)
