"""SMPL-conditioned geometry features (reference: lib/components/smpl.py:210-249) and the SMPL forward itself -- lbs() and
class SMPL (reference: lib/components/smpl.py:11-207) -- HIP-backed."""
import torch

import os

import numpy as np

from ... import _lib

GEO_DIM = 31
# H3D_NN_PRUNE=0: the full scan of the unsorted mesh (h3d_geo_features / h3d_nearest_vertex) instead of the pruned scan of the
# Morton-sorted one (h3d_mesh_sort + h3d_*_sorted): the same indices bit for bit, for A/B measurements
PRUNE = os.environ.get("H3D_NN_PRUNE", "1") != "0"
TILED = os.environ.get("H3D_NN_TILED", "1") != "0"      # compact 8 x 8 x 4 boxes of samples per wave (nearest_vertex(ray_shape=...))


def sort_mesh(vertices):
    """vertices [B,V,3] fp32 (device) -> the workspace of h3d_mesh_sort: per pose the vertices in Morton order with their original
    indices, and the bounding spheres of the chunks of 64.  One launch, one workgroup per pose; None when the mesh is too large
    for the LDS sort (the callers then take the unsorted path)."""
    B, V, _ = vertices.shape
    lib = _lib.load()
    nbytes = lib.h3d_mesh_sort_bytes(B, V)
    vpad = (V + 63) // 64 * 64
    # the sorted search keeps FOUR planes of the mesh in LDS (x, y, z, original index): larger meshes take the full scan (three)
    if nbytes <= 0 or V > 16384 or vpad // 64 > 256 or 4 * (4 * vpad + 24 * 3 + 4) > 160 * 1024:
        return None
    ws = torch.empty(nbytes // 4, device=vertices.device, dtype=torch.float32)
    rc = lib.h3d_mesh_sort(_lib.ptr(vertices), _lib.ptr(ws), B, V, _lib.stream_handle())
    _lib.check(rc, "h3d_mesh_sort")
    return ws


def vertex_inverse_transforms(fk_matrices, lbs_weights):
    """[B,V,16]: per-vertex blended inverse bone transforms (smpl.py:217-218).  Once per pose; a
    [V,24]x[24,16] product per sample, done by the BLAS library on the device."""
    ik = torch.inverse(fk_matrices.float())
    B, J = ik.shape[:2]
    return torch.bmm(lbs_weights.float(), ik.reshape(B, J, 16)).contiguous()


def get_geo_features(points, skeletons, vertices, tpose_vertices, fk_matrices, lbs_weights, legacy_mode=False,
                     vertex_ik=None, return_index=False, out_stride=GEO_DIM):
    """Same arguments and result as the reference function: points [B,N,3] -> [B,N,31].

    ``vertex_ik`` lets a caller that evaluates many point sets for one pose reuse the blended transforms."""
    _lib.need_cuda(points, skeletons, vertices, tpose_vertices, fk_matrices, lbs_weights, vertex_ik)
    B, N, _ = points.shape
    V = vertices.shape[1]
    if vertex_ik is None:
        vertex_ik = vertex_inverse_transforms(fk_matrices, lbs_weights)
    # every converted tensor is bound to a local: ptr() keeps only the address, so a temporary would be freed (and its
    # block reused by the next same-sized temporary) before the kernel launches
    pts = points.contiguous().float()
    sk = skeletons.contiguous().float()
    vt = vertices.contiguous().float()
    tv = tpose_vertices.contiguous().float()
    vertex_ik = vertex_ik.contiguous().float()
    geo = torch.empty((B, N, out_stride), device=pts.device, dtype=torch.float32)
    if out_stride > GEO_DIM:
        geo[..., GEO_DIM:].zero_()
    idx = torch.empty((B, N), device=pts.device, dtype=torch.int32) if return_index else None
    ws = sort_mesh(vt) if PRUNE and B > 0 and N > 0 else None
    if ws is not None:
        rc = _lib.load().h3d_geo_features_sorted(_lib.ptr(pts), _lib.ptr(sk), _lib.ptr(ws), _lib.ptr(tv), _lib.ptr(vertex_ik),
                                                 _lib.ptr(geo), _lib.ptr(idx), B, N, V, out_stride, int(bool(legacy_mode)),
                                                 _lib.stream_handle())
    else:
        rc = _lib.load().h3d_geo_features(_lib.ptr(pts), _lib.ptr(sk), _lib.ptr(vt), _lib.ptr(tv), _lib.ptr(vertex_ik),
                                          _lib.ptr(geo), _lib.ptr(idx), B, N, V, out_stride, int(bool(legacy_mode)),
                                          _lib.stream_handle())
    _lib.check(rc, "h3d_geo_features")
    return (geo, idx) if return_index else geo


def nearest_vertex(points, vertices, ray_shape=None):
    """K = 1 nearest mesh vertex of every point (the search inside get_geo_features; pytorch3d.ops.knn_points at
    lib/components/smpl.py:220 of the reference): points [B,N,3], vertices [B,V,3] -> int32 [B,N].  Feeds the fused render
    kernels that build the geometry features themselves (COORDCONCATSIREN.render_geo).
    ray_shape = (Hr, Wr, S): the points are the samples of a render grid, [B, Hr, Wr, S, 3] flattened (round 5) -- the pruned
    search then works on compact 8 x 8 x 4 boxes of samples (h3d_nearest_vertex_sorted_rays; H3D_NN_TILED=0: the linear
    assignment); the same indices either way."""
    _lib.need_cuda(points, vertices)
    B, N, _ = points.shape
    pts = points.contiguous().float()
    vt = vertices.contiguous().float()
    idx = torch.empty((B, N), device=pts.device, dtype=torch.int32)
    ws = sort_mesh(vt) if PRUNE and B > 0 and N > 0 else None
    if ws is not None and ray_shape is not None and TILED and int(ray_shape[0]) * int(ray_shape[1]) * int(ray_shape[2]) == N:
        rc = _lib.load().h3d_nearest_vertex_sorted_rays(_lib.ptr(pts), _lib.ptr(ws), _lib.ptr(idx), B, int(ray_shape[0]),
                                                        int(ray_shape[1]), int(ray_shape[2]), vt.shape[1], _lib.stream_handle())
    elif ws is not None:
        rc = _lib.load().h3d_nearest_vertex_sorted(_lib.ptr(pts), _lib.ptr(ws), _lib.ptr(idx), B, N, vt.shape[1], _lib.stream_handle())
    else:
        rc = _lib.load().h3d_nearest_vertex(_lib.ptr(pts), _lib.ptr(vt), _lib.ptr(idx), B, N, vt.shape[1], _lib.stream_handle())
    _lib.check(rc, "h3d_nearest_vertex")
    return idx


# --- the SMPL forward (csrc/smpl_lbs.hip) -------------------------------------------------------------------------------------

MODEL_KEYS = ("v_template", "shapedirs", "posedirs", "J_regressor", "parents", "lbs_weights")
MAX_JOINTS = 64


def validate_model(v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights):
    """Shapes of the six model arrays against each other and the kinematic tree; ValueError names what is wrong."""
    shape = lambda x: tuple(int(n) for n in x.shape)                                       # noqa: E731
    V = shape(v_template)[0] if len(shape(v_template)) == 2 else -1
    if V < 1 or shape(v_template) != (V, 3):
        raise ValueError(f"SMPL model: v_template must be [V,3] with V >= 1, got {shape(v_template)}")
    J = shape(J_regressor)[0] if len(shape(J_regressor)) == 2 else -1
    if shape(J_regressor) != (J, V) or not 1 <= J <= MAX_JOINTS:
        raise ValueError(f"SMPL model: J_regressor must be [J,{V}] with 1 <= J <= {MAX_JOINTS}, got {shape(J_regressor)}")
    if len(shape(shapedirs)) != 3 or shape(shapedirs)[:2] != (V, 3):
        raise ValueError(f"SMPL model: shapedirs must be [{V},3,NB], got {shape(shapedirs)}")
    if shape(posedirs) != ((J - 1) * 9, V * 3):
        raise ValueError(f"SMPL model: posedirs must be [(J-1)*9, V*3] = [{(J - 1) * 9},{V * 3}], got {shape(posedirs)}")
    if shape(lbs_weights) != (V, J):
        raise ValueError(f"SMPL model: lbs_weights must be [{V},{J}], got {shape(lbs_weights)}")
    par = [int(p) for p in torch.as_tensor(parents).reshape(-1).tolist()]
    if len(par) != J:
        raise ValueError(f"SMPL model: parents must have {J} entries, got {len(par)}")
    if par[0] != -1:
        raise ValueError(f"SMPL model: parents[0] must be -1 (joint 0 is the root), got {par[0]}")
    for i in range(1, J):
        if not 0 <= par[i] < i:
            raise ValueError(f"SMPL model: parents[{i}] = {par[i]} is not in [0, {i}): joint {i} must follow its parent")
    return V, J, shape(shapedirs)[2]


def fold_joint_regressor(J_regressor, v_template, shapedirs):
    """The joints are linear in betas: J = J_regressor . (v_template + shapedirs . betas) = joint_template + joint_dirs . betas with
    joint_template [J,3] = J_regressor . v_template and joint_dirs [J,3,NB] = J_regressor . shapedirs.  Exact algebra, evaluated
    once per model in float64."""
    reg = J_regressor.double()
    return reg @ v_template.double(), torch.einsum("ji,ikl->jkl", reg, shapedirs.double())


def batch_rodrigues(rot_vecs):
    """smplx's published definition in torch: rot_vecs [N,3] -> [N,3,3]; angle = |aa + 1e-8| (the epsilon on every component), the
    direction divides the raw vector, R = I + sin K + (1 - cos) K K."""
    angle = torch.norm(rot_vecs + 1e-8, dim=1, keepdim=True)
    d = rot_vecs / angle
    zero = torch.zeros_like(d[:, 0])
    K = torch.stack([zero, -d[:, 2], d[:, 1], d[:, 2], zero, -d[:, 0], -d[:, 1], d[:, 0], zero], dim=1).view(-1, 3, 3)
    s, c = torch.sin(angle)[:, None], torch.cos(angle)[:, None]
    return torch.eye(3, dtype=rot_vecs.dtype, device=rot_vecs.device)[None] + s * K + (1 - c) * torch.bmm(K, K)


def _refuse_grad(op, *tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError(f"{op} is not differentiable: an input requires grad; call it under torch.no_grad() or detach the inputs")


def _f32(t):
    return t.detach().contiguous().float()


def skin_vertices(v_in, fk_matrices, lbs_weights, pose_feature=None, posedirs=None, rigid=None, transl=None):
    """h3d_smpl_skin: verts [B,V,3] = sum_j W[v,j] (rigid_b .) A_bj . [v_in + pose_feature_b . posedirs, 1] (+ transl_b).
    v_in [B,V,3], fk_matrices [B,J,4,4], lbs_weights [V,J]; pose_feature [B,(J-1)*9] with posedirs [(J-1)*9, 3V], or neither (no
    pose offsets); rigid [B,4,4] and transl [B,3] optional."""
    _lib.need_cuda(v_in, fk_matrices, lbs_weights, pose_feature, posedirs, rigid, transl)
    _refuse_grad("smpl.skin_vertices", v_in, fk_matrices, lbs_weights, pose_feature, posedirs, rigid, transl)
    B, V, _ = v_in.shape
    J = fk_matrices.shape[1]
    if tuple(fk_matrices.shape) != (B, J, 4, 4) or tuple(lbs_weights.shape) != (V, J):
        raise ValueError(f"skin_vertices: fk_matrices {tuple(fk_matrices.shape)} / lbs_weights {tuple(lbs_weights.shape)} do not "
                         f"fit v_in {tuple(v_in.shape)}")
    if (pose_feature is None) != (posedirs is None):
        raise ValueError("skin_vertices: pose_feature and posedirs go together")
    P = (J - 1) * 9
    if posedirs is not None and (tuple(pose_feature.shape) != (B, P) or tuple(posedirs.shape) != (P, 3 * V)):
        raise ValueError(f"skin_vertices: pose_feature {tuple(pose_feature.shape)} / posedirs {tuple(posedirs.shape)}, expected "
                         f"[{B},{P}] / [{P},{3 * V}]")
    if rigid is not None and tuple(rigid.shape) != (B, 4, 4):
        raise ValueError(f"skin_vertices: rigid must be [{B},4,4], got {tuple(rigid.shape)}")
    if transl is not None and tuple(transl.shape) != (B, 3):
        raise ValueError(f"skin_vertices: transl must be [{B},3], got {tuple(transl.shape)}")
    # bound to locals until the launch: ptr() keeps only the address
    vi, fk, w = _f32(v_in), _lib.aligned16(_f32(fk_matrices)), _f32(lbs_weights)
    pf = None if pose_feature is None else _f32(pose_feature)
    pd = None if posedirs is None else _f32(posedirs)
    rg = None if rigid is None else _f32(rigid)
    tr = None if transl is None else _f32(transl)
    verts = torch.empty((B, V, 3), device=vi.device, dtype=torch.float32)
    rc = _lib.load().h3d_smpl_skin(_lib.ptr(vi), _lib.ptr(pf), _lib.ptr(pd), _lib.ptr(fk), _lib.ptr(rg), _lib.ptr(tr), _lib.ptr(w),
                                   _lib.ptr(verts), B, V, J, _lib.stream_handle())
    _lib.check(rc, "h3d_smpl_skin")
    return verts


def _lbs_launch(betas, pose, v_template, shapedirs, posedirs, joint_template, joint_dirs, parents_i32, lbs_weights, pose2rot, transl):
    """The three launches on validated fp32 model tensors -> (A, v_shaped, verts, J, J_transformed)."""
    V, J, NB = v_template.shape[0], lbs_weights.shape[1], shapedirs.shape[2]
    B = max(betas.shape[0], pose.shape[0])
    be, po = _f32(betas), _f32(pose)
    if be.shape[0] != B:
        if be.shape[0] != 1:
            raise ValueError(f"lbs: betas has batch {be.shape[0]}, pose has batch {po.shape[0]}")
        be = be.expand(B, -1).contiguous()
    if tuple(be.shape) != (B, NB):
        raise ValueError(f"lbs: betas must be [{B},{NB}], got {tuple(betas.shape)}")
    per_joint = 3 if pose2rot else 9
    if po.shape[0] != B or po.numel() != B * J * per_joint:
        raise ValueError(f"lbs: pose must hold [{B},{J}," + ("3]" if pose2rot else "3,3]") + f", got {tuple(pose.shape)}")
    lib, dev, st = _lib.load(), v_template.device, _lib.stream_handle()
    new = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)                       # noqa: E731
    v_shaped, A, joints, posed, feature = new(B, V, 3), new(B, J, 4, 4), new(B, J, 3), new(B, J, 3), new(B, max(J - 1, 1) * 9)
    rc = lib.h3d_smpl_shape(_lib.ptr(be), _lib.ptr(v_template), _lib.ptr(shapedirs), _lib.ptr(v_shaped), B, V, NB, st)
    _lib.check(rc, "h3d_smpl_shape")
    rc = lib.h3d_smpl_pose(_lib.ptr(be), _lib.ptr(po), _lib.ptr(joint_template), _lib.ptr(joint_dirs), _lib.ptr(parents_i32),
                           _lib.ptr(A), _lib.ptr(joints), _lib.ptr(posed), _lib.ptr(feature), B, J, NB, int(bool(pose2rot)), st)
    _lib.check(rc, "h3d_smpl_pose")
    verts = skin_vertices(v_shaped, A, lbs_weights, feature[:, :(J - 1) * 9] if J > 1 else None, posedirs if J > 1 else None,
                          transl=transl)
    return A, v_shaped, verts, joints, posed


def lbs(betas, pose, v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights, pose2rot=True):
    """Same arguments and return tuple as the reference's lbs (lib/components/smpl.py:11-107): betas [B,NB], pose [B,J*3]
    axis-angle (pose2rot) or [B,J,3,3] matrices -> (A [B,J,4,4], v_shaped [B,V,3], verts [B,V,3], J [B,J,3], J_transformed
    [B,J,3]), fp32 on the device.  v_template [V,3], shapedirs [V,3,NB], posedirs [(J-1)*9, V*3], J_regressor [J,V], parents [J],
    lbs_weights [V,J].  Not differentiable.  This form validates the tree and folds the joint regressor on every call; class SMPL
    does both once."""
    tensors = (betas, pose, v_template, shapedirs, posedirs, J_regressor, lbs_weights)
    _lib.need_cuda(*tensors, parents if torch.is_tensor(parents) and parents.is_cuda else None)
    _refuse_grad("smpl.lbs", *tensors)
    validate_model(v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights)
    jt, jd = fold_joint_regressor(J_regressor.detach(), v_template.detach(), shapedirs.detach())
    par = torch.as_tensor(parents).to(device=v_template.device, dtype=torch.int32).contiguous()
    return _lbs_launch(betas, pose, _f32(v_template), _f32(shapedirs), _f32(posedirs), _f32(jt), _f32(jd), par, _f32(lbs_weights),
                       pose2rot, None)


class SMPL:
    """The SMPL body model on the device: forward(betas, body_pose, global_orient) -> the dict of the reference's SMPL.forward
    (lib/components/smpl.py:110-207).

    Built from the six plain arrays of MODEL_KEYS -- as keyword arguments, a dict or the path of an .npz holding them (`weights`
    is accepted for `lbs_weights`, and posedirs also as [V,3,(J-1)*9], which is stored transposed as smplx does).  There is no
    smplx or chumpy dependency, and the licensed SMPL pickle is NOT read here: export its arrays to an .npz with the tools that
    licence gives you.  `vertex_joint_ids`: vertex indices whose posed positions are appended to `joints` (what smplx's
    vertex-joint selector appends)."""

    def __init__(self, model=None, device="cuda", vertex_joint_ids=None, **arrays):
        if isinstance(model, (str, os.PathLike)):
            model = dict(np.load(model))
        model = dict(model or {}, **arrays)
        if "lbs_weights" not in model and "weights" in model:
            model["lbs_weights"] = model["weights"]
        missing = [k for k in MODEL_KEYS if k not in model]
        if missing:
            raise ValueError(f"SMPL model: missing arrays {missing}")
        m = {k: torch.as_tensor(np.asarray(model[k]) if not torch.is_tensor(model[k]) else model[k]).detach().cpu() for k in MODEL_KEYS}
        if m["posedirs"].dim() == 3:
            m["posedirs"] = m["posedirs"].reshape(-1, m["posedirs"].shape[-1]).T
        self.num_vertices, self.num_joints, self.num_betas = validate_model(*(m[k] for k in MODEL_KEYS))
        jt, jd = fold_joint_regressor(m["J_regressor"], m["v_template"], m["shapedirs"])
        self.device = _lib.canonical_device(device)
        put = lambda t: t.to(torch.float32).contiguous().to(self.device)                   # noqa: E731
        self.v_template, self.shapedirs, self.posedirs = put(m["v_template"]), put(m["shapedirs"]), put(m["posedirs"])
        self.J_regressor, self.lbs_weights = put(m["J_regressor"]), put(m["lbs_weights"])
        self.joint_template, self.joint_dirs = put(jt), put(jd)
        self.parents = m["parents"].reshape(-1).long().to(self.device)
        self._parents_i32 = self.parents.to(torch.int32).contiguous()
        self.vertex_joint_ids = None
        if vertex_joint_ids is not None:
            ids = torch.as_tensor(vertex_joint_ids).reshape(-1).long()
            if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.num_vertices):
                raise ValueError(f"SMPL model: vertex_joint_ids must lie in [0, {self.num_vertices})")
            self.vertex_joint_ids = ids.to(self.device)

    def forward(self, betas, body_pose, global_orient, transl=None, pose2rot=True, return_full_pose=False):
        """betas [B or 1, NB]; global_orient [B,3] and body_pose [B,(J-1)*3] axis-angle, or [B,1,3,3] and [B,J-1,3,3] matrices with
        pose2rot=False; transl [B,3] is added to the vertices and joints.  -> fk_matrices [B,J,4,4], tpose_vertices (the shaped
        template) [B,V,3], vertices [B,V,3], joints_shaped [B,J,3], joints [B,J(+extra),3], betas, global_orient, body_pose,
        full_pose (None unless asked for), lbs_weights."""
        _lib.need_cuda(betas, body_pose, global_orient, transl, self.v_template)
        _refuse_grad("SMPL.forward", betas, body_pose, global_orient, transl)
        B = max(betas.shape[0], global_orient.shape[0], body_pose.shape[0])
        if pose2rot:
            full_pose = torch.cat([global_orient.reshape(B, -1), body_pose.reshape(B, -1)], dim=1)
        else:
            full_pose = torch.cat([global_orient.reshape(B, -1, 3, 3), body_pose.reshape(B, -1, 3, 3)], dim=1)
        if betas.shape[0] != B:
            betas = betas.expand(int(B / betas.shape[0]), -1)
        A, v_shaped, verts, joints_shaped, joints = _lbs_launch(
            betas, full_pose, self.v_template, self.shapedirs, self.posedirs, self.joint_template, self.joint_dirs,
            self._parents_i32, self.lbs_weights, pose2rot, transl)
        if transl is not None:
            joints = joints + transl.float().unsqueeze(1)
        if self.vertex_joint_ids is not None:
            joints = torch.cat([joints, verts[:, self.vertex_joint_ids]], dim=1)
        return {"fk_matrices": A, "tpose_vertices": v_shaped, "vertices": verts, "global_orient": global_orient,
                "body_pose": body_pose, "joints_shaped": joints_shaped, "joints": joints, "betas": betas,
                "full_pose": full_pose if return_full_pose else None, "lbs_weights": self.lbs_weights}

    __call__ = forward
