"""A numpy restatement of the two mesh-rig definitions of include/h3d.h (h3d_mesh_bind, h3d_mesh_pose), written from the text, not
from the kernels: whole arrays, joints in a python loop.  Every function takes dtype=: float64 is the reference, float32 runs the SAME
code in the kernels' number format and is the yardstick of their rounding (tests/test_gpu_mesh_rig.py takes its bars from the distance
of the two).  Beside it: the generator of the test rigs and cases (shared by the CPU and the GPU tests, so that the CPU test can hold
every GPU case's bar under its cap), and a small reader / evaluator of binary glTF files."""
import json
import struct

import numpy as np

f32, f64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------- definitions
def _unit(v, dtype):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        length = np.sqrt((v * v).sum(axis=-1))
        usable = np.isfinite(length) & (length > 0)
        return np.where(usable[..., None], v / np.where(usable, length, 1)[..., None], 0).astype(dtype)


def _cofactors(R):
    """cofactor matrices [...,3,3] and determinants (first-row expansion)"""
    a, b, c, d, e, f, g, h, i = (R[..., r, k] for r in range(3) for k in range(3))
    C = np.stack([np.stack([e * i - f * h, f * g - d * i, d * h - e * g], axis=-1),
                  np.stack([c * h - b * i, a * i - c * g, b * g - a * h], axis=-1),
                  np.stack([b * f - c * e, c * d - a * f, a * e - b * d], axis=-1)], axis=-2)
    return C, a * C[..., 0, 0] + b * C[..., 0, 1] + c * C[..., 0, 2]


def neighbours(X, P, K, dtype):
    """the K + 1 vertices of P of smallest squared distance, ordered by (d^2, index) -> (indices [M,K+1], d^2 [M,K+1])"""
    d = X[:, None, :].astype(dtype) - P[None].astype(dtype)
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    order = np.argsort(d2, axis=1, kind="stable")[:, :K + 1]
    return order, np.take_along_axis(d2, order, axis=1)


def blend_weights(X, P, W, K, eps, dtype):
    """steps 1-3: w [M,J] and the neighbour indices [M,K+1]"""
    order, dk = neighbours(X, P, K, dtype)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        inv = dtype(1) / (dk + dtype(eps))
        a = inv[:, :K] - inv[:, K:]
        s = np.zeros(len(X), dtype=dtype)
        for k in range(K):
            s = s + a[:, k]
        bad = ~np.isfinite(s) | (s <= 0)
        a[bad], s[bad] = 1, K
        ahat = a / s[:, None]
    w = np.zeros((len(X), W.shape[1]), dtype=dtype)
    for k in range(K):
        w = w + ahat[:, k:k + 1] * W.astype(dtype)[order[:, k]]
    return w, order


def cut_to_four(w, dtype):
    """step 4: w' [M,J] (at most four non-zero per row), joints [M,4], weights [M,4]"""
    M, J = w.shape
    c = -np.sort(-w, axis=1)[:, 4] if J >= 5 else np.zeros(M, dtype=dtype)
    u = np.maximum(w - c[:, None], 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        total = u.sum(axis=1)
        ok = np.isfinite(total) & (total > 0)
        wp = np.where(ok[:, None], u / np.where(ok, total, 1)[:, None], 0).astype(dtype)
    pad = np.concatenate([wp, np.zeros((M, max(0, 4 - J)), dtype=dtype)], axis=1)
    slots = np.argsort(-pad, axis=1, kind="stable")[:, :4]                     # descending weight, ties by lower joint
    weights = np.take_along_axis(pad, slots, axis=1)
    joints = np.where(weights > 0, slots, 0).astype(np.int32)
    return wp, joints, weights


def bind(X, P, W, A, N=None, K=4, eps=1e-8, dtype=f64):
    """h3d_mesh_bind -> dict(rest_vertices, rest_normals or None, joints, weights, det, dense [M,J] = w', neighbours [M,K+1])"""
    X, A = np.asarray(X, dtype=dtype), np.asarray(A, dtype=dtype)
    w, order = blend_weights(X, np.asarray(P), np.asarray(W), K, eps, dtype)
    wp, joints, weights = cut_to_four(w, dtype)
    T = np.zeros((len(X), 4, 4), dtype=dtype)
    for j in range(A.shape[0]):                                                 # ascending joint
        T = T + wp[:, j, None, None] * A[j]
    R, t = T[:, :3, :3], T[:, :3, 3]
    C, det = _cofactors(R)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rest = (np.swapaxes(C, 1, 2) @ (X - t)[..., None])[..., 0] / det[:, None]
    rest_normals = None
    if N is not None:
        rest_normals = _unit((np.swapaxes(R, 1, 2) @ np.asarray(N, dtype=dtype)[..., None])[..., 0], dtype)
    return {"rest_vertices": rest.astype(dtype), "rest_normals": rest_normals, "joints": joints, "weights": weights, "det": det,
            "dense": wp, "neighbours": order}


def pose(rest_vertices, joints, weights, A, rest_normals=None, dtype=f64):
    """h3d_mesh_pose: A [n,J,4,4] -> (vertices [n,M,3], normals [n,M,3] or None)"""
    x, A, weights = np.asarray(rest_vertices, dtype=dtype), np.asarray(A, dtype=dtype), np.asarray(weights, dtype=dtype)
    joints = np.asarray(joints)
    T = np.zeros((A.shape[0], len(x), 4, 4), dtype=dtype)
    for i in range(4):                                                          # slot order
        T = T + weights[None, :, i, None, None] * A[:, joints[:, i]]
    R, t = T[..., :3, :3], T[..., :3, 3]
    vertices = (R @ x[None, :, :, None])[..., 0] + t
    if rest_normals is None:
        return vertices.astype(dtype), None
    C, det = _cofactors(R)
    n = np.where(det < 0, -1, 1)[..., None] * (C @ np.asarray(rest_normals, dtype=dtype)[None, :, :, None])[..., 0]
    return vertices.astype(dtype), _unit(n, dtype)


def dense_weights(joints, weights, J):
    dense = np.zeros((len(joints), J), dtype=np.asarray(weights).dtype)
    np.add.at(dense, (np.arange(len(joints))[:, None], np.asarray(joints)), weights)
    return dense


# ------------------------------------------------------------------------------------------------------------- test rigs
def rodrigues(aa):
    angle = np.linalg.norm(aa, axis=-1, keepdims=True)
    d = aa / np.where(angle > 0, angle, 1)
    K = np.zeros(aa.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -d[..., 2], d[..., 1], d[..., 2], -d[..., 0], -d[..., 1], d[..., 0]
    s, c = np.sin(angle)[..., None], np.cos(angle)[..., None]
    return np.eye(3) + s * K + (1 - c) * (K @ K)


def forward_kinematics(rotations, rest_joints, parents, root_translation=None):
    """rotations [n,J,3,3], rest joints [J,3] -> bone transforms A [n,J,4,4] (rest -> posed), float64"""
    n, J = rotations.shape[:2]
    G = np.zeros((n, J, 4, 4))
    for j, p in enumerate(parents):
        L = np.tile(np.eye(4), (n, 1, 1))
        L[:, :3, :3] = rotations[:, j]
        L[:, :3, 3] = rest_joints[j] - (rest_joints[p] if p >= 0 else 0)
        if p < 0 and root_translation is not None:
            L[:, :3, 3] += root_translation
        G[:, j] = L if p < 0 else G[:, p] @ L
    undo = np.tile(np.eye(4), (J, 1, 1))
    undo[:, :3, 3] = -rest_joints
    return G @ undo[None]


def make_rig(V, J, seed, n_poses=1, angle=0.4):
    """An SMPL-like body: a random tree of J joints, V rest vertices scattered around the joints with min(4, J) non-zero skin
    weights each (the nearest joints), n_poses poses with joint rotations up to `angle` rad.  -> dict(parents, rest_joints [J,3],
    rest [V,3], W [V,J] fp32, A [n,J,4,4] fp32, P [n,V,3] fp32: the body posed by float64 skinning)"""
    rng = np.random.default_rng(seed)
    parents = [-1] + [int(rng.integers(max(0, j - 3), j)) for j in range(1, J)]
    rest_joints = np.zeros((J, 3))
    for j in range(1, J):
        step = rng.normal(size=3)
        rest_joints[j] = rest_joints[parents[j]] + 0.25 * step / np.linalg.norm(step)
    owner = rng.integers(J, size=V)
    rest = rest_joints[owner] + 0.08 * rng.normal(size=(V, 3))
    near = np.argsort(((rest[:, None] - rest_joints[None]) ** 2).sum(-1), axis=1, kind="stable")[:, :min(4, J)]
    W = np.zeros((V, J))
    np.put_along_axis(W, near, rng.dirichlet(np.ones(near.shape[1]) * 2.0, size=V), axis=1)
    W = W.astype(f32)
    axis = rng.normal(size=(n_poses, J, 3))
    aa = axis / np.linalg.norm(axis, axis=-1, keepdims=True) * rng.uniform(0, angle, size=(n_poses, J, 1))
    A = forward_kinematics(rodrigues(aa), rest_joints, parents, rng.normal(size=(n_poses, 3)) * 0.1).astype(f32)
    T = np.einsum("vj,njab->nvab", W.astype(f64), A.astype(f64))
    P = (T[..., :3, :3] @ rest[None, :, :, None])[..., 0] + T[..., :3, 3]
    return {"parents": parents, "rest_joints": rest_joints, "rest": rest, "W": W, "A": A, "P": P.astype(f32)}


def depth_of(parents):
    """joints on the longest chain from a root"""
    depth = []
    for p in parents:
        depth.append(1 if p < 0 else depth[p] + 1)
    return max(depth)


def min_spacing(P):
    P = P.astype(f64)
    d2 = ((P[:, None] - P[None]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    return float(np.sqrt(d2.min()))


POOL = 257
# (M, V, J, K): M over {1, 63, 64, 65, 257, 4099}, V over {K + 1, 97, 6890}, J over {1, 4, 5, 24, 64}, K over {1, 4, 8}
CASES = [(1, 97, 24, 4), (63, 97, 24, 4), (64, 97, 5, 4), (65, 97, 4, 4), (257, 97, 1, 4), (4099, 97, 24, 4), (257, 6890, 24, 4),
         (257, 6890, 24, 8), (257, 2, 24, 1), (65, 5, 64, 4), (257, 9, 5, 8), (257, 97, 64, 8), (4099, 97, 24, 1), (257, 97, 24, 1)]


def make_case(M, V, J, K, n_poses=1):
    """-> the rig of make_rig plus X [max(M, POOL), 3] fp32 and unit normals N: SMPL vertices of pose 0 plus noise; rows 1 and 2 are
    specials -- a point exactly on a vertex (d = 0) and the midpoint of a vertex and its nearest neighbour.  K = 1 is decided by
    construction: the offsets are at most 1/8 of the smallest vertex spacing.  The kernel gets the first M rows, the pool the bar."""
    rig = make_rig(V, J, seed=1000 * K + 10 * J + V % 7 + M, n_poses=n_poses)
    rng = np.random.default_rng(M + V + J + K)
    n, P = max(M, POOL), rig["P"][0]
    pick = rng.integers(V, size=n)
    if K == 1:
        offset = rng.normal(size=(n, 3))
        offset *= (min_spacing(P) / 8 * rng.uniform(0, 1, size=(n, 1))) / np.linalg.norm(offset, axis=1, keepdims=True)
    else:
        offset = 0.02 * rng.normal(size=(n, 3))
    X = (P[pick].astype(f64) + offset).astype(f32)
    if K > 1:
        X[1] = P[pick[1]]
        other = np.argsort(((P.astype(f64) - P[pick[2]].astype(f64)) ** 2).sum(-1), kind="stable")[1]
        X[2] = ((P[pick[2]].astype(f64) + P[other].astype(f64)) / 2).astype(f32)
    N = rng.normal(size=(n, 3))
    rig.update(X=X, N=(N / np.linalg.norm(N, axis=1, keepdims=True)).astype(f32), M=M, K=K)
    return rig


def bar_of(low, high):
    """8 x the distance of the float32 and the float64 restatement, not less than 4 ulp of the largest float64 output"""
    return max(8.0 * float(np.abs(low.astype(f64) - high).max()), 4.0 * 2.0 ** -23 * float(np.abs(high).max()))


def case_bars(case, eps=1e-8):
    """-> (float64 restatement of the pool, bars of dense weights, rest positions, rest normals, det)"""
    hi = bind(case["X"], case["P"][0], case["W"], case["A"][0], case["N"], case["K"], eps, f64)
    lo = bind(case["X"], case["P"][0], case["W"], case["A"][0], case["N"], case["K"], eps, f32)
    return hi, {k: bar_of(lo[k], hi[k]) for k in ("dense", "rest_vertices", "rest_normals", "det")}


def lattice_case(K, J=6, seed=0):
    """Exact degeneracy: 8 x 8 x 7 vertices on a half-integer lattice (index (ix 8 + iy) 7 + iz), points at the 294 cell centres --
    every distance is exact in fp32 and the 8 corners of a cell tie at 3/16.  Each vertex has two non-zero weights out of J joints."""
    rng = np.random.default_rng(seed)
    ix, iy, iz = np.meshgrid(np.arange(8), np.arange(8), np.arange(7), indexing="ij")
    P = (np.stack([ix, iy, iz], axis=-1).reshape(-1, 3) * 0.5).astype(f32)
    cx, cy, cz = np.meshgrid(np.arange(7), np.arange(7), np.arange(6), indexing="ij")
    cells = np.stack([cx, cy, cz], axis=-1).reshape(-1, 3)
    X = (cells * 0.5 + 0.25).astype(f32)
    corners = np.stack([((cells[:, 0] + a) * 8 + cells[:, 1] + b) * 7 + cells[:, 2] + c for a in (0, 1) for b in (0, 1) for c in (0, 1)], axis=1)
    W = np.zeros((len(P), J), dtype=f32)
    first = rng.integers(J, size=len(P))
    second = (first + rng.integers(1, J, size=len(P))) % J
    share = rng.uniform(0.1, 0.9, size=len(P))
    W[np.arange(len(P)), first], W[np.arange(len(P)), second] = share, 1 - share
    rig = make_rig(8, J, seed=seed + 50)
    return {"X": X, "P": P, "W": W, "A": rig["A"], "K": K, "corners": np.sort(corners, axis=1)}


def decided_rows(w):
    """rows of blended weights w [M,J] whose set of kept joints no rounding can change: the fourth largest is the fifth by more than
    1e-3 apart, or is exactly zero (fewer than four joints carry weight)"""
    if w.shape[1] < 5:
        return np.ones(len(w), dtype=bool)
    ranked = -np.sort(-w, axis=1)
    return (ranked[:, 3] - ranked[:, 4] > 1e-3) | (ranked[:, 3] == 0)


# ------------------------------------------------------------------------------------------------------------- binary glTF
_COMPONENT = {5120: "i1", 5121: "u1", 5122: "<i2", 5123: "<u2", 5125: "<u4", 5126: "<f4"}
_WIDTH = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}


class Glb:
    """Parses the container (asserting its layout: magic, version, lengths, 4-byte alignment of chunks, views and accessors) and
    evaluates the skin at a key of the first animation, in float64."""

    def __init__(self, path):
        raw = open(path, "rb").read()
        magic, version, total = struct.unpack_from("<III", raw, 0)
        assert magic == 0x46546C67 and version == 2 and total == len(raw) and total % 4 == 0, (magic, version, total, len(raw))
        n_json, kind = struct.unpack_from("<II", raw, 12)
        assert kind == 0x4E4F534A and n_json % 4 == 0
        self.json = json.loads(raw[20:20 + n_json].decode("ascii"))
        n_bin, kind = struct.unpack_from("<II", raw, 20 + n_json)
        assert kind == 0x004E4942 and n_bin % 4 == 0 and 28 + n_json + n_bin == total
        self.bin = raw[28 + n_json:]
        assert self.json["buffers"] == [{"byteLength": n_bin}] or self.json["buffers"][0]["byteLength"] <= n_bin
        for view in self.json["bufferViews"]:
            assert view["byteOffset"] % 4 == 0 and view["byteOffset"] + view["byteLength"] <= n_bin

    def accessor(self, index):
        acc = self.json["accessors"][index]
        view = self.json["bufferViews"][acc["bufferView"]]
        dtype, width = np.dtype(_COMPONENT[acc["componentType"]]), _WIDTH[acc["type"]]
        assert "byteStride" not in view and acc.get("byteOffset", 0) == 0
        assert acc["count"] * width * dtype.itemsize <= view["byteLength"]
        a = np.frombuffer(self.bin, dtype=dtype, count=acc["count"] * width, offset=view["byteOffset"])
        return a.reshape(acc["count"], width) if width > 1 else a

    def attribute(self, name):
        return self.accessor(self.json["meshes"][0]["primitives"][0]["attributes"][name])

    def faces(self):
        return self.accessor(self.json["meshes"][0]["primitives"][0]["indices"]).reshape(-1, 3)

    def keys(self):
        anim = self.json["animations"][0]
        return self.accessor(anim["samplers"][0]["input"]).astype(f64)

    def joint_matrices(self, key=None):
        """jointMatrix = global(node) . inverseBind per joint of the skin, float64 [J,4,4]; key=None: the nodes' own TRS (rest)"""
        nodes = self.json["nodes"]
        trs = {i: (np.asarray(nd.get("translation", [0, 0, 0]), dtype=f64), np.asarray(nd.get("rotation", [0, 0, 0, 1]), dtype=f64))
               for i, nd in enumerate(nodes)}
        if key is not None:
            anim = self.json["animations"][0]
            for ch in anim["channels"]:
                value = self.accessor(anim["samplers"][ch["sampler"]]["output"])[key].astype(f64)
                t, q = trs[ch["target"]["node"]]
                trs[ch["target"]["node"]] = (value, q) if ch["target"]["path"] == "translation" else (t, value)
        parent = {c: i for i, nd in enumerate(nodes) for c in nd.get("children", [])}

        def local(i):
            t, (x, y, z, w) = trs[i]
            L = np.eye(4)
            L[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
            L[:3, 3] = t
            return L

        def world(i):
            return local(i) if i not in parent else world(parent[i]) @ local(i)

        skin = self.json["skins"][0]
        inverse_bind = self.accessor(skin["inverseBindMatrices"]).astype(f64).reshape(-1, 4, 4).transpose(0, 2, 1)    # column-major
        return np.stack([world(node) @ inverse_bind[k] for k, node in enumerate(skin["joints"])])

    def skinned(self, key=None):
        """the vertices under the joint matrices at `key`, float64 [M,3]"""
        JM = self.joint_matrices(key)
        x, jt, wt = self.attribute("POSITION").astype(f64), self.attribute("JOINTS_0").astype(np.int64), self.attribute("WEIGHTS_0").astype(f64)
        T = (wt[:, :, None, None] * JM[jt]).sum(axis=1)
        return (T[:, :3, :3] @ x[:, :, None])[..., 0] + T[:, :3, 3]


def evaluator_bar(parents, coordinates):
    """64 . depth . 2^-24 . max(1, max |coordinate|): each local transform stores seven floats rounded to 2^-24 relative; the 64 is
    margin for the order of composition.  A lost joint rotation is of order 0.1."""
    return 64.0 * depth_of(parents) * 2.0 ** -24 * max(1.0, float(np.abs(coordinates).max()))
