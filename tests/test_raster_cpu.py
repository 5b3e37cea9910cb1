"""The mesh rasteriser without a GPU: its camera against the generator's, the float64 restatement of its contract
(tests/_raster_reference.py) on hand-checkable cases, and the C entry point's argument checks."""
import ctypes
import importlib
import math

import pytest
import torch

import _raster_reference as RR

synthetic = importlib.import_module("3dhumangan_amd.synthetic")
conditions = importlib.import_module("3dhumangan_amd.lib.data.conditions")
_lib = importlib.import_module("3dhumangan_amd._lib")


def _generator_pixels(verts, cam2world, focal, H, W):
    """Pixel (col, row) where the generator's camera sees `verts` [V,3]: the h3d_ray_setup grid, x over linspace(-W/H, W/H, W),
    y over linspace(-1, 1, H), x = F X / Z in camera space."""
    w2c = torch.inverse(cam2world.double())
    Xc = verts.double() @ w2c[:3, :3].T + w2c[:3, 3]
    x, y = focal * Xc[:, 0] / Xc[:, 2], focal * Xc[:, 1] / Xc[:, 2]
    span = W / H
    return (x + span) / (2 * span) * (W - 1), (y + 1) / 2 * (H - 1)


def _raster_pixels(verts, R, T, H, W):
    x, y, _ = RR.project(verts, R, T, -conditions.FOCAL_RASTER)
    s = min(H, W)
    return (W - s * x - 1) / 2, (H - s * y - 1) / 2


@pytest.mark.parametrize("seed", [0, 3, 7])
@pytest.mark.parametrize("scale", [0.5, 0.8])
def test_raster_camera_is_the_generator_camera(seed, scale):
    """Contract items 1-3 (view, projection, pixel centres) put every vertex where the generator's camera puts it."""
    H, W = 512, 256
    hs = [0.0, 0.5, -1.2, 2.5]
    cond = synthetic.make_conditions(len(hs), seed=seed, scale=scale)
    pre = conditions.CameraPreprocessor()
    z = torch.zeros(len(hs))
    view = pre.forward_with_rotation(cond, torch.tensor(hs), z, z, gen_height=H, gen_width=W)
    T = conditions.raster_translation(view)
    for b in range(len(hs)):
        gc, gr = _generator_pixels(cond["vertices"][b], view["cam2world_matrices"][b], float(cond["intrinsics"][b, 0, 0]), H, W)
        rc, rr = _raster_pixels(cond["vertices"][b], view["raster_rotation"][b], T[b], H, W)
        d = torch.hypot(gc - rc, gr - rr)
        assert float(d.median()) <= 1.0 and float(d.max()) <= 8.0, (hs[b], float(d.median()), float(d.max()))


def test_pixel_centres():
    xs, ys = RR.pixel_centres(4, 2)              # H > W: x spans [-1, 1], y [-2, 2]
    assert torch.allclose(xs, torch.tensor([0.5, -0.5], dtype=torch.float64))
    assert torch.allclose(ys, torch.tensor([1.5, 0.5, -0.5, -1.5], dtype=torch.float64))
    xs, ys = RR.pixel_centres(2, 4)              # W > H
    assert torch.allclose(xs, torch.tensor([1.5, 0.5, -0.5, -1.5], dtype=torch.float64))
    assert torch.allclose(ys, torch.tensor([0.5, -0.5], dtype=torch.float64))


def _camera(B=1, depth=10.0):
    """Identity view at `depth`, focal = -depth: NDC (x, y) = (-X, -Y) for vertices at Z = 0."""
    return torch.eye(3)[None].repeat(B, 1, 1), torch.tensor([[0.0, 0.0, depth]]).repeat(B, 1), -depth


@pytest.mark.parametrize("winding", [(0, 1, 2), (0, 2, 1)])
def test_large_triangle_covers_the_expected_pixels(winding):
    H, W = 24, 20
    # NDC triangle (x, y): right angle at (0.9, 0.9) with legs to (-0.7, 0.9) and (0.9, -0.7): covered iff x + y > 0.2 strictly
    # inside the legs; vertices are given as (-x, -y) because the camera mirrors
    ndc = torch.tensor([[0.9, 0.9], [-0.7, 0.9], [0.9, -0.7]], dtype=torch.float64)
    verts = torch.cat([-ndc, torch.zeros(3, 1, dtype=torch.float64)], 1).float()[None]
    faces = torch.tensor([winding])
    R, T, f = _camera()
    out = RR.rasterize(verts, faces, R, T, f, H, W)
    xs, ys = RR.pixel_centres(H, W)
    X, Y = xs[None, :].expand(H, W), ys[:, None].expand(H, W)
    vx, vy = verts[0, :, 0].double() * -1, verts[0, :, 1].double() * -1     # the float32 corners in NDC
    # the hypotenuse from (vx1, vy1) to (vx2, vy2): inside on the side of the right-angle corner
    side = lambda x, y: (x - vx[1]) * (vy[2] - vy[1]) - (y - vy[1]) * (vx[2] - vx[1])   # noqa: E731
    expect = (X < vx[0]) & (Y < vy[0]) & (side(X, Y) * side(vx[0], vy[0]) > 0)
    assert expect.sum() > 50
    assert torch.equal(out["pix_to_face"][0] == 0, expect)
    assert torch.allclose(out["zbuf"][0][expect], torch.full_like(out["zbuf"][0][expect], 10.0))
    b = out["bary"][0][expect]
    assert torch.allclose(b.sum(-1), torch.ones_like(b[:, 0])) and (b > 0).all()


def test_zero_area_face_is_ignored():
    verts = torch.tensor([[[-0.5, -0.5, 0.0], [0.5, 0.5, 0.0], [0.0, 0.0, 0.0], [0.5, -0.5, 0.0]]])
    faces = torch.tensor([[0, 1, 2], [0, 1, 1]])                  # collinear, then a repeated vertex
    R, T, f = _camera()
    out = RR.rasterize(verts, faces, R, T, f, 16, 16)
    assert (out["pix_to_face"] == -1).all()


def test_nearer_face_wins_and_equal_depth_goes_to_the_lower_index():
    square = torch.tensor([[-0.8, -0.8], [0.8, -0.8], [0.8, 0.8], [-0.8, 0.8]])
    far = torch.cat([square, torch.full((4, 1), 1.0)], 1)          # Z = 11
    near = torch.cat([square, torch.full((4, 1), -1.0)], 1)        # Z = 9
    verts = torch.cat([far, near])[None]
    R, T, f = _camera()
    faces = torch.tensor([[0, 1, 2], [4, 5, 6], [0, 2, 3], [4, 6, 7]])
    out = RR.rasterize(verts, faces, R, T, f, 16, 16)
    hit = out["pix_to_face"][0] >= 0
    assert hit.sum() > 100 and set(out["pix_to_face"][0][hit].tolist()) == {1, 3}
    assert torch.allclose(out["zbuf"][0][hit], torch.full_like(out["zbuf"][0][hit], 9.0))
    # the same triangle twice: the lower index wins everywhere
    faces = torch.tensor([[4, 5, 6], [4, 5, 6], [0, 1, 2]])
    out = RR.rasterize(verts, faces, R, T, f, 16, 16)
    assert set(out["pix_to_face"][0][out["pix_to_face"][0] >= 0].tolist()) == {0}


def test_mesh_raster_rejects_bad_arguments_without_a_gpu():
    build = importlib.import_module("3dhumangan_amd._build")
    lib = ctypes.CDLL(build.build_lib())
    fn = lib.h3d_mesh_rasterize
    fn.restype = ctypes.c_int
    fn.argtypes = _lib._SIGNATURES["h3d_mesh_rasterize"][1]
    lib.h3d_last_error.restype = ctypes.c_char_p
    lib.h3d_mesh_raster_bytes.restype = ctypes.c_int64
    lib.h3d_mesh_raster_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    assert lib.h3d_mesh_raster_bytes(4, 13776) >= 4 * 13776 * 56
    p = ctypes.c_void_p(16)                     # never dereferenced: validation runs before any HIP call

    def call(B=2, H=8, W=8, verts=p):
        return fn(verts, p, p, p, -114.59, None, None, p, None, None, None, None, p, B, 10, 4, H, W, None)

    assert call(verts=None) == -1 and b"null pointer" in lib.h3d_last_error()
    assert call(B=0) == -1 and b"B=0" in lib.h3d_last_error()
    assert call(B=-3) == -1
    assert call(H=0) == -1 and b"image size" in lib.h3d_last_error()
    assert call(W=-1) == -1
    # segments without labels, semantics without a table
    assert fn(p, p, p, p, -1.0, None, None, p, None, None, p, None, p, 1, 10, 4, 8, 8, None) == -1
    assert fn(p, p, p, p, -1.0, None, None, p, None, None, None, p, p, 1, 10, 4, 8, 8, None) == -1


def test_init_smpl_then_forward_on_cpu_raises():
    cond, faces, labels = synthetic.make_mesh_conditions(1)
    pre = conditions.CameraPreprocessor()
    pre.init_smpl(faces, labels)
    z = torch.zeros(1)
    with pytest.raises(_lib.H3DError):
        pre.forward_with_rotation(cond, z, z, z, gen_height=16, gen_width=8)


def test_tube_body_is_smpl_sized():
    J, V, Wt, faces, labels = synthetic.tube_body()
    assert faces.shape == (13776, 3) and V.shape == (6936, 3) and Wt.shape == (6936, 24)
    assert int(faces.min()) == 0 and int(faces.max()) == V.shape[0] - 1
    assert set(labels.tolist()) == set(range(24))
    assert torch.allclose(Wt.sum(1), torch.ones(V.shape[0]), atol=1e-5)
    # closed surface: every edge is shared by exactly two faces
    e = torch.cat([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).sort(1).values
    _, cnt = torch.unique(e, dim=0, return_counts=True)
    assert (cnt == 2).all()
    assert math.isclose(float(V[:, 1].max() - V[:, 1].min()), 1.6, abs_tol=0.3)
