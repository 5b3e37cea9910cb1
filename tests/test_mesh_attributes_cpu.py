"""The float64 restatement of the mesh attributes (tests/_mesh_attributes_reference.py) held to what vertex normals and projected
colours must satisfy on scenes with analytic answers -- so that the GPU tests (tests/test_gpu_mesh_attributes.py) compare the
kernels with something that is itself checked -- plus the parts of the feature that need no GPU: the PLY writer with normals and
colours, the refusals of the entry points, and the app's flags."""
import importlib

import numpy as np
import pytest
import torch

import _isosurface_reference as R
import _mesh_attributes_reference as M

iso = importlib.import_module("3dhumangan_amd.lib.components.isosurface")
mesh_color = importlib.import_module("3dhumangan_amd.lib.components.mesh_color")
mesh_io = importlib.import_module("3dhumangan_amd.lib.components.mesh_io")
SHAPE = (13, 21, 34)


# ----------------------------------------------------------------------------------------------------------------- normals
def test_sphere_normals_are_radial():
    """radius - distance, radius 5 voxels: the normal of the restatement at the surface's vertices is radial to within the
    discretisation of the central differences (7.4e-3 at this radius)"""
    centre = [(n - 1) / 2 + o for n, o in zip(SHAPE, (0.13, 0.21, -0.17))]
    volume = R.sphere(SHAPE, 5.0)
    vertices = R.marching_tetrahedra(volume, 0.0)[0]
    normals, gradient = M.vertex_normals(volume, vertices)
    radial = vertices - np.asarray(centre)
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    err = np.abs(normals - radial).max()
    print(f"{len(vertices)} vertices: max |normal - radial| = {err:.2e}")
    assert len(vertices) > 1000 and err < 1e-2
    assert np.allclose(np.linalg.norm(normals, axis=1), 1.0, atol=1e-12)


@pytest.mark.parametrize("spacing", [(1.0, 1.0, 1.0), (0.5, 2.0, 0.25)])
def test_linear_field_gives_the_constant_normal_everywhere(spacing):
    """v = a.x + b: every difference, central or one-sided, is exact, so the gradient is `a` at the border planes and for vertices
    clamped from outside the grid as well"""
    a, origin, spacing = np.array([0.5, -1.25, 2.0]), np.array([-1.0, 2.0, 0.5]), np.asarray(spacing)
    shape = (5, 3, 2)
    grid = np.stack(np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij"), axis=-1)
    volume = (origin + spacing * grid) @ a + 3.0
    top = origin + spacing * (np.array(shape) - 1)
    rng = np.random.default_rng(1)
    inside = origin + rng.uniform(size=(50, 3)) * (top - origin)
    nodes = (origin + spacing * grid).reshape(-1, 3)
    outside = np.concatenate([origin - rng.uniform(0.1, 3, size=(10, 3)), top + rng.uniform(0.1, 3, size=(10, 3)),
                              np.array([[origin[0] - 1, top[1] + 1, 0.5 * (origin[2] + top[2])]])])
    vertices = np.concatenate([inside, nodes, outside])
    normals, gradient = M.vertex_normals(volume, vertices, origin, spacing)
    assert np.allclose(gradient, a, rtol=0, atol=1e-12)
    assert np.allclose(normals, -a / np.linalg.norm(a), rtol=0, atol=1e-12)


def test_zero_gradient_and_non_finite_vertices_give_the_zero_normal():
    normals, gradient = M.vertex_normals(np.full((3, 4, 5), 2.5), np.array([[1.0, 1.5, 2.5], [0.0, 0.0, 0.0]]))
    assert (normals == 0).all() and (gradient == 0).all()
    volume = R.sphere(SHAPE, 5.0)
    vertices = np.array([[3.0, 4.0, 5.0], [np.nan, 4.0, 5.0], [3.0, np.inf, 5.0], [3.0, 4.0, -np.inf]])
    normals, gradient = M.vertex_normals(volume, vertices)
    assert np.isclose(np.linalg.norm(normals[0]), 1.0) and (normals[1:] == 0).all() and (gradient[1:] == 0).all()


def test_the_gradient_is_continuous_across_cell_faces():
    """a vertex on a grid face gets the same value from either side: the cells share the face's nodes"""
    volume = R.smooth_random(SHAPE, 3)
    on_face = np.array([[4.0, 7.3, 11.6], [2.7, 9.0, 20.2], [6.1, 3.4, 17.0]])
    for axis in range(3):
        below, above = on_face.copy(), on_face.copy()
        below[axis, axis] -= 1e-9
        above[axis, axis] += 1e-9
        g = M.vertex_gradient(volume, np.stack([below[axis], on_face[axis], above[axis]]))
        assert np.abs(g[0] - g[1]).max() < 1e-7 and np.abs(g[2] - g[1]).max() < 1e-7


# ----------------------------------------------------------------------------------------------------------------- colours
H_, W_, h_, w_ = 128, 64, 64, 32


def scene(K=3):
    return M.sphere_scene(K, h_, w_, H_, W_)


def scalar_bilinear(plane, x, y):
    """an independent bilinear sample: one point, python scalars"""
    rows, cols = plane.shape
    x, y = min(max(x, 0.0), cols - 1.0), min(max(y, 0.0), rows - 1.0)
    x0, y0 = min(int(np.floor(x)), cols - 2), min(int(np.floor(y)), rows - 2)
    ax, ay = x - x0, y - y0
    return ((plane[y0, x0] * (1 - ax) + plane[y0, x0 + 1] * ax) * (1 - ay) + (plane[y0 + 1, x0] * (1 - ax) + plane[y0 + 1, x0 + 1] * ax) * ay)


def camera_args(s, views=None):
    views = list(range(len(s["focals"]))) if views is None else views
    return tuple(s[k][views] for k in ("images", "depths", "focals", "scales", "cam2world"))


@pytest.mark.parametrize("power", [1, 2, 8])
def test_a_vertex_facing_a_camera_takes_that_image(power):
    """Vertices on the sphere seen by camera 0 alone, at several angles off its axis.  By hand: the projection (pinhole through
    (x, y, focal)), the image's value there in the resize convention, face = (-n.d)^power; the depth map is the analytic one, so
    vis = 1 up to its bilinear interpolation (up to 0.7 rad off the axis the map sags by less than 0.01 over one render pixel, 2 % of
    the tolerance 0.5; nearer the silhouette it sags more and the weight drops, as it should)."""
    s = scene()
    c2w, focal, centre = s["cam2world"][0], s["focals"][0], s["centre"]
    o, to_camera = c2w[:3, 3], (c2w[:3, 3] - s["centre"]) / np.linalg.norm(c2w[:3, 3] - s["centre"])
    for angle, axis in ((0.0, 0), (0.2, 0), (0.5, 1), (-0.7, 1), (0.6, 0)):
        n = np.cos(angle) * to_camera + np.sin(angle) * c2w[:3, axis]
        x = centre + s["radius"] * n
        colors, coverage = M.project_colors(x[None], n[None], *camera_args(s, [0]), 0.5, power, fill=0.25, eps=1e-3)
        p = np.linalg.inv(c2w)[:3] @ np.append(x, 1.0)
        u = (focal * p[0] / p[2] + w_ / h_) / (2 * w_ / h_) * (w_ - 1)
        v = (focal * p[1] / p[2] + 1) / 2 * (h_ - 1)
        assert 1 < u < w_ - 2 and 1 < v < h_ - 2
        d = (x - o) / np.linalg.norm(x - o)
        face = max(0.0, -(n @ d)) ** power
        assert face > 0.01 and abs(coverage[0] - face) < 0.02 * face, (angle, coverage[0], face)
        want = np.array([scalar_bilinear(s["images"][0, c], (u + 0.5) * W_ / w_ - 0.5, (v + 0.5) * H_ / h_ - 0.5) for c in range(3)])
        blend = (coverage[0] * want + 1e-3 * 0.25) / (coverage[0] + 1e-3)
        assert np.abs(colors[0] - blend).max() < 1e-12, (angle, colors[0], blend)


def test_two_cameras_blend_by_their_weights():
    s = scene()
    x, n = M.sphere_points(200, s["centre"], s["radius"], 2)
    colors, coverage = M.project_colors(x, n, *camera_args(s), 0.5, 2)
    singles = [M.project_colors(x, n, *camera_args(s, [k]), 0.5, 2, eps=1e-3) for k in range(3)]
    total = sum(cov for _, cov in singles)
    numerator = sum(col * (cov + 1e-3)[:, None] for col, cov in singles)
    assert np.allclose(coverage, total, atol=1e-14) and np.allclose(colors, numerator / (total + 1e-3)[:, None], atol=1e-12)
    assert (coverage > 0.5).sum() > 20 and (coverage == 0).sum() > 5


def test_the_far_side_is_not_covered():
    s = scene(1)
    to_camera = (s["cam2world"][0, :3, 3] - s["centre"]) / np.linalg.norm(s["cam2world"][0, :3, 3] - s["centre"])
    x, n = M.sphere_points(300, s["centre"], s["radius"], 3)
    far = n @ to_camera < -0.3
    colors, coverage = M.project_colors(x, n, *camera_args(s), 0.05, 2, fill=-0.5)
    assert far.sum() > 50 and (coverage[far] == 0).all() and np.allclose(colors[far], -0.5, atol=1e-15)
    # the same points with normals turned towards the camera: the depth map holds the near side, 1.2 and more in front of them
    colors, coverage = M.project_colors(x[far], -n[far], *camera_args(s), 0.05, 2, fill=-0.5)
    assert (coverage == 0).all() and np.allclose(colors, -0.5, atol=1e-15)


def test_an_occluder_in_the_depth_map_removes_the_coverage():
    s = scene(1)
    to_camera = (s["cam2world"][0, :3, 3] - s["centre"]) / np.linalg.norm(s["cam2world"][0, :3, 3] - s["centre"])
    x, n = M.sphere_points(300, s["centre"], s["radius"], 4)
    near = n @ to_camera > 0.8
    images, depths, focals, scales, cams = camera_args(s)
    _, open_view = M.project_colors(x[near], n[near], images, depths, focals, scales, cams, 0.05, 2)
    assert near.sum() > 20 and (open_view > 0.1).all()
    _, blocked = M.project_colors(x[near], n[near], images, depths - 1.0, focals, scales, cams, 0.05, 2)      # a surface 1.0 nearer
    assert (blocked == 0).all()
    # the tent: half a tolerance off gives half the weight
    _, half = M.project_colors(x[near], n[near], images, depths - 0.2, focals, scales, cams, 0.4, 2)
    _, full = M.project_colors(x[near], n[near], images, depths, focals, scales, cams, 0.4, 2)
    assert (np.abs(half / full - 0.5) < 0.03).all()


def test_behind_the_camera_and_outside_the_image():
    s = scene(1)
    c2w = s["cam2world"][0]
    o, right, fwd = c2w[:3, 3], c2w[:3, 0], c2w[:3, 2]
    behind = o - 2.0 * fwd
    sideways = o + 3.0 * fwd + 5.0 * right                  # x / z = 5/3: far outside the image's half-width of w/h / focal = 1/3
    just_inside = o + 3.0 * fwd
    x = np.stack([behind, sideways, just_inside])
    n = np.stack([fwd, -(sideways - o) / np.linalg.norm(sideways - o), -fwd])       # all three face the camera origin
    depths = np.full_like(s["depths"], 1.0)
    images, _, focals, scales, cams = camera_args(s)
    for k, point in enumerate(x):                           # the depth map agrees with each point's distance: only ok / edge decide
        _, coverage = M.project_colors(point[None], n[k][None], images, depths * np.linalg.norm(point - o), focals, scales, cams, 0.05, 1)
        assert (coverage[0] == 0) == (k < 2), (k, coverage)
    assert abs(coverage[0] - 1.0) < 1e-12


# ---------------------------------------------------------------------------------------------------------- writer, refusals
def test_ply_round_trip_with_normals_and_colours(tmp_path):
    volume = R.sphere((9, 9, 9), 3.0)
    v, f, _ = R.marching_tetrahedra(volume, 0.0)
    normals, _ = M.vertex_normals(volume, v)
    rng = np.random.default_rng(0)
    colors = rng.uniform(-1.2, 1.2, size=v.shape).astype(np.float32)
    colors[0] = [-1.0, 0.0, 1.0]
    colors[1] = [np.nan, -7.0, 7.0]
    path = str(tmp_path / "attributed.ply")
    mesh_io.write_ply(path, torch.as_tensor(v), torch.as_tensor(f), torch.as_tensor(normals), torch.as_tensor(colors))
    names, rows, faces = M.parse_attributed_ply(path)
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert np.array_equal(np.stack([rows[k] for k in "xyz"], axis=1), v.astype(np.float32))
    assert np.array_equal(np.stack([rows[k] for k in ("nx", "ny", "nz")], axis=1), normals.astype(np.float32))
    app = importlib.import_module("3dhumangan_amd.apps.sample_from_generator")
    want = app.to_uint8_nhwc(torch.as_tensor(np.nan_to_num(colors, nan=-1.0)).T.reshape(1, 3, -1, 1))[0, :, 0, :]
    got = np.stack([rows[k] for k in ("red", "green", "blue")], axis=1)
    assert np.array_equal(got, want) and got[0].tolist() == [0, 127, 255] and got[1].tolist() == [0, 0, 255]
    assert np.array_equal(faces, f)
    # one attribute alone
    mesh_io.write_ply(path, v, f, normals=normals)
    assert M.parse_attributed_ply(path)[0] == ["x", "y", "z", "nx", "ny", "nz"]
    mesh_io.write_ply(path, v, f, colors=colors)
    assert M.parse_attributed_ply(path)[0] == ["x", "y", "z", "red", "green", "blue"]
    with pytest.raises(ValueError, match="normals"):
        mesh_io.write_ply(path, v, f, normals=normals[:-1])
    with pytest.raises(ValueError, match="colors"):
        mesh_io.write_ply(path, v, f, colors=colors[:, :2])


def test_ply_without_attributes_is_the_three_argument_file(tmp_path):
    v, f, _ = R.marching_tetrahedra(R.sphere((9, 9, 9), 3.0), 0.0)
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    mesh_io.write_ply(a, v, f)
    mesh_io.write_ply(b, v, f, normals=None, colors=None)
    assert open(a, "rb").read() == open(b, "rb").read()
    pv, pf = R.parse_ply(a)                                 # and it is the file the plain reader knows
    assert np.array_equal(pv, v.astype(np.float32)) and np.array_equal(pf, f)


def test_vertex_normals_refusals():
    vol, vert = torch.zeros(3, 4, 5), torch.zeros(7, 3)
    with pytest.raises(TypeError, match="vertex_normals: volume"):
        iso.vertex_normals(vol.numpy(), vert)
    with pytest.raises(TypeError, match="vertex_normals: vertices"):
        iso.vertex_normals(vol, vert.numpy())
    with pytest.raises(ValueError, match="vertex_normals: volume must be float32"):
        iso.vertex_normals(vol.double(), vert)
    with pytest.raises(ValueError, match="vertex_normals: volume must be float32"):
        iso.vertex_normals(vol[0], vert)
    with pytest.raises(ValueError, match="at least 2 nodes"):
        iso.vertex_normals(torch.zeros(3, 1, 5), vert)
    with pytest.raises(ValueError, match="vertex_normals: vertices must be float32"):
        iso.vertex_normals(vol, vert.double())
    with pytest.raises(ValueError, match="vertex_normals: vertices must be float32"):
        iso.vertex_normals(vol, torch.zeros(7, 2))
    with pytest.raises(ValueError, match="three numbers"):
        iso.vertex_normals(vol, vert, origin=(0, 0))
    with pytest.raises(ValueError, match="spacing must be positive"):
        iso.vertex_normals(vol, vert, spacing=(1, 0, 1))


def test_project_colors_refusals():
    K, V = 2, 5
    good = dict(vertices=torch.zeros(V, 3), normals=torch.zeros(V, 3), images=torch.zeros(K, 3, 4, 6), depths=torch.zeros(K, 2, 3),
                focals=torch.ones(K), scales=torch.ones(K), cam2world=torch.eye(4).repeat(K, 1, 1), depth_tolerance=0.05)
    bad = [("vertices", torch.zeros(V, 2), "vertices must be float32"), ("normals", torch.zeros(V, 3).double(), "normals must be float32"),
           ("normals", torch.zeros(V + 1, 3), "normals for 5 vertices"), ("images", torch.zeros(K, 4, 4, 6), "images must be float32"),
           ("images", torch.zeros(K, 3, 1, 6), "images must be float32"), ("depths", torch.zeros(K, 1, 3), "depths must be float32"),
           ("depths", torch.zeros(K + 1, 2, 3), "depths has shape"), ("focals", torch.ones(K + 1), "focals has shape"),
           ("scales", torch.ones(1), "scales has shape"), ("cam2world", torch.eye(4).repeat(3, 1, 1), "cam2world has shape"),
           ("cam2world", torch.zeros(K, 3, 4), "cam2world has shape"), ("images", torch.zeros(0, 3, 4, 6), "at least one view"),
           ("depth_tolerance", 0.0, "depth_tolerance=0.0 must be positive"), ("depth_tolerance", -1.0, "must be positive"),
           ("eps", 0.0, "eps=0.0 must be positive"), ("normal_power", 0, "normal_power=0"), ("normal_power", 9, "normal_power=9"),
           ("normal_power", 2.5, "normal_power=2.5")]
    for name, value, message in bad:
        with pytest.raises(ValueError, match=message):
            mesh_color.project_colors(**{**good, name: value})
    with pytest.raises(TypeError, match="project_colors: depths"):
        mesh_color.project_colors(**{**good, "depths": np.zeros((K, 2, 3), dtype=np.float32)})


def test_camera_table_is_the_float64_inverse():
    s = scene(3)
    table = mesh_color.camera_table(torch.as_tensor(s["focals"]), torch.as_tensor(s["cam2world"]))
    assert table.shape == (3, 16) and table.dtype == np.float32
    for k in range(3):
        inverse = np.linalg.inv(s["cam2world"][k])
        assert np.array_equal(table[k, :12], inverse[:3].reshape(-1).astype(np.float32))
        assert np.array_equal(table[k, 12:15], s["cam2world"][k, :3, 3].astype(np.float32)) and table[k, 15] == np.float32(s["focals"][k])


def test_extract_textured_mesh_refusals():
    gens = importlib.import_module("3dhumangan_amd.lib.generators")
    call = gens.Map3DGenerator.extract_textured_mesh
    cfg = dict(ray_start=-1.0, ray_end=1.0, num_steps=8)
    with pytest.raises(NotImplementedError, match="clamp_mode='softplus'"):
        call(None, None, None, [], **dict(cfg, clamp_mode="softplus"))
    for power in (0, 9, 1.5):
        with pytest.raises(ValueError, match="normal_power"):
            call(None, None, None, [], normal_power=power, **cfg)
    with pytest.raises(ValueError, match="depth_tolerance=0.0 must be positive"):
        call(None, None, None, [], depth_tolerance=0.0, **cfg)
    assert gens.Map3DGenerator.default_depth_tolerance(cfg) == 0.5


def test_the_apps_flags():
    app = importlib.import_module("3dhumangan_amd.apps.sample_from_generator")
    opt = app.build_parser().parse_args(["--save", "mesh"])
    assert (opt.mesh_normals, opt.mesh_color_views, opt.mesh_color_range) == (False, 0, 30.0)
    opt = app.build_parser().parse_args(["--save", "mesh", "--mesh_normals", "--mesh_color_views", "8", "--mesh_color_range", "45"])
    assert (opt.mesh_normals, opt.mesh_color_views, opt.mesh_color_range) == (True, 8, 45.0)
    for flags in (["--mesh_color_views", "3"], ["--mesh_normals"], ["--save", "png", "--mesh_color_views", "3"]):
        with pytest.raises(ValueError, match="go with --save mesh"):
            app.main(flags)
    with pytest.raises(ValueError, match="--mesh_color_views -1"):
        app.main(["--save", "mesh", "--mesh_color_views", "-1"])
