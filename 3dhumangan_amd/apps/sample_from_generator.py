"""Inference app, counterpart of the reference's apps/sample_from_generator.py: seeds -> rotating-camera frames ->
png / gif (mp4 when imageio is installed).  Same CLI flags, same config overrides (:94-99), same seed -> latent
convention (:26-29), angle schedule (:35-43), uint8 conversion (:59-62) and output naming (:140-149).

The SMPL model file and the SHHQ dataset cannot ship, so `--synthetic-conditions` (the default when --dataroot is
absent) drives the generator with the procedural body of `synthetic.py`; `--dataroot DIR --smpl-model PATH.npz` takes each
seed's body from the records of a dataset in the reference's layout (lib/data/datasets.py), as the reference's app does: the items
come in a shuffled order drawn before the first seed is set, the k-th seed takes the k-th of them; with random-init weights (no
`--checkpoint`) it is a plumbing / throughput run.  `--smpl-record PATH.npz` drives it through the real front-end
instead: one SMPL regression record (the keys preprocess_smpl_fix_body reads) with `joints_index`,
`smpl_tpose_vertices`, `faces` and `faces_to_labels`; the camera preprocessor then rasterises the mesh on the device
and the `_smpl` images are its semantics.  `--pose-sequence PATH.npz` (poses [n,J,3] axis-angle, betas,
optionally orig_cam [n,4]) with `--smpl-model PATH.npz` (the arrays of lib/components/smpl.SMPL plus faces,
faces_to_labels, optionally joints_index) poses the body instead of turning the camera: all poses go through the SMPL
forward and smpl_conditions on the device in one batch, and there is one frame per pose -- the camera fixed, or, with
`--n_angles K` given as well, frame i at angle i mod K of the sweep.  `--pose-sequence synthetic` takes the procedural
model and motion of `synthetic.py` (`--n_poses` frames) and needs no file.  `--save mesh` writes the body's surface instead of
images: the iso-surface of the field's density (Map3DGenerator.extract_mesh) for the seed's latent and conditions, before any
camera rotation, as `{seed:03d}_mesh.ply` -- one file per pose, `{seed:03d}_mesh_{i:03d}.ply`, with `--pose-sequence`.
`--mesh_normals` adds per-vertex normals (nx ny nz: the normalised gradient of the density) to those files, `--mesh_color_views K
[--mesh_color_range DEG, default 30]` per-vertex colours as well (red green blue; it implies the normals): K frames panned evenly
over +-DEG, each made as a frame of this app is made (RNGs seeded anew, the latent, the preprocessor, staged_forward -- the view at
angle 0 is the frame the app saves for the seed and pose), carried onto the vertices by geometry_export.colour.  A vertex no
view sees stays at colour 0 (mid grey).  With random-init weights the frames are noise and so are the colours.  `--save avatar`
(with `--pose-sequence`) writes ONE rigged mesh per seed, `{seed:03d}_avatar.glb` (binary glTF 2.0): the surface is extracted at pose
`--avatar_bind_pose` of the sequence, takes the SMPL body's skin weights from its `--avatar_k` nearest body vertices and goes to the
rest pose (Map3DGenerator.extract_avatar); the file holds the rest mesh with normals (colours with `--mesh_color_views`), the skin, the
skeleton and every pose of the sequence as a key of one animation -- a viewer plays the motion without the network.
`--mesh_texture S` (with `--mesh_color_views K`, K >= 1) bakes the same K frames into an S x S texture atlas
(the same stage): the avatar's `.glb` then carries the texture instead of vertex colours, and `--save mesh` writes, beside
each `.ply` (unchanged), a static `.glb` of the same stem with the texture -- the appearance then has the resolution of the frames,
whatever `--mesh_resolution` is.  `--mesh_simplify K` (with `--save mesh` / `--save avatar`) reduces every surface by quadric vertex
clustering on cells of K voxels of the density grid (Map3DGenerator.extract_mesh(simplify=K)) before anything else is computed on it:
fewer triangles of the same shape, and a larger cell of the atlas for each.

    python -m 3dhumangan_amd.apps.sample_from_generator --config MAP3DBN --seeds 1 2 --n_angles 8 --save png
"""
import argparse
import math
import os

import numpy as np
import torch

from .. import checkpoints, configs, synthetic
from ..lib import data as lib_data
from ..lib import generators as lib_generators
from ..lib.components.mesh_io import write_glb, write_ply
from ..lib.generators import geometry_export

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")


def latent_for_seed(seed, latent_dim):
    """Seed -> latent convention of the reference app (:26-29): both RNGs seeded, one N(0,1) row drawn on the app device
    (so a CUDA run consumes the device RNG, as the reference does)."""
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)
    return torch.randn((1, latent_dim), device=device)


def camera_sweep(n_angles, range_h, range_v, back_and_forth):
    """Angle schedule of the reference app (:35-43) as two float32 lists [n_angles]: a linear pan across
    [-range, +range], or (back_and_forth) one period of a (sin, cos) loop."""
    if back_and_forth:
        phase = torch.linspace(-np.pi, np.pi, n_angles)
        return range_h * torch.sin(phase), range_v * torch.cos(phase)
    return torch.linspace(-range_h, range_h, n_angles), torch.linspace(-range_v, range_v, n_angles)


def to_uint8_nhwc(images):
    """[-1, 1] NCHW float -> uint8 NHWC numpy, the reference's conversion (:59-62): *0.5+0.5, *255, clamp, truncate."""
    return (images * 0.5 + 0.5).mul(255).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()


@torch.no_grad()
def generate_frames(generator, preprocessor, config, seed, conditions, n_angles, angle_range_h, angle_range_v, back_and_forth):
    """One frame per camera angle for the latent of `seed` -> (frames, rasterized_semantics), both uint8
    [n_angles,H,W,3].  Same behaviour as the reference's generate_frames (apps/sample_from_generator.py:24-67; pinned by
    tests/test_app.py against frames the reference function produced); the batch-1 conditions are reused per angle
    instead of being replicated n_angles times up front."""
    dev = generator.device
    z = latent_for_seed(seed, config["latent_dim"]).to(dev)
    base = {k: v[:1].to(dev) for k, v in conditions.items()}
    pan, tilt = camera_sweep(n_angles, angle_range_h, angle_range_v, back_and_forth)
    frames, semantics = [], []
    for a_h, a_v in zip(pan.to(dev), tilt.to(dev)):
        frame, sem = _one_frame(generator, preprocessor, config, z, base, a_h, a_v)
        semantics.append(sem)
        frames.append(frame)
    return to_uint8_nhwc(torch.cat(frames).float()), to_uint8_nhwc(torch.cat(semantics).float())


def _one_frame(generator, preprocessor, config, z, base, a_h, a_v):
    """Batch-1 conditions at one camera angle -> (rgbs, semantics with empty pixels white), both clamped to [-1, 1]."""
    a_h, a_v = a_h.reshape(1, 1), a_v.reshape(1, 1)
    view = preprocessor.forward_with_rotation(dict(base), a_h, a_v, torch.zeros_like(a_h), **config)
    sem = view["rasterized_semantics"].clamp(-1, 1)
    sem = torch.where((sem == 0).all(dim=1, keepdim=True), torch.ones_like(sem), sem)      # empty pixels -> white
    return generator.staged_forward(z, view, **config)["rgbs"].clamp(-1, 1), sem


@torch.no_grad()
def generate_pose_frames(generator, preprocessor, config, seed, conditions, pan, tilt):
    """One frame per item of the batched `conditions` (one pose each) for the latent of `seed`; frame i is seen from
    (pan[i % len(pan)], tilt[i % len(pan)]).  -> (frames, rasterized_semantics), both uint8 [n_poses,H,W,3].  The RNGs are seeded
    anew for every frame, so each frame draws the same latent and the same ray jitter: two frames differ through their pose and
    camera alone, and a repeated pose gives the same frame."""
    dev = generator.device
    pan, tilt = pan.to(dev), tilt.to(dev)
    cached = getattr(generator, "cached_avg_latent", None)
    if cached is not None and config.get("cache_avg_latent") and config.get("truncation_psi", 1.0) < 1.0 and cached() is None:
        latent_for_seed(seed, config["latent_dim"])         # the truncation mean, drawn where the first frame of a sweep draws it,
        generator.generate_avg_latent()                     # but ahead of the frames: no frame's jitter may depend on being first
    frames, semantics = [], []
    for i in range(conditions["scales"].shape[0]):
        z = latent_for_seed(seed, config["latent_dim"]).to(dev)
        base = {k: v[i:i + 1].to(dev) for k, v in conditions.items()}
        frame, sem = _one_frame(generator, preprocessor, config, z, base, pan[i % len(pan)], tilt[i % len(pan)])
        semantics.append(sem)
        frames.append(frame)
    return to_uint8_nhwc(torch.cat(frames).float()), to_uint8_nhwc(torch.cat(semantics).float())


def load_pose_sequence(model_path, sequence_path, dev, n_synthetic=8, return_skeleton=False):
    """--smpl-model / --pose-sequence: -> (conditions of every pose of the sequence, batched on `dev`, a CameraPreprocessor on
    `dev` with the model's faces and labels).  One SMPL forward and one smpl_conditions call for the whole sequence.
    return_skeleton: a third entry, dict(rest_joints [n,J,3]: the joints of each frame's shaped body at rest, parents [J])."""
    from ..lib.components import smpl as smpl_ops
    if sequence_path == "synthetic" and model_path is None:
        model = synthetic.make_smpl_model()
    elif model_path is None:
        raise ValueError("--pose-sequence PATH.npz needs --smpl-model PATH.npz (only `--pose-sequence synthetic` brings its own)")
    else:
        model = dict(np.load(model_path))
    n_joints = np.asarray(model["parents"]).reshape(-1).shape[0]
    seq = synthetic.make_pose_sequence(n_synthetic) if sequence_path == "synthetic" else dict(np.load(sequence_path))
    poses = torch.as_tensor(seq["poses"]).float().reshape(-1, n_joints, 3).to(dev)
    n = poses.shape[0]
    betas = torch.as_tensor(seq["betas"]).float().reshape(-1, np.asarray(model["shapedirs"]).shape[2]).to(dev)
    cam = torch.as_tensor(seq["orig_cam"]).float().reshape(-1, 4) if "orig_cam" in seq else torch.tensor([[1.6, 1.6, 0.0, 0.0]])
    body = smpl_ops.SMPL({k: model[k] for k in smpl_ops.MODEL_KEYS}, device=dev)
    out = body.forward(betas, poses[:, 1:].reshape(n, -1), poses[:, 0])
    joints_index = model["joints_index"].tolist() if "joints_index" in model else list(range(n_joints))
    cond = lib_data.smpl_conditions(out, cam.expand(n, 4) if cam.shape[0] == 1 else cam, joints_index, model["v_template"])
    pre = lib_data.CameraPreprocessor(dev)
    pre.init_smpl(torch.as_tensor(model["faces"]), torch.as_tensor(model["faces_to_labels"]))
    if return_skeleton:
        return cond, pre, {"rest_joints": out["joints_shaped"], "parents": np.asarray(model["parents"]).reshape(-1).astype(np.int64)}
    return cond, pre


def load_smpl_record(path, dev):
    """--smpl-record: -> (batch-1 conditions on `dev`, a CameraPreprocessor on `dev` with the record's faces and labels)."""
    rec = dict(np.load(path))
    cond = lib_data.preprocess_smpl_fix_body(rec, rec["joints_index"].tolist(), rec["smpl_tpose_vertices"])
    cond = {k: v[None].to(dev) for k, v in cond.items()}
    cond["scales"] = cond["scales"].reshape(1)
    pre = lib_data.CameraPreprocessor(dev)
    pre.init_smpl(torch.as_tensor(rec["faces"]), torch.as_tensor(rec["faces_to_labels"]))
    return cond, pre


@torch.no_grad()
def generate_meshes(generator, config, seed, conditions, resolution, level=None, simplify=None):
    """The surface of every item of the batched `conditions` for the latent of `seed` -> list of (vertices, faces).  The RNGs are
    seeded anew per item, as generate_pose_frames does per frame: a mesh belongs to the frame of the same seed and pose.
    simplify: Map3DGenerator.extract_mesh's (the cluster cell in voxels, None: off)."""
    dev = generator.device
    meshes = []
    for i in range(conditions["vertices"].shape[0]):
        z = latent_for_seed(seed, config["latent_dim"]).to(dev)
        body = {k: conditions[k][i:i + 1].to(dev) for k in generator.MESH_CONDITIONS}
        meshes += generator.extract_mesh(z, body, level=level, resolution=resolution, simplify=simplify, **config)
    return meshes


@torch.no_grad()
def generate_textured_meshes(generator, preprocessor, config, seed, conditions, resolution, level=None, n_views=0, view_range=30.0,
                             avatar_k=None, texture_size=0, simplify=None):
    """generate_meshes with normals and, for n_views > 0, colours -> list of dict(vertices, faces, normals, colors, coverage).
    avatar_k: the meshes come from Map3DGenerator.extract_avatar(k=avatar_k) and carry its rig entries as well.
    The colours come from `n_views` frames panned evenly over +-view_range degrees (one view: angle 0), each made as
    generate_pose_frames makes a frame -- RNGs seeded anew, the latent drawn, the conditions turned by the preprocessor, staged_forward
    -- so the view at angle 0 is the frame the app saves for this seed and pose.  texture_size > 0 (with views): the dicts carry
    uvs, texture and texture_coverage as well, baked from the same frames.  simplify: as in generate_meshes; normals, rig, colours
    and texture belong to the simplified mesh."""
    dev = generator.device
    pan = torch.linspace(-math.radians(view_range), math.radians(view_range), n_views) if n_views > 1 else torch.zeros(n_views)
    method, rig = ("extract_textured_mesh", {}) if avatar_k is None else ("extract_avatar", {"k": avatar_k})
    look = geometry_export.settings(method, config, n_views, level, texture_size=n_views and texture_size or None, simplify=simplify)
    meshes = []
    for i in range(conditions["vertices"].shape[0]):
        z = latent_for_seed(seed, config["latent_dim"]).to(dev)
        base = {k: v[i:i + 1].to(dev) for k, v in conditions.items()}
        base["scales"] = base["scales"].reshape(1)
        body = {k: base[k] for k in generator.MESH_CONDITIONS}
        mesh, = getattr(generator, method)(z, body, views=[], level=level, resolution=resolution, simplify=simplify, **rig, **config)
        views, frames = [], []                              # the app's own, after the geometry: the RNGs are seeded anew per view
        for a_h in pan.to(dev):
            z = latent_for_seed(seed, config["latent_dim"]).to(dev)
            a_h = a_h.reshape(1, 1)
            views.append(preprocessor.forward_with_rotation(dict(base), a_h, torch.zeros_like(a_h), torch.zeros_like(a_h), **config))
            frames.append(geometry_export.view_frame(generator, z, views[-1], config))
        if views:
            geometry_export.colour([mesh], views, frames, look.depth_tolerance, look.normal_power, look.texture_size)
        meshes.append(mesh)
    return meshes


def _save(path_stem, frames, mode):
    from PIL import Image
    if mode == "png":
        Image.fromarray(np.concatenate(list(frames), axis=1)).save(path_stem + ".png")
    elif mode == "gif":
        ims = [Image.fromarray(f) for f in frames]
        ims[0].save(path_stem + ".gif", save_all=True, append_images=ims[1:], duration=100, loop=0)
    elif mode == "mp4":
        try:
            import imageio
        except ImportError as e:
            raise RuntimeError("--save mp4 needs imageio (not installed); use --save gif or png") from e
        imageio.mimwrite(path_stem + ".mp4", frames, fps=20, quality=9)
    else:
        raise NotImplementedError


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, default="MAP3DBN")
    ap.add_argument("--tune", type=str, default="")
    ap.add_argument("--variant", type=int, default=0)
    ap.add_argument("--checkpoint", type=str, help="a *_state_dict.pth file or the trainer's pickled <step>_generator.pth")
    ap.add_argument("--ema", type=str, default=None, help="the trainer's pickled <step>_ema.pth: its shadow parameters "
                    "replace the trainable parameters (what the reference evaluates with)")
    ap.add_argument("--seeds", nargs="+", type=int, default=list(range(1, 10)))
    ap.add_argument("--dataroot", type=str, default=None)
    ap.add_argument("--dataset_length", type=int, default=10)
    ap.add_argument("--output_dir", type=str, default="results/sample_from_generator")
    ap.add_argument("--postfix", type=str, default="")
    ap.add_argument("--lock_view_dependence", default=None)
    ap.add_argument("--n_angles", type=int, default=None, help="camera angles of the sweep (default 40)")
    ap.add_argument("--back_and_forth", default=False, action="store_true")
    ap.add_argument("--save", type=str, default="png", choices=["mp4", "png", "gif", "mesh", "avatar"])
    ap.add_argument("--mesh_resolution", type=int, default=256, help="--save mesh: grid nodes along the body box's longest axis")
    ap.add_argument("--mesh_level", type=float, default=None, help="--save mesh: the density of the surface (default: the "
                    "density at which one integration step of the render is half opaque)")
    ap.add_argument("--mesh_normals", default=False, action="store_true", help="--save mesh: write per-vertex normals (the "
                    "normalised gradient of the density) as nx ny nz")
    ap.add_argument("--mesh_color_views", type=int, default=0, help="--save mesh: colour the vertices from this many frames "
                    "panned evenly over +-mesh_color_range (red green blue; implies --mesh_normals)")
    ap.add_argument("--mesh_color_range", type=float, default=30.0, help="--mesh_color_views: half-width of the pan in degrees")
    ap.add_argument("--mesh_texture", type=int, default=0, help="--save mesh / avatar: bake the --mesh_color_views frames into a "
                    "texture atlas of this many texels a side, written into the .glb (0: none)")
    ap.add_argument("--mesh_simplify", type=float, default=0.0, help="--save mesh / avatar: reduce the surface by quadric vertex "
                    "clustering on cells of this many voxels of the density grid (0: off)")
    ap.add_argument("--avatar_k", type=int, default=4, help="--save avatar: body vertices (1..8) whose skin weights a mesh vertex blends")
    ap.add_argument("--avatar_bind_pose", type=int, default=0, help="--save avatar: the pose of the sequence at which the mesh is "
                    "extracted and bound; every pose becomes a key of the file's animation")
    ap.add_argument("--stitch", default=False, action="store_true")
    ap.add_argument("--synthetic-conditions", action="store_true", default=True)
    ap.add_argument("--smpl-record", type=str, default=None, help="an .npz SMPL record (+ joints_index, smpl_tpose_vertices, "
                    "faces, faces_to_labels): conditions and the _smpl images through the front-end and its rasteriser")
    ap.add_argument("--smpl-model", type=str, default=None, help="an .npz SMPL model (v_template, shapedirs, posedirs, "
                    "J_regressor, parents, lbs_weights, faces, faces_to_labels): the body that --pose-sequence poses")
    ap.add_argument("--pose-sequence", type=str, default=None, help="an .npz pose sequence (poses [n,J,3], betas, orig_cam) or "
                    "`synthetic`: one frame per pose; the camera is fixed unless --n_angles is given as well")
    ap.add_argument("--n_poses", type=int, default=8, help="frames of the procedural motion of `--pose-sequence synthetic`")
    return ap


def main(argv=None):
    parser = build_parser()
    opt = parser.parse_args(argv)
    if opt.mesh_texture < 0:
        parser.error(f"--mesh_texture {opt.mesh_texture}: the texture's edge in texels, 0 for none")
    if opt.mesh_texture and opt.mesh_color_views < 1:
        parser.error("--mesh_texture needs the frames it is baked from: pass --mesh_color_views K with K >= 1")
    if opt.mesh_texture and opt.save not in ("mesh", "avatar"):
        parser.error("--mesh_texture goes with --save mesh or --save avatar")
    if not 0.0 <= opt.mesh_simplify < math.inf:
        parser.error(f"--mesh_simplify {opt.mesh_simplify}: the cluster cell in voxels, 0 for off")
    if opt.mesh_simplify and opt.save not in ("mesh", "avatar"):
        parser.error("--mesh_simplify goes with --save mesh or --save avatar")
    simplify = opt.mesh_simplify or None
    sweep_given = opt.n_angles is not None
    if opt.n_angles is None:
        opt.n_angles = 40
    if opt.smpl_model is not None and opt.pose_sequence is None and opt.dataroot is None:
        raise ValueError("--smpl-model goes with --pose-sequence or --dataroot")
    if sum(x is not None for x in (opt.pose_sequence, opt.smpl_record, opt.dataroot)) > 1:
        raise ValueError("--pose-sequence, --smpl-record and --dataroot are three ways to give the body: pass one")
    if opt.dataroot is not None and opt.smpl_model is None:
        raise ValueError("--dataroot needs --smpl-model PATH.npz: the SMPL model as plain arrays (the licensed file cannot ship)")
    if (opt.mesh_normals or opt.mesh_color_views) and opt.save != "mesh" and not (opt.save == "avatar" and not opt.mesh_normals):
        raise ValueError("--mesh_normals and --mesh_color_views go with --save mesh")
    if opt.save == "avatar" and opt.pose_sequence is None:
        raise ValueError("--save avatar needs the skeleton of the body: pass `--pose-sequence synthetic`, or --pose-sequence PATH.npz "
                         "with --smpl-model PATH.npz")
    if opt.save == "avatar" and not 1 <= opt.avatar_k <= 8:
        raise ValueError(f"--avatar_k {opt.avatar_k}: 1..8 nearest body vertices")
    if opt.mesh_color_views < 0:
        raise ValueError(f"--mesh_color_views {opt.mesh_color_views}: a number of views, 0 for none")
    config = configs.get_config(opt)
    config = {k: v for k, v in config.items() if type(k) is str}
    config["truncation_psi"] = 0.7
    config["v_stddev"] = 0
    config["h_stddev"] = 0
    if opt.lock_view_dependence is not None:
        config["lock_view_dependence"] = opt.lock_view_dependence
    config["last_back"] = config.get("eval_last_back", False)
    config["nerf_noise"] = 0
    config["dataset_length"] = opt.dataset_length
    config["cache_avg_latent"] = True                  # the reference recomputes the 10 000-sample mean per call
    out_dir = os.path.join(opt.output_dir, config["name"] + opt.postfix)
    os.makedirs(out_dir, exist_ok=True)

    generator = getattr(lib_generators, config["generator"])(**config).to(device)
    if opt.checkpoint:
        checkpoints.load_generator(generator, opt.checkpoint, ema_path=opt.ema, map_location=device)
    generator.set_device(device)
    generator.eval()
    preprocessor = synthetic.SyntheticPreprocessor(device)
    if opt.smpl_record is not None:
        record, preprocessor = load_smpl_record(opt.smpl_record, device)
    if opt.dataroot is not None:
        dataset = lib_data.SHHQDataset(**dict(config, dataroot=opt.dataroot, smpl_model=opt.smpl_model, inference=True, condition_only=True))
        preprocessor = lib_data.get_preprocessor(device, opt.smpl_model)
        order = torch.randperm(len(dataset)).tolist()       # the reference's shuffled loader, batch 1: drawn before any seed is set
    if opt.pose_sequence is not None:
        sequence, preprocessor, skeleton = load_pose_sequence(opt.smpl_model, opt.pose_sequence, device, opt.n_poses, return_skeleton=True)
        if opt.save == "avatar" and not 0 <= opt.avatar_bind_pose < sequence["vertices"].shape[0]:
            raise ValueError(f"--avatar_bind_pose {opt.avatar_bind_pose}: the sequence has {sequence['vertices'].shape[0]} poses")
        pan, tilt = camera_sweep(opt.n_angles, math.pi / 6, 0, opt.back_and_forth) if sweep_given else (torch.zeros(1), torch.zeros(1))
    for k, seed in enumerate(opt.seeds):
        if opt.save == "avatar":
            b = opt.avatar_bind_pose
            mesh, = generate_textured_meshes(generator, preprocessor, config, seed, {key: v[b:b + 1] for key, v in sequence.items()},
                                             opt.mesh_resolution, opt.mesh_level, opt.mesh_color_views, opt.mesh_color_range,
                                             avatar_k=opt.avatar_k, texture_size=opt.mesh_texture, simplify=simplify)
            look = dict(uvs=mesh["uvs"], texture=mesh["texture"]) if opt.mesh_texture else dict(colors=mesh["colors"])
            write_glb(os.path.join(out_dir, f"{seed:03d}_avatar.glb"), mesh["rest_vertices"], mesh["faces"], mesh["joints"],
                      mesh["weights"], skeleton["rest_joints"][b], skeleton["parents"], normals=mesh["rest_normals"],
                      frames=sequence["fk_matrices"], fps=20, **look)
            continue
        if opt.save == "mesh":
            if opt.pose_sequence is not None:
                data = sequence
            elif opt.dataroot is not None:
                data = {k: v[None] for k, v in dataset[order[k % len(order)]].items()}
            else:
                data = record if opt.smpl_record is not None else synthetic.make_conditions(1, 6890, seed=seed)
            if opt.mesh_normals or opt.mesh_color_views:
                meshes = generate_textured_meshes(generator, preprocessor, config, seed, data, opt.mesh_resolution, opt.mesh_level,
                                                  opt.mesh_color_views, opt.mesh_color_range, texture_size=opt.mesh_texture,
                                                  simplify=simplify)
            else:
                meshes = [dict(vertices=v, faces=f) for v, f in generate_meshes(generator, config, seed, data, opt.mesh_resolution,
                                                                                opt.mesh_level, simplify)]
            for i, m in enumerate(meshes):
                name = f"{seed:03d}_mesh_{i:03d}.ply" if opt.pose_sequence is not None else f"{seed:03d}_mesh.ply"
                write_ply(os.path.join(out_dir, name), m["vertices"], m["faces"], m.get("normals"), m.get("colors"))
                if opt.mesh_texture:
                    write_glb(os.path.join(out_dir, name[:-4] + ".glb"), m["vertices"], m["faces"], normals=m["normals"], uvs=m["uvs"],
                              texture=m["texture"])
            continue
        if opt.pose_sequence is not None:
            frames, semantics = generate_pose_frames(generator, preprocessor, config, seed, sequence, pan, tilt)
        else:
            if opt.dataroot is not None:
                item = dataset[order[k % len(order)]]
                data = {k: v[None] for k, v in item.items()}
                data["scales"] = data["scales"].reshape(1)
            else:
                data = record if opt.smpl_record is not None else synthetic.make_conditions(1, 6890, seed=seed)
            frames, semantics = generate_frames(generator, preprocessor, config, seed, data, opt.n_angles, math.pi / 6, 0,
                                                opt.back_and_forth)
        if opt.stitch:
            frames = np.stack([np.concatenate([f, s], axis=0) for f, s in zip(frames, semantics)])
        _save(os.path.join(out_dir, f"{seed:03d}_uncond"), frames, opt.save)
        if not opt.stitch:
            _save(os.path.join(out_dir, f"{seed:03d}_smpl"), semantics, opt.save)
    return out_dir


if __name__ == "__main__":
    main()
