"""Fused render with the feature head applied once per ray (field_x3.hip, RAYHEAD): the head and the compositing are linear, so
the kernel composites the colour layer's activations, parks the ray's hbar in its feature slots and runs Wf over 32 parked rays at
a time (a "flush").  Reference semantics: COORDCONCATSIREN.forward + volume_rendering.ray_integration through the float64 oracle.
Tolerances are the existing ones (TOL of test_gpu_fused_geo.py, FIELD_TOL of test_gpu_field.py)."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import h3d_oracle as O
from conftest import GOLDEN, rel_err
from test_gpu_field import FIELD_TOL, random_state
from test_gpu_fused_geo import TOL, dev_dict

pytestmark = pytest.mark.gpu
smpl = importlib.import_module("3dhumangan_amd.lib.components.smpl")
synthetic = importlib.import_module("3dhumangan_amd.synthetic")
vr = importlib.import_module("3dhumangan_amd.lib.generators.volume_rendering")
h3dlib = importlib.import_module("3dhumangan_amd._lib")
DEV = "cuda"
NAMES = ("feats", "depth", "weights")


def geo_setup(S, R, hidden, feature=None, B=2, V=500, seed=None, engine="f16x2", with_noise=True):
    """The setup of test_render_geo_vs_oracle_and_vs_the_two_kernel_path: -> (state, net, cpu inputs, device call)."""
    feature = hidden if feature is None else feature
    state, net = random_state(hidden, feature, seed=S + hidden if seed is None else seed, precision=engine)
    with torch.no_grad():
        net.sigma_layer.weight.mul_(40.0)
        state["neural_field.sigma_layer.weight"] = net.sigma_layer.weight.detach().cpu().clone()
    N = R * S
    cond = synthetic.make_conditions(B, n_vertices=V, seed=R)
    g = torch.Generator().manual_seed(R)
    pts = torch.rand(B, N, 3, generator=g) * 2 - 1
    freq = torch.randn(B, 4 * hidden, generator=g) * 0.5
    phase = torch.randn(B, 4 * hidden, generator=g)
    z = torch.sort(torch.rand(B, R, S, 1, generator=g) + 11, dim=2).values
    noise = torch.randn(B, R, S, 1, generator=g) * 0.3 if with_noise else None
    c = dev_dict(cond)
    vik = smpl.vertex_inverse_transforms(c["fk_matrices"], c["lbs_weights"])
    idx = smpl.nearest_vertex(pts.to(DEV), c["vertices"])
    dpts, dfreq, dphase, dz = pts.to(DEV), freq.to(DEV), phase.to(DEV), z.to(DEV)
    dnoise = None if noise is None else noise.to(DEV)

    def run(last_back, white_back, precision=None):
        return net.render_geo(dpts, dfreq, dphase, idx, c["skeletons_xyz"], c["vertices"], c["tpose_vertices"], vik, None, dz, S,
                              input_scaler=0.7, noise=dnoise, clamp_mode="relu", last_back=last_back, white_back=white_back,
                              precision=precision)

    return state, net, dict(cond=cond, c=c, pts=pts, freq=freq, phase=phase, z=z, noise=noise), run


_ORACLE_FIELD = {}


def oracle_field(key, state, inp):
    """The float64 field of one setup, computed once and shared by the four compositing variants (never modified)."""
    if key not in _ORACLE_FIELD:
        cond, pts = inp["cond"], inp["pts"]
        B, N = pts.shape[:2]
        geo = O.geo_features(pts, cond["skeletons_xyz"], cond["vertices"], cond["tpose_vertices"], cond["fk_matrices"],
                             cond["lbs_weights"], False)
        dirs = torch.zeros(B, N, 3)
        dirs[..., 2] = -1
        sd = {k: v.double() for k, v in state.items()}
        _ORACLE_FIELD[key] = O.neural_field(sd, pts.double(), inp["freq"].double(), inp["phase"].double(), geo.double(),
                                            dirs.double(), 0.7)
    return _ORACLE_FIELD[key]


@pytest.mark.parametrize("engine", ["f16x2", "f16x3"])
@pytest.mark.parametrize("S,R,hidden", [(64, 7, 64), (64, 40, 256), (128, 12, 128), (96, 3, 200)])
def test_ray_head_vs_oracle(S, R, hidden, engine):
    """NT 4 and 8, padded channels (200), 2 / 3 / 4 steps per ray, a tail flush with fewer than 32 rays; all four
    (last_back, white_back) combinations against the oracle."""
    state, net, inp, run = geo_setup(S, R, hidden, engine=engine)
    net.refine_last_sample = False          # the engine under test alone (the x3 relaunch has its own test below)
    field = oracle_field((S, R, hidden), state, inp)
    B = 2
    for last_back in (False, True):
        for white_back in (False, True):
            ref = O.ray_integration(field.reshape(B, R, S, -1), inp["z"].double(), inp["noise"].double(), "relu", last_back, white_back)
            got = run(last_back, white_back)
            for a, b, nm in zip(got, ref, NAMES):
                assert a.shape == b.shape, nm
                e = rel_err(a.cpu(), b)
                print(f"{engine} S={S} R={R} hidden={hidden} last_back={last_back} white_back={white_back} {nm}: {e:.3e}")
                assert e < TOL, (nm, last_back, white_back)
            e = rel_err(got[0].cpu()[..., :3], ref[0][..., :3])
            print(f"  colours: {e:.3e}")
            assert e < TOL


def test_units_relaunch_with_a_full_flush_equals_the_x3_whole_render():
    """The refinement relaunch runs at most 8 workgroups per item: 1200 units of one ray (S = 32) are 300 unit groups, so every
    wave walks ~37 rays, a full 32-ray flush plus a tail.  Every unit listed: bit-identical to the x3 engine's whole render (a
    row's head result does not depend on the rows that share its tile)."""
    S, R, hidden, B = 32, 1200, 64, 2
    _, net, _, run = geo_setup(S, R, hidden, B=B, V=300, engine="f16x2", with_noise=False)
    net.refine_last_sample = False
    x3 = [t.clone() for t in run(True, True, precision="f16x3")]
    net.refine_last_sample, net.refine_eps, net.refine_capacity = True, 1e30, R
    out = run(True, True)
    assert net.refined_units().tolist() == [R] * B
    for a, b, nm in zip(out, x3, NAMES):
        assert torch.equal(a, b), nm


def test_main_kernel_waves_that_flush_twice_vs_the_unfused_path():
    """B = 1, S = 32 and just more rays than 32 per wave of every persistent workgroup: some waves run a full flush and a tail.
    Against the unfused GPU path (per-sample field + ray_integration)."""
    S, hidden, B = 32, 64, 1
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    R = 32 * 4 * (4 * cus) + 37            # 4 persistent workgroups per CU, 4 waves each: ten workgroups get a 33rd trip
    state, net = random_state(hidden, hidden, seed=5, precision="f16x2")
    with torch.no_grad():
        net.sigma_layer.weight.mul_(40.0)
    g = torch.Generator(device=DEV).manual_seed(17)
    N = R * S
    pts = torch.rand(B, N, 3, generator=g, device=DEV) * 2 - 1
    geo = torch.rand(B, N, 31, generator=g, device=DEV) * 2 - 1
    freq = torch.randn(B, 4 * hidden, generator=g, device=DEV) * 0.5
    phase = torch.randn(B, 4 * hidden, generator=g, device=DEV)
    z = torch.sort(torch.rand(B, R, S, 1, generator=g, device=DEV) + 11, dim=2).values
    noise = torch.randn(B, R, S, 1, generator=g, device=DEV) * 0.3
    for engine in ("f16x2", "f16x3"):
        got = net.render(pts, freq, phase, geo, None, z, S, input_scaler=0.7, noise=noise, clamp_mode="relu", last_back=False,
                         white_back=True, precision=engine)
        field = net(pts, freq, phase, geo, None, input_scaler=0.7, precision=engine)
        ref = vr.ray_integration(field.reshape(B, R, S, -1), z, last_back=False, white_back=True, clamp_mode="relu", noise=noise)
        for a, b, nm in zip(got, ref, NAMES):
            assert a.shape == b.shape, nm
            e = rel_err(a, b)
            print(f"{engine} R={R} {nm}: {e:.3e}")
            assert e < FIELD_TOL, (engine, nm)
        assert rel_err(got[0][..., :3], ref[0][..., :3]) < FIELD_TOL


@pytest.mark.parametrize("engine,entry", [("f16x2", "h3d_render_fused_x2"), ("f16x3", "h3d_render_fused_x3")])
def test_every_row_is_finished_whatever_the_buffer_held(engine, entry):
    """The feature slots double as the parking place of hbar: a direct C-ABI call on caller-owned buffers pre-filled with NaN ends
    with finite outputs that equal, bit for bit, a run on zero-filled buffers; two runs are bit-identical (no atomics)."""
    S, R, hidden, B = 64, 150, 64, 2
    _, net = random_state(hidden, hidden, seed=11, precision=engine)
    g = torch.Generator().manual_seed(23)
    N = R * S
    pts = (torch.rand(B, N, 3, generator=g) * 2 - 1).to(DEV)
    geo = (torch.rand(B, N, 31, generator=g) * 2 - 1).to(DEV)
    freq = (torch.randn(B, 4 * hidden, generator=g) * 0.5).to(DEV)
    phase = torch.randn(B, 4 * hidden, generator=g).to(DEV)
    z = torch.sort(torch.rand(B, R, S, generator=g) + 11, dim=2).values.to(DEV)
    blob = net.packed_weights(torch.device(DEV), engine)
    lib, p = h3dlib.load(), h3dlib.ptr

    def call(fill):
        feats = torch.full((B, R, hidden + 3), fill, device=DEV)
        depth = torch.full((B, R, 1), fill, device=DEV)
        weights = torch.full((B, R, S, 1), fill, device=DEV)
        rc = getattr(lib, entry)(p(blob), p(pts), p(geo), None, p(freq), p(phase), p(z), None, p(feats), p(depth), p(weights),
                                 B, R, S, hidden, hidden, 31, ctypes.c_float(0.7), 0, 1, 1, h3dlib.stream_handle())
        h3dlib.check(rc, entry)
        torch.cuda.synchronize()
        return feats, depth, weights

    nan, zero, again = call(float("nan")), call(0.0), call(0.0)
    for a, b, c, nm in zip(nan, zero, again, NAMES):
        assert bool(torch.isfinite(a).all()), nm
        assert torch.equal(a, b), nm
        assert torch.equal(b, c), nm


GATING = [("s16", 16, 30, 48, 48), ("narrow_head", 64, 5, 64, 32)]


def gating_outputs():
    """The two calls the per-ray head must NOT take (S < 32; feature_dim < hidden_dim), on both engines -> {key: array}."""
    out = {}
    for tag, S, R, hidden, feature in GATING:
        for engine in ("f16x2", "f16x3"):
            _, net, _, run = geo_setup(S, R, hidden, feature=feature, V=200, seed=7, engine=engine)
            net.refine_last_sample = False
            for t, nm in zip(run(True, True), NAMES):
                out[f"{tag}/{engine}/{nm}"] = t.cpu().numpy()
    return out


def test_calls_outside_the_gate_keep_the_per_sample_heads_bits():
    """S = 16 and feature_dim < hidden_dim stay on the per-sample head: the same bits as the kernel before the per-ray head
    existed (tests/golden/ray_head_gating.npz, recorded on that build with gating_outputs())."""
    want = np.load(os.path.join(GOLDEN, "ray_head_gating.npz"))
    got = gating_outputs()
    assert sorted(want.files) == sorted(got)
    for k in want.files:
        assert got[k].shape == want[k].shape, k
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
