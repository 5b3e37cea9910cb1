"""The register engines hand out their work on demand (synthesis_x3.hip: 128-pixel tiles, field_x3.hip: unit groups): a persistent
workgroup starts at blockIdx.x and takes every further index from a per-item counter (h3d::work_counters).  A tile's arithmetic does
not depend on the workgroup that computes it, so every output must keep the bits it had when each workgroup walked a fixed stride:
tests/golden/dynamic_tiles.npz was recorded on that build with tests/golden/make_golden_dynamic_tiles.py.

The fixture holds one SHA-256 per batch item and array, not the arrays: the raw outputs of the cases below are 2.6 MB, a committed
file may be 1 MiB.  Equal digests are equal bits.

The cases the change was specified with hand every workgroup a single index on a 256-CU device (fewer tiles / unit groups per item
than workgroups per item); the two "walk" cases add launches whose workgroups come back to the counter."""
import ctypes
import hashlib
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_gpu_ray_head import NAMES, geo_setup
from test_gpu_x2_guard import make, run

pytestmark = pytest.mark.gpu
_lib = importlib.import_module("3dhumangan_amd._lib")
DEV = "cuda"
FIXTURE = os.path.join(GOLDEN, "dynamic_tiles.npz")

# tag -> (width, H, W, Hr, Wr, B)
SYNTH = {
    "w256": (256, 64, 128, 12, 24, 3),
    "w128": (128, 64, 128, 12, 24, 3),
    "few_tiles": (256, 40, 96, 8, 18, 2),          # 30 tiles: fewer than the workgroups per item
    "walk": (128, 64, 128, 12, 24, 40),            # 64 tiles for ceil(4 * 256 / 40) = 26 workgroups: two or three trips each
}
# tag -> (S, rays, hidden, B)
RENDER = {
    "s64": (64, 100, 256, 3),                      # 10 x 10 rays: 25 unit groups per item
    "s32": (32, 100, 256, 3),
    "walk": (32, 1500, 64, 3),                     # 375 unit groups for ceil(4 * 256 / 3) = 342 workgroups
}


def digests(t):
    """[B, ...] tensor -> uint8 [B, 32]: SHA-256 of every batch item's bytes."""
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return np.stack([np.frombuffer(hashlib.sha256(a[b].tobytes()).digest(), dtype=np.uint8) for b in range(a.shape[0])])


_SYNTH = {}


def synth_case(tag):
    """-> (G, meta, fmap, style, {engine: image}) of one synthesis case, computed once and never modified.  The x2 image is the
    x2 engine's own (monitor tolerance 1: no item is redone)."""
    if tag not in _SYNTH:
        width, H, W, Hr, Wr, B = SYNTH[tag]
        G, meta, _ = make(width, H, W, Hr, Wr, seed=21)
        plan = G.synthesis_plan(DEV)
        assert plan.engine == "f16x2"
        g = torch.Generator().manual_seed(width + H)
        fmap, style = torch.randn(B, Hr * Wr, width, generator=g), torch.randn(B, width, generator=g)
        plan.x2_monitor_tol = 1.0
        img = {"f16x2": run(G, meta, fmap, style)}
        assert plan.x2_fallback_items() == []
        plan.engine = "bf16x3"
        img["bf16x3"] = run(G, meta, fmap, style)
        plan.engine = "f16x2"
        _SYNTH[tag] = (G, meta, fmap, style, img)
    return _SYNTH[tag]


def synthesis_outputs():
    out = {}
    for tag in SYNTH:
        img = synth_case(tag)[4]
        for engine in ("f16x2", "bf16x3"):
            out[f"synthesis/{tag}/{engine}"] = digests(img[engine])
    return out


_RENDER = {}


def render_case(tag):
    """-> (net, run, {engine: (feats, depth, weights)}): f16x2 with its refinement relaunch (the default), and f16x3."""
    if tag not in _RENDER:
        S, R, hidden, B = RENDER[tag]
        _, net, _, go = geo_setup(S, R, hidden, B=B, V=300, seed=31, engine="f16x2")
        assert net.refine_last_sample
        res = {"f16x2": [t.clone() for t in go(True, True)], "f16x3": [t.clone() for t in go(True, True, precision="f16x3")]}
        _RENDER[tag] = (net, go, res)
    return _RENDER[tag]


def render_outputs():
    out = {}
    for tag in RENDER:
        res = render_case(tag)[2]
        for engine in ("f16x2", "f16x3"):
            for t, nm in zip(res[engine], NAMES):
                out[f"render/{tag}/{engine}/{nm}"] = digests(t)
    return out


def fixture_outputs():
    """Everything the fixture records -> {key: uint8 [B, 32]}."""
    return {**synthesis_outputs(), **render_outputs()}


def assert_matches_fixture(got):
    want = np.load(FIXTURE)
    for k, v in got.items():
        assert k in want.files, k
        same = (want[k] == v).all(axis=1)
        assert bool(same.all()), f"{k}: batch items {np.nonzero(~same)[0].tolist()} differ from the recorded bits"


@pytest.mark.parametrize("tag", list(SYNTH))
def test_synthesis_keeps_the_recorded_bits(tag):
    img = synth_case(tag)[4]
    assert_matches_fixture({f"synthesis/{tag}/{e}": digests(img[e]) for e in ("f16x2", "bf16x3")})


@pytest.mark.parametrize("engine", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("tag", list(SYNTH))
def test_every_pixel_is_written_on_every_run(tag, engine):
    """Three direct launches back to back into an image pre-filled with a sentinel: a counter left over from an earlier launch would
    end a workgroup's walk early and leave sentinel pixels."""
    G, meta, fmap, style, img = synth_case(tag)
    width, H, W, Hr, Wr, B = SYNTH[tag]
    plan = G.synthesis_plan(DEV)
    x2 = engine == "f16x2"
    seg = plan.build_x3(x2)
    Gt, cst, ab = plan.x3_forward_tables(fmap.to(DEV).float(), style.to(DEV).float(), x2)
    lib = _lib.load()
    entry = lib.h3d_synthesis_x2 if x2 else lib.h3d_synthesis_x3
    sentinel = -12345.0
    for _ in range(3):
        out = torch.full((B, 3, H, W), sentinel, device=DEV)
        _lib.check(entry(*plan._args(seg, Gt, cst, ab, out, B, Hr, Wr, H, W), _lib.stream_handle()), "synthesis")
        assert not bool((out == sentinel).any())
        assert torch.equal(out, img[engine])


@pytest.mark.parametrize("tag", list(SYNTH))
def test_redo_of_one_flagged_item(tag):
    """A tolerance between the largest and the second largest sampled error flags exactly one item: it comes from the bf16 engine,
    the others keep their x2 pixels, bit for bit."""
    G, meta, fmap, style, img = synth_case(tag)
    plan = G.synthesis_plan(DEV)
    B = fmap.shape[0]
    try:
        plan.x2_monitor_tol = 1.0
        run(G, meta, fmap, style)
        err = torch.sort(plan.x2_monitor_errors().cpu()).values
        assert float(err[-1]) > float(err[-2])
        plan.x2_monitor_tol = float((err[-1] + err[-2]) / 2)
        out = run(G, meta, fmap, style)
        flagged = plan.x2_fallback_items()
        assert len(flagged) == 1
        for b in range(B):
            assert torch.equal(out[b], img["bf16x3" if b in flagged else "f16x2"][b]), b
        assert not torch.equal(img["f16x2"][flagged[0]], img["bf16x3"][flagged[0]])
    finally:
        plan.x2_monitor_tol = 1.0


@pytest.mark.parametrize("tag", list(RENDER))
def test_render_keeps_the_recorded_bits_and_repeats_them(tag):
    net, go, res = render_case(tag)
    got = {}
    for engine in ("f16x2", "f16x3"):
        again = go(True, True, precision=engine)
        for a, b, nm in zip(again, res[engine], NAMES):
            assert torch.equal(a, b), (engine, nm)
            got[f"render/{tag}/{engine}/{nm}"] = digests(b)
    assert_matches_fixture(got)


@pytest.mark.parametrize("tag", list(RENDER))
def test_units_relaunch_reproduces_the_x3_render(tag):
    """Every unit listed for the refinement relaunch: the f16x2 call then returns the f16x3 render, bit for bit."""
    S, R, hidden, B = RENDER[tag]
    net, go, res = render_case(tag)
    keep = net.refine_eps, net.refine_capacity
    try:
        net.refine_eps, net.refine_capacity = 1e30, R
        out = go(True, True)
        assert net.refined_units().tolist() == [R] * B
        for a, b, nm in zip(out, res["f16x3"], NAMES):
            assert torch.equal(a, b), nm
    finally:
        net.refine_eps, net.refine_capacity = keep


@pytest.mark.parametrize("tag", ["w256", "walk"])
def test_two_streams_at_once(tag):
    """The same case launched on two streams at the same time (two generators of the same seed: a plan's own buffers belong to one
    stream at a time): each launch has its own block of counters, both images keep the recorded bits."""
    G, meta, fmap, style, img = synth_case(tag)
    width, H, W, Hr, Wr, B = SYNTH[tag]
    G2 = make(width, H, W, Hr, Wr, seed=21)[0]
    for g in (G, G2):
        g.synthesis_plan(DEV).x2_monitor_tol = 1.0
    run(G2, meta, fmap, style)                          # plans packed, buffers allocated: the timed part below is launches only
    dfmap, dstyle = fmap.to(DEV), style.to(DEV)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for _ in range(2):
        with torch.cuda.stream(s1):
            a = run(G, meta, dfmap, dstyle)
        with torch.cuda.stream(s2):
            b = run(G2, meta, dfmap, dstyle)
        outs += [a, b]
    torch.cuda.synchronize()
    for o in outs:
        assert torch.equal(o, img["f16x2"])
    assert_matches_fixture({f"synthesis/{tag}/f16x2": digests(outs[0]), })
