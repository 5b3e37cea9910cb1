"""Which entry point of the C ABI each field engine's _forward_fused / render / render_geo calls, and with how many arguments
(lib/implicit_funcitions/modulated.py), pinned without a GPU: _lib.load() is a fake whose entry points record their name and
argument count and succeed.  The count must be the one _lib._SIGNATURES declares -- ctypes would refuse anything else on the
device -- and the engine may be named per call (`precision=`) instead of through the module attribute."""
import importlib
from unittest import mock

import pytest
import torch

impl = importlib.import_module("3dhumangan_amd.lib.implicit_funcitions")
h3dlib = importlib.import_module("3dhumangan_amd._lib")

# engine -> pack-size, pack, field, fused render, fused render with in-kernel geometry
ENTRY = {
    "f16x3": ("h3d_field_pack_x3_size", "h3d_field_pack_x3", "h3d_neural_field_x3", "h3d_render_fused_x3", "h3d_render_fused_x3_geo"),
    "f16x2": ("h3d_field_pack_x2_size", "h3d_field_pack_x2", "h3d_neural_field_x2", "h3d_render_fused_x2", "h3d_render_fused_x2_geo"),
    "f16x3t": ("h3d_field_pack_x3t_size", "h3d_field_pack_x3t", "h3d_neural_field_x3t", "h3d_render_fused_x3t", None),
    "f16x1t": ("h3d_field_pack_x3t_size", "h3d_field_pack_x3t", "h3d_neural_field_x3t_tier", "h3d_render_fused_x3t_tier", None),
    "f16x2t": ("h3d_field_pack_x3t_size", "h3d_field_pack_x2t", "h3d_neural_field_x3t_tier", "h3d_render_fused_x3t_tier", None),
    "f32": ("h3d_field_pack_size", "h3d_field_pack", "h3d_neural_field", "h3d_render_fused", None),
}
B, R, S, V, HID, F = 2, 3, 8, 5, 32, 32


class Field(impl.COORDCONCATSIREN):
    assigned = []

    def __setattr__(self, name, value):
        if name == "precision":
            Field.assigned.append(value)
        super().__setattr__(name, value)


class FakeLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, len(args)))
            return 4096 if name.endswith("_size") else 0
        return entry


def declared(*names):
    return [(n, len(h3dlib._SIGNATURES[n][1])) for n in names]


@pytest.fixture
def rig():
    net = Field(input_dim=3, latent_dim=HID, hidden_dim=HID, geo_feature_dim=31, output_dim=F + 4, feature_dim=F, num_blocks=4).eval()
    net.refine_last_sample = False
    lib = FakeLib()
    with mock.patch.object(h3dlib, "load", lambda: lib), mock.patch.object(h3dlib, "need_cuda", lambda *t: None), \
            mock.patch.object(h3dlib, "stream_handle", lambda: None):
        yield net, lib


def inputs():
    N = R * S
    z = torch.zeros
    return dict(pts=z(B, N, 3), fr=z(B, 4 * HID), ph=z(B, 4 * HID), geo=z(B, N, 31), dirs=z(B, N, 3), zv=z(B, R, S, 1),
                noise=z(B, R, S, 1), idx=z(B, N, dtype=torch.int32), sk=z(B, 24, 3), vt=z(B, V, 3), tv=z(B, V, 3), vik=z(B, V, 16))


def call(net, what, t, **kw):
    if what == "field":
        out = net._forward_fused(t["pts"], t["fr"], t["ph"], t["geo"], t["dirs"], 0.7, **kw)
        assert out.shape == (B, R * S, F + 4)
        return
    if what == "render":
        out = net.render(t["pts"], t["fr"], t["ph"], t["geo"], None, t["zv"], S, input_scaler=0.7, noise=t["noise"], clamp_mode="softplus",
                         last_back=True, **kw)
    else:
        out = net.render_geo(t["pts"], t["fr"], t["ph"], t["idx"], t["sk"], t["vt"], t["tv"], t["vik"], t["dirs"], t["zv"], S,
                             input_scaler=0.7, clamp_mode="relu", white_back=True, **kw)
    assert [tuple(o.shape) for o in out] == [(B, R, F + 3), (B, R, 1), (B, R, S, 1)]


@pytest.mark.parametrize("engine", list(ENTRY))
def test_each_engine_calls_its_entry_points(rig, engine):
    net, lib = rig
    size, pack, field, render, geo = ENTRY[engine]
    net.precision = engine
    t = inputs()
    call(net, "field", t)
    assert lib.calls == declared(size, pack, field)                  # packed at first use ...
    call(net, "render", t)
    assert lib.calls[3:] == declared(render)                         # ... and cached while the weights stand
    assert net.render_geo_supported(S) == (geo is not None)
    if geo is not None:
        call(net, "render_geo", t)
        assert lib.calls[4:] == declared(geo)
    assert list(net._packed) == [pack] and net._packed[pack][1].numel() == 1024


def test_the_refinement_runs_the_x2_launch_then_the_x3_units(rig):
    net, lib = rig
    net.precision, net.refine_last_sample = "f16x2", True
    del Field.assigned[:]
    call(net, "render_geo", inputs())
    assert lib.calls == declared("h3d_field_pack_x2_size", "h3d_field_pack_x2", "h3d_field_pack_x3_size", "h3d_field_pack_x3",
                                 "h3d_render_fused_x2_geo_ref", "h3d_render_fused_x3_geo_units")
    assert sorted(net._packed) == ["h3d_field_pack_x2", "h3d_field_pack_x3"]
    assert net.refined_units().shape == (B,) and net.precision == "f16x2"
    assert Field.assigned == []                                      # the x3 blob is asked for by name, nothing is swapped


@pytest.mark.parametrize("engine", list(ENTRY))
def test_the_engine_can_be_named_per_call(rig, engine):
    """precision= runs the call on that engine whatever the module's own is, and leaves the attribute alone."""
    net, lib = rig
    size, pack, field, render, geo = ENTRY[engine]
    net.precision = own = "f32" if engine != "f32" else "f16x3t"
    del Field.assigned[:]
    t = inputs()
    call(net, "field", t, precision=engine)
    call(net, "render", t, precision=engine)
    names = [size, pack, field, render]
    assert net.render_geo_supported(S, engine) == (geo is not None) and not net.render_geo_supported(S)
    if geo is not None:
        call(net, "render_geo", t, precision=engine)
        names.append(geo)
    assert lib.calls == declared(*names)
    assert net.packed_weights("cpu", engine) is net._packed[pack][1] and list(net._packed) == [pack]
    assert net.fused_supported(96, engine) == (engine in ("f16x2", "f16x3")) and not net.fused_supported(96)
    assert Field.assigned == [] and net.precision == own
    with pytest.raises(ValueError, match="unknown precision 'f8'"):
        net.packed_weights("cpu", "f8")


def test_render_geo_checks_its_shapes(rig):
    net, _ = rig
    net.precision = "f16x2"
    t = inputs()
    with pytest.raises(ValueError, match=r"nn_index must be int32 \[B, N\]"):
        call(net, "render_geo", dict(t, idx=t["idx"].long()))
    with pytest.raises(ValueError, match="skeletons .B,24,3., vertices / tpose_vertices .B,V,3., vertex_ik .B,V,16. expected"):
        call(net, "render_geo", dict(t, vik=torch.zeros(B, V + 1, 16)))


def test_cuda_means_the_current_device():
    with mock.patch.object(torch.cuda, "current_device", lambda: 3):
        assert h3dlib.canonical_device("cuda") == torch.device("cuda", 3)
        assert h3dlib.canonical_device(torch.device("cuda")) == torch.device("cuda", 3)
        assert h3dlib.canonical_device("cuda:1") == torch.device("cuda", 1)
        assert h3dlib.canonical_device("cpu") == torch.device("cpu")
