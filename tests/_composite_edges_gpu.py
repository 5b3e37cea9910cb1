"""The GPU side of the compositing edge rays (tests/_composite_reference.py): run one kernel on one case and return its per-ray
errors against the float64 oracle.  Shared by tests/test_gpu_composite_edges.py and tools/composite_edges_report.py."""
import importlib

import torch

import _composite_reference as CR

DEV = "cuda"
vr = importlib.import_module("3dhumangan_amd.lib.generators.volume_rendering")

FORWARD_S, BACKWARD_S, CHANNELS = (1, 7, 64, 65, 128, 200), (8, 64, 65, 200), (7, 6)      # C = 7: the vec4 kernels, 6: the scalar ones
LONG_RAYS = ("opaque_at_64_lastneg", "after_opaque_at_64_lastneg")      # 2 rays: an early opaque sample in front of 127 carries, a plain one
GEO_CASE = (32, 32, 32, ("relu", True, False))                          # S, hidden, feature, mode of the render_geo case


def fused_cases():
    """(engine, S, hidden) with feature = 32: hidden = 32 takes the per-ray feature head from S = 32 on; hidden 64 at S = 64 the
    per-sample one."""
    out = []
    for engine in ("f16x2", "f16x3", "f16x3t", "f16x2t", "f32"):
        steps = (8, 16, 32, 64, 96) if CR.ENGINE_WIDTH[engine] == 32 else (8, 16, 32, 64, 128)
        out += [(engine, S, 32) for S in steps] + [(engine, 64, 64)]
    return out


def integrate(i, mode, grad=False):
    """vr.ray_integration on case_inputs `i` -> (its outputs, the same flattened to rays: features [N, C], depth [N], weights
    [N, S], the field tensor on the device)."""
    field = i["field"].to(DEV).requires_grad_(grad)
    f, d, w = vr.ray_integration(field, i["z"].to(DEV), noise=i["noise"].to(DEV), clamp_mode=mode[0], last_back=mode[1], white_back=mode[2])
    N, S = CR.B * i["R"], i["z"].shape[2]
    assert f.shape == (CR.B, i["R"], i["field"].shape[-1] - 1) and d.shape == (CR.B, i["R"], 1) and w.shape == (CR.B, i["R"], S, 1)
    return (f, d, w), (f.reshape(N, -1), d.reshape(N), w.reshape(N, S)), field


def forward_errors(S, C, mode, only=None):
    _, got, _ = integrate(CR.case_inputs(S, C, only), mode)
    return CR.forward_errors_of(got, S, mode, C, only)


def backward_errors(S, C, mode):
    """The kernel pair's gradients with the cotangents of case_inputs against autograd through the float64 oracle."""
    i = CR.case_inputs(S, C)
    (f, d, w), _, field = integrate(i, mode, grad=True)
    ((f * i["pf"].to(DEV)).sum() + (d * i["pd"].to(DEV)).sum() + (w * i["pw"].to(DEV)).sum()).backward()
    N = CR.B * i["R"]
    got = field.grad[..., -1].reshape(N, S), field.grad[..., :-1].reshape(N, S, -1)
    return CR.backward_errors(got, CR.oracle_backward(S, mode, C))


def edge_net(c, hidden, feature, engine):
    """random_state's module (tests/test_gpu_field.py) on the engine, with the scaled density head of the CPU case `c`."""
    from test_gpu_field import random_state
    state, net = random_state(hidden, feature, seed=c["seed"], precision=engine)
    assert torch.equal(state["neural_field.network.0.layer.weight"], c["state"]["neural_field.network.0.layer.weight"])
    with torch.no_grad():
        net.sigma_layer.weight.copy_(c["state"]["neural_field.sigma_layer.weight"])
        net.sigma_layer.bias.copy_(c["state"]["neural_field.sigma_layer.bias"])
    return net


def fused_errors(engine, S, hidden, feature=32):
    """net.render on the engine in all eight modes -> {mode: per-ray errors}."""
    c = CR.fused_case(S, hidden, feature)
    net = edge_net(c, hidden, feature, engine)
    pts, freq, phase, geo, z, noise = (c[k].to(DEV) for k in ("pts", "freq", "phase", "geo", "z", "noise"))
    out = {}
    for mode in CR.MODES:
        got = net.render(pts, freq, phase, geo, None, z, S, input_scaler=0.7, noise=noise, clamp_mode=mode[0], last_back=mode[1],
                         white_back=mode[2], precision=engine)
        out[mode] = CR.fused_errors(got, S, hidden, feature, mode)
    return out


def render_geo_errors():
    """The default production route (x2 with the x3 relaunch for listed units) on the edge rays -> (per-ray errors, units listed
    per item)."""
    smpl = importlib.import_module("3dhumangan_amd.lib.components.smpl")
    S, hidden, feature, mode = GEO_CASE
    c = CR.fused_case(S, hidden, feature, geo=True)
    net = edge_net(c, hidden, feature, "f16x2")
    assert net.refine_last_sample and net.render_geo_supported(S)
    cond = {k: v.to(DEV) for k, v in c["cond"].items()}
    pts, freq, phase, z, noise = (c[k].to(DEV) for k in ("pts", "freq", "phase", "z", "noise"))
    vik = smpl.vertex_inverse_transforms(cond["fk_matrices"], cond["lbs_weights"])
    idx = smpl.nearest_vertex(pts, cond["vertices"])
    got = net.render_geo(pts, freq, phase, idx, cond["skeletons_xyz"], cond["vertices"], cond["tpose_vertices"], vik, None, z, S,
                         legacy_mode=False, input_scaler=0.7, noise=noise, clamp_mode=mode[0], last_back=mode[1], white_back=mode[2])
    return CR.fused_errors(got, S, hidden, feature, mode, geo=True), net.refined_units().cpu().tolist()
