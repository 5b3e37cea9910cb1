"""GPU parity: fp32-MFMA neural field and fused render vs golden vectors / the CPU oracle."""
import importlib

import pytest
import torch

import h3d_oracle as O
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
impl = importlib.import_module("3dhumangan_amd.lib.implicit_funcitions")
DEV = "cuda"
FIELD_TOL = 1e-3      # north_star: within 1e-3 relative fp32; per-engine bars from the arithmetic: tests/test_gpu_field_ladder.py


ENGINES = ["f16x2", "f16x2t", "f16x3", "f16x3t", "f32"]


def make_field(state, hidden, feature, prefix="neural_field.", precision=None):
    net = impl.COORDCONCATSIREN(input_dim=3, latent_dim=hidden, hidden_dim=hidden, geo_feature_dim=31,
                                output_dim=feature + 4, feature_dim=feature, num_blocks=4)
    sd = {k[len(prefix):]: v for k, v in state.items() if k.startswith(prefix)}
    net.load_state_dict(sd)
    if precision:
        net.precision = precision
    return net.to(DEV).eval()          # eval: the fused inference kernels (train mode would take the differentiable path)


def random_state(hidden, feature, seed, precision=None):
    torch.manual_seed(seed)
    net = impl.COORDCONCATSIREN(input_dim=3, latent_dim=hidden, hidden_dim=hidden, geo_feature_dim=31,
                                output_dim=feature + 4, feature_dim=feature, num_blocks=4)
    with torch.no_grad():
        for p in net.parameters():
            if p.ndim == 1:
                p.add_(0.05 * torch.randn_like(p))
    if precision:
        net.precision = precision
    return {"neural_field." + k: v.detach().clone() for k, v in net.state_dict().items()}, net.to(DEV).eval()


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name,hidden", [("field_h64", 64), ("field_h40", 40)])
def test_field_golden(name, hidden, engine):
    g = load_golden(name)
    net = make_field(g["state"], hidden, hidden, precision=engine)
    out = net(g["points"].to(DEV), g["freq"].to(DEV), g["phase"].to(DEV), g["geo"].to(DEV), g["dirs"].to(DEV),
              input_scaler=2.0 / 2.85)
    assert out.shape == g["out"].shape
    assert rel_err(out.cpu(), g["out"]) < FIELD_TOL
    # per-channel-group check so a wrong small head cannot hide behind large features
    for sl in (slice(0, 3), slice(3, 3 + hidden), slice(3 + hidden, 4 + hidden)):
        assert rel_err(out.cpu()[..., sl], g["out"][..., sl]) < FIELD_TOL


@pytest.mark.parametrize("hidden,engine", [(256, "f16x2"), (256, "f16x3"), (256, "f16x3t"), (256, "f16x2t"), (256, "f32"), (384, "f16x3t"), (384, "f16x2t"), (384, "f32"), (420, "f16x2t"),
                                           (420, "f16x3t"), (420, "f32")])
def test_field_reference_vectors_at_shipped_widths(hidden, engine):
    """The reference module's own output at the widths of MAP3DBN512 / MAP3DBN / MAP3DBN512L (not the oracle's)."""
    g = load_golden(f"field_h{hidden}")
    net = make_field({k: v.float() for k, v in g["state"].items()}, hidden, hidden, precision=engine)
    out = net(g["points"].to(DEV), g["freq"].to(DEV), g["phase"].to(DEV), g["geo"].to(DEV), g["dirs"].to(DEV),
              input_scaler=2.0 / 2.85)
    for sl in (slice(0, 3), slice(3, 3 + hidden), slice(3 + hidden, 4 + hidden)):
        assert rel_err(out.cpu()[..., sl], g["out"][..., sl]) < FIELD_TOL, sl


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", ["gen_tiny_mixed", "gen_tiny_isolated_legacy"])
def test_field_in_generator_fixture(name, engine):
    g = load_golden(name)
    s, cfg = g["stage"], g["meta"]
    H = cfg["hidden_dim"]
    net = make_field(g["state"], H, cfg["feature_dim"], precision=engine)
    B = s["points"].shape[0]
    # lock_view_dependence: pass None (kernel folds dir=(0,0,-1)) and the explicit tensor; both must agree
    a = net(s["points"].to(DEV), s["freq"].to(DEV), s["phase"].to(DEV), s["geo"].to(DEV), None,
            input_scaler=2.0 / cfg["side_length"])
    b = net(s["points"].to(DEV), s["freq"].to(DEV), s["phase"].to(DEV), s["geo"].to(DEV), s["dirs"].to(DEV),
            input_scaler=2.0 / cfg["side_length"])
    ref = s["field"].reshape(B, -1, H + 4)
    assert rel_err(a.cpu(), ref) < FIELD_TOL
    assert rel_err(b.cpu(), ref) < FIELD_TOL


@pytest.mark.parametrize("hidden,feature,N,engine", [(256, 256, 200, "f32"), (256, 256, 200, "f16x3"), (256, 256, 200, "f16x2"), (128, 96, 77, "f16x2"),
                                                     (200, 256, 333, "f16x2"), (32, 32, 1, "f16x2"), (384, 384, 130, "f32"),
                                                     (420, 420, 64, "f32"), (32, 32, 1, "f32"), (32, 32, 1, "f16x3"),
                                                     (128, 96, 77, "f32"), (128, 96, 77, "f16x3"), (200, 256, 333, "f16x3"),
                                                     (384, 384, 130, "f16x3t"), (420, 420, 200, "f16x3t"), (256, 256, 65, "f16x3t"),
                                                     (32, 32, 1, "f16x3t"), (128, 96, 77, "f16x3t"), (200, 300, 333, "f16x3t"),
                                                     (448, 448, 64, "f16x3t"), (170, 170, 100, "f16x3t"),
                                                     (384, 384, 130, "f16x2t"), (420, 420, 200, "f16x2t"), (256, 256, 65, "f16x2t"),
                                                     (32, 32, 1, "f16x2t"), (128, 96, 77, "f16x2t"), (200, 300, 333, "f16x2t"),
                                                     (448, 448, 64, "f16x2t"), (170, 170, 100, "f16x2t")])
def test_field_real_widths_vs_oracle(hidden, feature, N, engine):
    state, net = random_state(hidden, feature, seed=hidden, precision=engine)
    g = torch.Generator().manual_seed(N)
    B = 2
    pts = torch.rand(B, N, 3, generator=g) * 2 - 1
    geo = torch.rand(B, N, 31, generator=g) * 2 - 1
    dirs = torch.nn.functional.normalize(torch.randn(B, N, 3, generator=g), dim=-1)
    freq = torch.randn(B, 4 * hidden, generator=g) * 0.5
    phase = torch.randn(B, 4 * hidden, generator=g)
    ref = O.neural_field({k: v.double() for k, v in state.items()}, pts.double(), freq.double(), phase.double(),
                         geo.double(), dirs.double(), 2.0 / 2.85)
    out = net(pts.to(DEV), freq.to(DEV), phase.to(DEV), geo.to(DEV), dirs.to(DEV), input_scaler=2.0 / 2.85)
    for sl in (slice(0, 3), slice(3, 3 + feature), slice(3 + feature, 4 + feature)):
        assert rel_err(out.cpu()[..., sl], ref[..., sl]) < FIELD_TOL, sl


@pytest.mark.parametrize("S,R,hidden,engine", [(8, 20, 32, "f32"), (16, 30, 48, "f32"), (32, 9, 64, "f32"), (64, 5, 256, "f32"),
                                                (128, 3, 64, "f32"), (32, 7, 384, "f32"), (8, 20, 32, "f16x3"),
                                                (8, 20, 32, "f16x2"), (16, 30, 48, "f16x2"), (32, 9, 64, "f16x2"), (64, 5, 256, "f16x2"),
                                                (128, 3, 64, "f16x2"), (32, 7, 256, "f16x2"), (96, 3, 128, "f16x2"),
                                                (16, 30, 48, "f16x3"), (32, 9, 64, "f16x3"), (64, 5, 256, "f16x3"),
                                                (128, 3, 64, "f16x3"), (32, 7, 256, "f16x3"), (96, 3, 128, "f16x3"),
                                                (8, 20, 32, "f16x3t"), (16, 30, 48, "f16x3t"), (32, 9, 64, "f16x3t"),
                                                (64, 5, 420, "f16x3t"), (128, 3, 200, "f16x3t"), (32, 7, 384, "f16x3t"),
                                                (64, 6, 384, "f16x3t"), (192, 2, 300, "f16x3t"), (16, 11, 420, "f16x3t"),
                                                (8, 20, 32, "f16x2t"), (16, 30, 48, "f16x2t"), (32, 9, 64, "f16x2t"),
                                                (64, 5, 420, "f16x2t"), (128, 3, 200, "f16x2t"), (32, 7, 384, "f16x2t"),
                                                (64, 6, 384, "f16x2t"), (192, 2, 300, "f16x2t"), (16, 11, 420, "f16x2t")])
@pytest.mark.parametrize("last_back,white_back,clamp", [(False, True, "relu"), (True, False, "softplus")])
def test_fused_render_vs_oracle(S, R, hidden, engine, last_back, white_back, clamp):
    state, net = random_state(hidden, hidden, seed=S + hidden, precision=engine)
    # make densities matter: scale the sigma head up
    with torch.no_grad():
        net.sigma_layer.weight.mul_(40.0)
        state["neural_field.sigma_layer.weight"] = net.sigma_layer.weight.detach().cpu().clone()
    g = torch.Generator().manual_seed(R)
    B, N = 2, R * S
    pts = torch.rand(B, N, 3, generator=g) * 2 - 1
    geo = torch.rand(B, N, 31, generator=g) * 2 - 1
    freq = torch.randn(B, 4 * hidden, generator=g) * 0.5
    phase = torch.randn(B, 4 * hidden, generator=g)
    z = torch.sort(torch.rand(B, R, S, 1, generator=g) + 11, dim=2).values
    noise = torch.randn(B, R, S, 1, generator=g) * 0.3
    dirs = torch.zeros(B, N, 3)
    dirs[..., 2] = -1
    sd = {k: v.double() for k, v in state.items()}
    field = O.neural_field(sd, pts.double(), freq.double(), phase.double(), geo.double(), dirs.double(), 0.7)
    ref = O.ray_integration(field.reshape(B, R, S, -1), z.double(), noise.double(), clamp, last_back, white_back)
    got = net.render(pts.to(DEV), freq.to(DEV), phase.to(DEV), geo.to(DEV), None, z.to(DEV), S, input_scaler=0.7,
                     noise=noise.to(DEV), clamp_mode=clamp, last_back=last_back, white_back=white_back)
    for a, b, nm in zip(got, ref, ("feats", "depth", "weights")):
        assert a.shape == b.shape, nm
        assert rel_err(a.cpu(), b) < FIELD_TOL, nm
    assert rel_err(got[0].cpu()[..., :3], ref[0][..., :3]) < FIELD_TOL


def test_x3_engine_rejects_wide_models():
    h3dlib = importlib.import_module("3dhumangan_amd._lib")
    _, net = random_state(384, 384, seed=0, precision="f16x3")
    with pytest.raises(h3dlib.H3DError):
        net(torch.zeros(1, 4, 3, device=DEV), torch.zeros(1, 1536, device=DEV), torch.zeros(1, 1536, device=DEV),
            torch.zeros(1, 4, 31, device=DEV), None)


def test_fused_rejects_unsupported_steps():
    _, net = random_state(32, 32, seed=0)
    h3dlib = importlib.import_module("3dhumangan_amd._lib")
    B, R, S = 1, 4, 12
    x = torch.zeros(B, R * S, 3, device=DEV)
    with pytest.raises(h3dlib.H3DError):
        net.render(x, torch.zeros(B, 128, device=DEV), torch.zeros(B, 128, device=DEV),
                   torch.zeros(B, R * S, 31, device=DEV), None, torch.zeros(B, R, S, 1, device=DEV), S)
