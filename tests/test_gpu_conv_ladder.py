"""The convolution family (csrc/conv_x3.hip, csrc/wgrad_x3.hip, their AMP instantiations, ops/linear.py on the 1x1 instantiation)
against the bars of its own arithmetic (tests/_conv_arithmetic.py; derivation and the CPU side: tests/test_conv_ladder_cpu.py,
DESIGN.md 2).  The 1e-3 bar of test_gpu_conv.py lets a kernel pass that lost a cross term in one tap, chunk, K-slice or k-step;
these do not:
    fp32 operands, dW from f16 operands   against float64: (smallest single-defect error D1 / D2 over the declared loop units) / 3
    two-plane AMP outputs                 share of stored elements that are not f16(float64 result): (smallest D4 share) / 3;
                                          max-norm: 3 x the healthy fp32-accumulated emulation
    one-plane AMP outputs                 share and max-norm: 3 x the healthy fp32-accumulated emulation
Inputs and weights are seeded fp32 (non-zero lo planes); the CPU side of a case is computed once and shared by its tiers.
tools/conv_accuracy_report.py records the same figures in profiles/conv_accuracy_ladder.json."""
import pytest
import torch

import _conv_arithmetic as A
import _conv_ladder_gpu as G

pytestmark = pytest.mark.gpu


def _show(records):
    for r in records:
        print(f"{r['tier']:6s} {r['case']:20s} {r['group']:9s} measured {r['measured']:.3e}  bar {r['bar']:.3e}  "
              f"healthy {r['healthy_reference']:.3e}  headroom {r['headroom']:7.1f} x")


def _failed(records, groups=None):
    return [(r["group"], r["measured"], r["bar"]) for r in records if (groups is None or r["group"] in groups) and not r["measured"] < r["bar"]]


@pytest.mark.parametrize("case,tier", [pytest.param(c, t, id=f"{c.name}-{t}") for c in A.CASES for t in c.tiers])
def test_kernels_meet_the_bars_of_their_arithmetic(case, tier, monkeypatch):
    if tier in G.PLANES:
        monkeypatch.setattr(G.conv, "AMP_WEIGHT_PLANES", G.PLANES[tier])
    records = G.measure(case, tier)
    _show(records)
    assert not _failed(records), _failed(records)


# One end-to-end sensitivity test per tier that changes no kernel: the weight stream comes back from the packer with the lo plane of
# ONE filter tap zeroed (D2 for fp32 activations, D4 for the two-plane AMP tier).  The bars must fail on it and hold without it.
SENSITIVITY = [("c64-64-k3-p63", "f32", ("y", "y_ch"), ("dx", "dx_ch")), ("c64-64-k3-p63", "f16x2", ("y_share",), ("dx_share",)),
               ("c512-512-k3-p32", "f32", ("y", "y_ch"), ("dx", "dx_ch")), ("c512-512-k3-p32", "f16x2", ("y_share",), ("dx_share",))]


@pytest.mark.parametrize("name,tier,fwd_groups,dx_groups", SENSITIVITY, ids=[f"{s[0]}-{s[1]}" for s in SENSITIVITY])
def test_a_zeroed_lo_plane_in_one_tap_violates_the_bars(name, tier, fwd_groups, dx_groups, monkeypatch):
    case = A.CASE[name]
    if tier in G.PLANES:
        monkeypatch.setattr(G.conv, "AMP_WEIGHT_PLANES", G.PLANES[tier])
    for transposed, groups, others in ((False, fwd_groups, dx_groups), (True, dx_groups, fwd_groups)):
        with G.lo_plane_zeroed(tap=4, transposed=transposed) as hits:
            broken = G.measure(case, tier)
        assert len(hits) == 1, hits                                   # exactly one stream of the run was tampered with
        print(f"lo plane of tap 4 zeroed in the {'backward-data' if transposed else 'forward'} stream:")
        _show([r for r in broken if r["group"] in groups + others])
        over = {r["group"]: r["measured"] / r["bar"] for r in broken if r["group"] in groups}
        assert all(v > 1.0 for v in over.values()), over             # every bar of the tampered primitive is violated
        assert not _failed(broken, others), _failed(broken, others)  # ... and only those: the other primitive still meets its own
    healthy = G.measure(case, tier)
    assert not _failed(healthy), _failed(healthy)


@pytest.mark.parametrize("co,ci,k", [(128, 64, 3), (64, 256, 1), (192, 192, 3)])
def test_device_f16_streams_hold_the_emulated_planes(co, ci, k):
    """h3d_conv_x3_pack_f16 / _f16x1 against split_f16 / f16 of the emulation, bit for bit (the bf16 stream: test_gpu_conv.py against
    conv.pack_stream_torch, which tests/test_conv_ladder_cpu.py ties to the emulation).  Layouts: include/h3d.h."""
    w = torch.randn(co, ci, k, k, generator=torch.Generator().manual_seed(co + ci + k)) / (ci * k * k) ** 0.5
    NT, nblk, _, _ = G.conv.tiling(ci, co)
    two = G.conv.pack_stream(w.to(G.DEV), half=True, planes=2).cpu().view(torch.float16)
    two = two.view(nblk, k * k, ci // 16, NT, 2, 2, 32, 8).permute(4, 0, 3, 6, 2, 5, 7, 1).reshape(2, co, ci, k, k)      # ob, tap, ks, nt, hi|lo, h, j, e
    hi, lo = A.split_f16(w.double())
    assert torch.equal(two[0].double(), hi) and torch.equal(two[1].double(), lo)
    one = G.conv.pack_stream(w.to(G.DEV), half=True, planes=1).cpu().view(torch.float16)
    one = one.view(nblk, k * k, ci // 32, NT, 2, 2, 32, 8).permute(0, 3, 6, 2, 4, 5, 7, 1).reshape(co, ci, k, k)         # ob, tap, ks / 2, nt, ks % 2, h, j, e
    assert torch.equal(one.double(), A.f16(w.double()))
