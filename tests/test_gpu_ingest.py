"""h3d_ingest on the GPU against the float64 restatement (tests/_ingest_reference.py).

Bars.  body_segments: bit-equal.  images and masks: 1e-6 absolute, derived: the values lie in [-1, 1], lambda is exact to one
rounding, the normalisation is two roundings and three lerps are six more -- at most 8 roundings of 2^-24, about 5e-7.
The measured maximum over every case of this file is recorded in profiles/ingest_parity.json."""
import importlib

import numpy as np
import pytest
import torch

from _ingest_reference import SHAPES, ingest_f64, make_inputs

pytestmark = pytest.mark.gpu
ing = importlib.import_module("3dhumangan_amd.lib.data.ingest")
BAR = 1e-6
# beside the listed shapes: the two at which the kernel takes another path -- 16-byte stores with 8-byte reads (the data's 2:1 with
# W % 4 == 0), and 16-byte stores with byte reads (W % 4 == 0 at another ratio)
ALL_SHAPES = SHAPES + [((32, 16), (16, 8)), ((5, 24), (10, 12))]


def _dev(arrays):
    return [torch.from_numpy(a).cuda() for a in arrays]


@pytest.mark.parametrize("geo_only", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("src,size", ALL_SHAPES)
def test_ingest_matches_the_float64_restatement(src, size, B, geo_only):
    worst = 0.0
    for kind in ("zero", "full", "random"):
        arrays = make_inputs(B, src[0], src[1], seed=11 * B + src[0], mask_kind=kind)
        want_i, want_m, want_s = ingest_f64(*arrays, size, geo_only)
        got = ing.ingest(*_dev(arrays), size, geo_only)
        assert got["images"].shape == (B, 3, *size) and got["images"].dtype == torch.float32
        assert got["masks"].shape == (B, 1, *size) and got["masks"].dtype == torch.float32
        assert got["body_segments"].shape == (B, *size) and got["body_segments"].dtype == torch.int64
        assert np.array_equal(got["body_segments"].cpu().numpy(), want_s)
        e_i = float(np.abs(got["images"].cpu().numpy().astype(np.float64) - want_i).max())
        e_m = float(np.abs(got["masks"].cpu().numpy().astype(np.float64) - want_m).max())
        worst = max(worst, e_i, e_m)
        print(f"ingest {src}->{size} B={B} geo_only={geo_only} mask={kind}: images {e_i:.2e} masks {e_m:.2e}")
        assert e_i <= BAR and e_m <= BAR, (kind, e_i, e_m)
        if kind == "zero" and not geo_only:
            assert bool((got["images"] == 1.0).all())                         # the white background, exactly
        if kind == "zero":
            assert bool((got["masks"] == -1.0).all())
    print(f"ingest {src}->{size} B={B} geo_only={geo_only}: worst {worst:.2e}")


@pytest.mark.parametrize("src,size", ALL_SHAPES)
def test_two_runs_are_bit_identical_and_an_item_ignores_its_batch(src, size):
    arrays = make_inputs(3, src[0], src[1], seed=5)
    dev = _dev(arrays)
    a, b = ing.ingest(*dev, size), ing.ingest(*dev, size)
    one = ing.ingest(*[t[:1].contiguous() for t in dev], size)
    last = ing.ingest(*[t[2:].contiguous() for t in dev], size)
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k][:1], one[k]) and torch.equal(a[k][2:], last[k]), k


def test_the_wide_path_equals_the_byte_path_bit_for_bit():
    """16x8 -> 8x4 takes the 8-byte reads and 16-byte stores; the same bytes in storage that starts one byte off an 8-byte boundary
    take the byte reads."""
    arrays = make_inputs(2, 16, 8, seed=9)
    wide = ing.ingest(*_dev(arrays), (8, 4))
    off = []
    for a in arrays:
        buf = torch.empty(a.size + 1, dtype=torch.uint8, device="cuda")
        buf[1:] = torch.from_numpy(a).cuda().flatten()
        off.append(buf[1:].view(a.shape))
    assert all(t.data_ptr() % 8 == 1 and t.is_contiguous() for t in off)
    narrow = ing.ingest(*off, (8, 4))
    for k in wide:
        assert torch.equal(wide[k], narrow[k]), k


def test_fused_and_torch_compositions_agree():
    arrays = make_inputs(2, 32, 16, seed=3)
    dev = _dev(arrays)
    a, b = ing.ingest(*dev, (16, 8)), ing.ingest_torch(*dev, (16, 8))
    assert torch.equal(a["body_segments"], b["body_segments"])
    assert float((a["images"] - b["images"]).abs().max()) <= 2 * BAR and float((a["masks"] - b["masks"]).abs().max()) <= 2 * BAR


def test_wrong_inputs_are_refused_by_name():
    rgb, mask, seg = _dev(make_inputs(1, 8, 4, seed=1))
    with pytest.raises(TypeError, match="rgb must be a uint8"):
        ing.ingest(rgb.float(), mask, seg, (4, 2))
    with pytest.raises(TypeError, match="seg must be a uint8"):
        ing.ingest(rgb, mask, seg.long(), (4, 2))
    with pytest.raises(ValueError, match="mask is on cpu"):
        ing.ingest(rgb, mask.cpu(), seg, (4, 2))
    with pytest.raises(ValueError, match="rgb is on cpu"):
        ing.ingest(rgb.cpu(), mask.cpu(), seg.cpu(), (4, 2))
    with pytest.raises(ValueError, match="mask must be contiguous"):
        ing.ingest(rgb, mask.transpose(1, 2).contiguous().transpose(1, 2), seg, (4, 2))
    with pytest.raises(ValueError, match=r"rgb must be \[B,Hs,Ws,3\]"):
        ing.ingest(rgb[..., :2].contiguous(), mask, seg, (4, 2))
    with pytest.raises(ValueError, match=r"seg must be \[B,Hs,Ws\]"):
        ing.ingest(rgb, mask, seg[:, :4].contiguous(), (4, 2))
