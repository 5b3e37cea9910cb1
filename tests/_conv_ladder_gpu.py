"""The GPU side of the convolution family's accuracy ladder (tests/_conv_arithmetic.py): run the product's path on one case in one
tier and set its errors against the bars.  Shared by tests/test_gpu_conv_ladder.py and tools/conv_accuracy_report.py."""
import contextlib
import importlib

import torch

import _conv_arithmetic as A
from conftest import rel_err

conv = importlib.import_module("3dhumangan_amd.lib.components.ops.conv")
lin = importlib.import_module("3dhumangan_amd.lib.components.ops.linear")
_lib = importlib.import_module("3dhumangan_amd._lib")
DEV = "cuda"
PLANES = {"f16x2": 2, "f16x1": 1}


@contextlib.contextmanager
def weight_planes(tier):
    """conv.AMP_WEIGHT_PLANES for the tier (tests use monkeypatch; the report tool uses this)."""
    keep = conv.AMP_WEIGHT_PLANES
    conv.AMP_WEIGHT_PLANES = PLANES.get(tier, keep)
    try:
        yield
    finally:
        conv.AMP_WEIGHT_PLANES = keep


def run(case, tier):
    """-> dict of the product's results for the case, on the CPU: y, dx, dw, db (dw, db only for the tier "f16w").
    The AMP tiers expect conv.AMP_WEIGHT_PLANES to be set by the caller (PLANES[tier])."""
    i = A.inputs_of(case)
    if tier == "f16w":
        M = case.P
        dy = i["coth"].to(DEV).permute(0, 2, 3, 1).reshape(M, case.co).contiguous()
        x = i["xh"].to(DEV).permute(0, 2, 3, 1).reshape(M, case.ci).contiguous()
        dw, db = lin.wgrad_x3(dy, x, with_bias=True)
        return dict(dw=dw.cpu()[:, :, None, None], db=db.cpu())
    w, b = i["w"].to(DEV).requires_grad_(), i["b"].to(DEV).requires_grad_()
    if case.dense:
        # the dense layer's own dispatch (ops/linear.py: _route) with the row threshold out of the way: the test shapes have a few
        # hundred rows, the route taken is the one of a training-size batch
        M = case.P
        assert lin._native_ok(case.co, case.ci)              # else _LinearX3 runs the library's GEMM, which meets every bar
        x = i["x"].to(DEV).permute(0, 2, 3, 1).reshape(M, case.ci).contiguous().requires_grad_()
        cot = i["cot"].to(DEV).permute(0, 2, 3, 1).reshape(M, case.co).contiguous()
        keep, lin.MIN_ROWS = lin.MIN_ROWS, 1
        try:
            y = lin.linear(x, w.view(case.co, case.ci), b)
        finally:
            lin.MIN_ROWS = keep
        assert type(y.grad_fn).__name__.startswith("_LinearX3"), type(y.grad_fn).__name__
        dx, dw, db = torch.autograd.grad(y, [x, w, b], cot)
        img = lambda t, C: t.detach().cpu().reshape(1, 1, M, C).permute(0, 3, 1, 2)
        return dict(y=img(y, case.co), dx=img(dx, case.ci), dw=dw.cpu(), db=db.cpu())
    half = tier != "f32"
    if half:
        assert conv.AMP_WEIGHT_PLANES == PLANES[tier]
    x = (i["xh"] if half else i["x"]).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
    cot = (i["coth"] if half else i["cot"]).to(DEV).contiguous(memory_format=torch.channels_last)
    assert conv.supported(x, w)
    y = conv.conv2d(x, w, b)
    assert y.dtype == x.dtype
    dx, dw, db = torch.autograd.grad(y, [x, w, b], cot)
    assert dx.dtype == x.dtype and dw.dtype == torch.float32 and db.dtype == torch.float32
    return dict(y=y.detach().cpu(), dx=dx.cpu(), dw=dw.cpu(), db=db.cpu())


def errors(case, tier, got, ref):
    """One number per group of the results in `got`."""
    e = {}
    for prim in ("y", "dx"):
        if prim in got:
            e.update(A.out_errors(got[prim], ref[prim], prim))
            if tier in PLANES:
                e[prim + "_share"] = A.share(got[prim], ref[prim])
    e.update(A.dw_errors(got["dw"], ref["dw"]))
    e["db"] = rel_err(got["db"], ref["db"])
    return e


def records_of(case, tier, got):
    L = A.ladder_of(case, tier)
    err = errors(case, tier, got, L["ref"])
    return [dict(case=case.name, tier=tier, group=g, measured=err[g], bar=bar, healthy_reference=L["healthy"][g],
                 headroom=bar / max(err[g], 1e-300)) for g, bar in L["bars"].items()]


def measure(case, tier):
    """-> one record per group: the measured error, the bar, the upper-bound fp32-accumulation emulation's own figure, the headroom."""
    return records_of(case, tier, run(case, tier))


@contextlib.contextmanager
def lo_plane_zeroed(tap, transposed):
    """conv.pack_stream replaced by one whose streams (of the forward, or with transposed=True of the backward-data convolution) come
    back with the lo plane of filter tap `tap` zeroed, past conv._stream_cache.  Stream layout (include/h3d.h, conv_pack_kernel; the
    same for the bf16 pair and the f16 pair): [ob][tap][chunk][ks][nt][hi|lo][h][j][e], i.e. [ob][tap][Cin / 16][NT][2][512] int16,
    with NT from h3d_conv_x3_nt_for.  D2 for fp32 activations, D4 for the two-plane AMP tier; no kernel is changed."""
    real = conv.pack_stream
    hits = []

    def wrapped(w, transposed_=False, half=False, owner=None, planes=2, nt=0):
        s = real(w.detach().clone(), transposed_, half=half, owner=None, planes=planes, nt=nt)      # a fresh tensor: never cached
        if bool(transposed_) != transposed:
            return s
        assert not (half and planes == 1), "the one-plane stream has no lo plane"
        k = w.shape[2]
        cout, cin = (w.shape[1], w.shape[0]) if transposed_ else (w.shape[0], w.shape[1])
        NT = nt or conv.tiling(cin, cout)[0]
        s = s.clone()
        s.view(cout // (32 * NT), k * k, cin // 16, NT, 2, 512)[:, tap, :, :, 1] = 0
        hits.append(1)
        return s

    conv.pack_stream = wrapped
    try:
        yield hits
    finally:
        conv.pack_stream = real
