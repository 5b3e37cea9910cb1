"""One statement of the convolution family's arithmetic on the CPU, and the accuracy bars derived from it ("accuracy
ladder").  No GPU, no kernel launch: float64 everywhere except where a kernel or a packer rounds --

    fp32 tier (csrc/conv_x3.hip MODE 0, csrc/wgrad_x3.hip HALF = false), every operand v split as
        hi = bf16(v), lo = bf16(v - hi)          weights:     conv_pack_kernel, `const __bf16 hi = (__bf16)v` / `lo = (__bf16)(v - (float)hi)`
                                                 activations: split_chunk -> split2_bf16 (x3_common.hpp), round to nearest even
        product = hi.hi + hi(W).lo(x) + lo(W).hi(x)           gemm_x3_roll: b.h x xh, b.h x xl (XLO), b.l x xh; fp32 accumulators
        weight gradient: lo(dY).hi(X) + hi(dY).lo(X) + hi(dY).hi(X)      wgrad_x3.hip Frag<false>::mul
    two-plane AMP tier (MODE 1): f16 activations as they are (fragments(): "the f16 words as loaded"), weights
        hi = f16(v), lo = f16(v - hi)            conv_pack_kernel, `const _Float16 hi = (_Float16)v` / `lo = (_Float16)(v - (float)hi)`
        product = W_hi.x + W_lo.x                             gemm_x3_roll with XLO = false
    one-plane AMP tier (MODE 2): the weight rounded to f16 once (conv_pack_kernel, f16 == 2), product = f16(W).x (PAIRK)
    f16-stored outputs: bias (and addend) added to the fp32 accumulator, then ONE rounding to f16 at the store
        (conv_x3_kernel: "round to f16 once, after the fp32 accumulation and the bias"; conv_splitk_reduce likewise)
    weight gradient from f16 operands (wgrad_x3.hip HALF = true): the f16 values THEMSELVES are multiplied -- Frag<true>::mul is one
        v_mfma_f32_32x32x16_f16 on the words read_frag took from LDS, no bf16 split anywhere -- with fp32 accumulation.  Nothing of a
        product can be lost there short of a whole k-step.  Its bar is nevertheless the x3 class's: the single defects are those of
        the bf16 split of the f16 values (exact: 8 + 3 bits), the tightest loss any instantiation of that file could suffer.

The four primitives are contractions with selectable terms over an explicit K axis, so a term can be left out in ONE loop unit:
    C (x, W)   out[p, o]    = sum_{tap, i} W[o, i, tap] x[p + tap, i]             K = taps x input channels, tap-major as the kernel's loop
    Ct(g, W)   the same contraction on the flipped, transposed weights (conv._transposed), K = taps x OUTPUT channels
    Cw(x, g)   dW[o, i, tap] = sum_p g[p, o] x[p + tap, i]                        one output block per tap, contraction over the pixels
    dense      1x1 forward over M rows and dW = dY^T X (ops/linear.py: the image is [1, C, 1, M])

Single defects (float64 sums):  D1 hi(W).lo(x) missing, D2 lo(W).hi(x) missing (weight gradient: D1 hi(dY).lo(X), D2 lo(dY).hi(X)),
D4 W_lo.x missing in the two-plane AMP tier -- each in one loop unit taken from the library's host helpers:
    forward / backward-data   "tap"    every filter tap in turn (3x3)
                              "chunk"  every channel chunk in turn, in all taps (tilings with > 1 chunk: `source` offsets the
                                       activations by the chunk index; a single iteration of the tap x chunk loop is no unit of its
                                       own -- the k-step unit is the finer one wherever it is declared)
                              "kstep"  the last 16-channel k-step of the last tap that holds a real channel (the stem's and the head's
                                       zero-padded channels multiply zeros: a defect there is invisible to anything)
                              "slice"  every K-slice's iterations (h3d_conv_x3_slices > 1)
    weight gradient           "kstep"  the last 16-row k-step of the last slice (the ragged one)
                              "slice"  every K-slice's rows (h3d_conv_wgrad_x3_slices / h3d_wgrad_x3_slices > 1)
                              "tap"    one tap's whole block (3x3)

Bars (ladder_of), from these emulations and float64 alone:
    x3 class (fp32 operands; dW from f16 operands)   (smallest single-defect error over the declared units) / 3, per group
    two-plane AMP outputs                            share metric: (smallest D4 share over the declared units) / 3
                                                     max-norm: 3 x the healthy fp32-accumulated emulation's figure
    one-plane AMP outputs                            share and max-norm: 3 x the healthy fp32-accumulated emulation's figure
    db                                               the fp32 summation bound of the kernel's own summation tree (no product to lose)
"Healthy fp32-accumulated emulation" is accumulate_fp32 / wgrad_fp32: an UPPER-BOUND model of the accumulators' rounding (one rounding
per product; the code does not say how a matrix instruction sums its 16 products), not a statement of what the hardware does.
The share of an f16-stored output is the fraction of its elements that are not f16(float64 result); the float64 result uses the
f16-rounded weights for the one-plane tier and the fp32 weights for the two-plane tier.
tests/test_conv_ladder_cpu.py checks that every case separates; tests/test_gpu_conv_ladder.py holds the kernels to the bars."""
import importlib
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

from conftest import rel_err, rel_err_channels

conv = importlib.import_module("3dhumangan_amd.lib.components.ops.conv")
_lib = importlib.import_module("3dhumangan_amd._lib")

MARGIN = 3.0
TIERS = ("f32", "f16x2", "f16x1")


# ---- roundings

def bf16(v):
    """float64 -> the nearest bf16 (ties to even), as float64.  The kernels round fp32 values: v must be exact in fp32."""
    return v.float().to(torch.bfloat16).double()


def f16(v):
    return v.float().to(torch.float16).double()


def split_bf16(v):
    """hi = bf16(v), lo = bf16(v - hi) of an fp32-exact tensor (the difference is exact in fp32, as in split2_bf16)."""
    hi = bf16(v)
    return hi, bf16(v - hi)


def split_f16(v):
    """h3d_conv_x3_pack_f16: hi = f16(v), lo = f16(v - hi)."""
    hi = f16(v)
    return hi, f16(v - hi)


def _up64(n):
    return (n + 63) // 64 * 64


# ---- the K axis of forward / backward-data

def columns(x, k):
    """x [B, C, H, W] -> [P, taps, C] float64: row p holds, per tap, the pixel the kernel's `source` lambda reads (zeros outside)."""
    B, C, H, W = x.shape
    pad = k // 2
    xp = F.pad(x.double(), (pad, pad, pad, pad))
    taps = [xp[:, :, ky:ky + H, kx:kx + W] for ky in range(k) for kx in range(k)]          # tap = ky * k + kx reads (y + ky - pad, x + kx - pad)
    return torch.stack(taps, dim=1).permute(0, 3, 4, 1, 2).reshape(B * H * W, k * k, C)


def weight_matrix(w):
    """w [Co, Ci, k, k] -> [Co, taps, Ci]"""
    co, ci, k, _ = w.shape
    return w.double().permute(0, 2, 3, 1).reshape(co, k * k, ci)


class Plan(NamedTuple):
    """The loop of one h3d_conv_x3_ex launch (conv_plan / conv_x3_any of csrc/conv_x3.hip), from the host helpers."""
    nt: int
    blocks: int
    ksc: int
    chunks: int
    n_iter: int
    slices: int            # slices that actually run
    it_per_slice: int
    occ2: bool


def conv_plan(ci, co, k, P):
    lib = _lib.load()
    nt = lib.h3d_conv_x3_nt_for(ci, co, P)
    _, _, ksc, chunks = conv.tiling(ci, co)
    if k == 1 and ksc == 8:                                  # conv_plan: 1x1 runs two workgroups per CU on 4-k-step chunks
        ksc, chunks = 4, chunks * 2
    n_iter = k * k * chunks
    asked = lib.h3d_conv_x3_slices(ci, co, k, P, nt)
    ips, nz = n_iter, 1
    if asked > 1:                                            # conv_x3_any: ceil(n_iter / it_per_slice) slices actually run
        ips = (n_iter + asked - 1) // asked
        nz = (n_iter + ips - 1) // ips
    return Plan(nt, co // (32 * nt), ksc, chunks, n_iter, nz, ips, k == 1)


def conv_units(plan, ci, k, real_ci):
    """-> {unit kind: [boolean mask over [taps, ci], ...]} of the forward / backward-data loop."""
    taps = k * k
    units = {}
    width = 16 * plan.ksc

    def iteration_mask(its):
        m = torch.zeros(taps, ci, dtype=torch.bool)
        for it in its:
            tap, chunk = divmod(it, plan.chunks)
            m[tap, chunk * width:(chunk + 1) * width] = True
        return m

    if taps > 1:
        units["tap"] = [iteration_mask(range(t * plan.chunks, (t + 1) * plan.chunks)) for t in range(taps)]
    if plan.chunks > 1:
        units["chunk"] = [iteration_mask(range(c, plan.n_iter, plan.chunks)) for c in range(plan.chunks)]
    last = (real_ci - 1) // 16                               # the last k-step that holds a real channel
    m = torch.zeros(taps, ci, dtype=torch.bool)
    m[taps - 1, 16 * last:16 * last + 16] = True
    units["kstep"] = [m]
    if plan.slices > 1:
        units["slice"] = [iteration_mask(range(z * plan.it_per_slice, min((z + 1) * plan.it_per_slice, plan.n_iter)))
                          for z in range(plan.slices)]
    return units


def contraction(cols, Wm, terms):
    """sum over K of the planes' products in float64.  cols [P, taps, C], Wm [Co, taps, C]; terms: name -> (W plane, x plane), in
    the kernel's order."""
    P, Co = cols.shape[0], Wm.shape[0]
    y = torch.zeros(P, Co, dtype=torch.float64)
    for name, (wp, xp) in terms.items():
        y = y + xp.reshape(P, -1) @ wp.reshape(Co, -1).t()
    return y


def lost(terms, drop, mask):
    """What a defect takes off the healthy sum: the term `drop` over the K positions `mask` [taps, C] -> [P, Co]."""
    wp, xp = terms[drop]
    m = mask.reshape(-1)
    return xp.reshape(xp.shape[0], -1)[:, m] @ wp.reshape(wp.shape[0], -1)[:, m].t()


def accumulate_fp32(cols, Wm, terms, plan, bias):
    """The UPPER-BOUND model of the kernels' fp32 accumulation (what the ladder calls the healthy fp32-accumulated emulation): every
    product (exact in fp32: 16- and 22-bit significands) is added to an fp32 accumulator, one rounding each, in the kernel's order:
    gemm_x3_roll issues a k-step's matrix instructions in the order of `terms`, an instruction contracts the k-step's 16 channels, the
    k-steps follow the K axis (tap, chunk, k-step).  The code does not say how a matrix instruction sums its 16 products internally;
    one rounding per product is the least precise summation an fp32 accumulator can have, a wider exact dot product rounds less
    often -- so this is not a statement of what the hardware does but a ceiling on its rounding noise, and every "3 x healthy" bar
    (the f16-stored outputs' max-norm, the one-plane tier's share) is 3 x that ceiling.  A K-slice
    keeps its own accumulator from zero (conv_x3_kernel: A.partial); conv_splitk_reduce starts from the bias and adds the slices in
    order; without slices the epilogue adds the bias to the accumulator.  -> [P, Co] float32."""
    P, Co = cols.shape[0], Wm.shape[0]
    planes = [(wp.reshape(Co, -1).float().t().contiguous(), xp.reshape(P, -1).float().t().contiguous()) for wp, xp in terms.values()]
    width = 16 * plan.ksc
    per_tap = plan.chunks * width
    parts = []
    for z in range(plan.slices):
        acc = torch.zeros(P, Co, dtype=torch.float32)
        for it in range(z * plan.it_per_slice, min((z + 1) * plan.it_per_slice, plan.n_iter)):
            tap, chunk = divmod(it, plan.chunks)
            for s in range(plan.ksc):
                k0 = tap * per_tap + chunk * width + 16 * s
                for wp, xp in planes:
                    for k in range(k0, k0 + 16):
                        acc.addcmul_(xp[k][:, None], wp[k][None, :])          # the product is exact in fp32: one rounding, fused or not
        parts.append(acc)
    if plan.slices == 1:
        return parts[0] if bias is None else parts[0] + bias.float()
    v = torch.zeros(P, Co, dtype=torch.float32) if bias is None else bias.float().expand(P, Co).clone()
    for acc in parts:
        v = v + acc
    return v


def tier_terms(tier, cols, Wm):
    """The products a tier forms, and the float64 weights its outputs are compared on."""
    if tier == "f32":
        (wh, wl), (xh, xl) = split_bf16(Wm), split_bf16(cols)
        return {"hi_hi": (wh, xh), "hi_lo": (wh, xl), "lo_hi": (wl, xh)}
    if tier == "f16x2":
        wh, wl = split_f16(Wm)
        return {"hi": (wh, cols), "lo": (wl, cols)}
    return {"hi": (f16(Wm), cols)}


DEFECTS = {"f32": {"D1": "hi_lo", "D2": "lo_hi"}, "f16x2": {"D4": "lo"}, "f16x1": {}}


# ---- cases

class Case(NamedTuple):
    name: str
    B: int
    H: int
    W: int
    ci: int
    co: int
    k: int
    dense: bool = False           # ops/linear.py: lin.linear on [M = W, ci] rows, dW on h3d_wgrad_x3
    tiers: tuple = ("f32",)
    undeclared: tuple = ()        # (primitive, unit) pairs left undeclared -- at most one per case, never "tap" or "slice"

    @property
    def P(self):
        return self.B * self.H * self.W

    @property
    def seed(self):
        return 1000 * self.ci + 10 * self.co + self.k + self.P


AMP = ("f32", "f16x2", "f16x1")
# name (B, H, W, ci, co, k): what the case reaches (tests/test_conv_ladder_cpu.py::test_the_cases_reach_every_path confirms it with
# the host helpers).  At these pixel counts h3d_conv_x3_nt_for always answers 2 -- a wider blocking needs >= 256 workgroups -- so NT = 4
# and 8 take two 1x1 cases with many pixels and K = 64: pixels x K stays under that of the 300-pixel, K = 4608 limit.
CASES = (
    # 63 pixels: ragged against the 32-pixel wave and the 128-pixel workgroup; ragged last k-step of the weight gradient (63 = 3 x 16 + 15)
    Case("c64-64-k3-p63", 1, 9, 7, 64, 64, 3, tiers=AMP),
    # two output blocks; 300 pixels = 3 workgroups, the last ragged; weight gradient in 2 K-slices of 160 + 140 rows, the last k-step ragged
    Case("c64-128-k3-p300", 2, 15, 10, 64, 128, 3, tiers=AMP),
    # two channel chunks of 128; forward and backward-data in 4 K-slices
    Case("c256-256-k3-p32", 1, 8, 4, 256, 256, 3),
    # three output blocks, three 64-channel chunks (4-k-step chunks), 6 K-slices, the last one short
    Case("c192-192-k3-p30", 1, 6, 5, 192, 192, 3),
    # K = 4608.  AMP: the k-step unit does not separate on the share metric at this K (one k-step of 288: the share of a lost W_lo.x
    # is 4.1-4.6 % against 0.9-1.1 % healthy) -- tap, chunk and slice are declared for the two-plane tier's outputs, the k-step is not
    Case("c512-512-k3-p32", 1, 8, 4, 512, 512, 3, tiers=AMP, undeclared=(("amp", "kstep"),)),
    # 1x1: the two-workgroups-per-CU instantiation, NT = 2
    Case("c64-256-k1-p63", 1, 9, 7, 64, 256, 1, tiers=AMP),
    # 64 -> 512 at 64 workgroups per output block: NT = 4 (four blocks); the weight gradient in 32 K-slices of 256 rows, the last k-step
    # ragged (8190 = 511 x 16 + 14)
    Case("c64-512-k1-p8190", 1, 91, 90, 64, 512, 1),
    # ... and at 129 workgroups per output block: NT = 8 (two blocks of 256 channels), 65 K-slices.  The thinnest separation of the set:
    # a cross term lost in the last 16 of 16471 rows is 9e-5 of the worst gradient row, 3.1 x 3 x the healthy 9.6e-6
    Case("c64-512-k1-p16471", 1, 181, 91, 64, 512, 1),
    # the stem: 3 channels zero-padded to 64
    Case("c3-128-k3-p128", 2, 8, 8, 3, 128, 3),
    # the one-channel head: the output zero-padded to 64 channels, backward-data contracts over them
    Case("c64-1-k1-p45", 1, 9, 5, 64, 1, 1),
    # dense layers (rows as a [1, C, 1, M] image): 300 rows -> weight gradient in 2 K-slices with a ragged last k-step; 768 outputs -> 12 blocks
    Case("dense-256-256-m300", 1, 1, 300, 256, 256, 1, dense=True, tiers=("f32", "f16w")),
    Case("dense-128-768-m77", 1, 1, 77, 128, 768, 1, dense=True, tiers=("f32", "f16w")),
)
CASE = {c.name: c for c in CASES}
# tiers: "f32" the fp32 path; "f16x2" / "f16x1" conv.conv2d on f16 channels-last activations with conv.AMP_WEIGHT_PLANES = 2 / 1;
# "f16w" lin.wgrad_x3 on f16 operands (the dense layers' forward under autocast is the library's GEMM, not this family)

_INPUTS, _LADDER = {}, {}


def inputs_of(case):
    """Seeded fp32 inputs (never f16-exact weights: the lo planes are non-zero), shared and never modified: x, w, b, cot (fp32) and
    xh, coth (the f16 activations / cotangents of the AMP tiers)."""
    if case.name in _INPUTS:
        return _INPUTS[case.name]
    g = torch.Generator().manual_seed(case.seed)
    x = torch.randn(case.B, case.ci, case.H, case.W, generator=g)
    w = torch.randn(case.co, case.ci, case.k, case.k, generator=g) / (case.ci * case.k * case.k) ** 0.5
    b = torch.randn(case.co, generator=g) * 0.1
    cot = torch.randn(case.B, case.co, case.H, case.W, generator=g)
    _INPUTS[case.name] = dict(x=x, w=w, b=b, cot=cot, xh=x.half(), coth=cot.half())
    return _INPUTS[case.name]


def padded(case, i, half):
    """The operands as conv.conv2d hands them to the kernels: channel counts zero-padded to multiples of 64, float64."""
    x, cot = (i["xh"], i["coth"]) if half else (i["x"], i["cot"])
    cip, cop = _up64(case.ci), _up64(case.co)
    xp = F.pad(x.double(), (0, 0, 0, 0, 0, cip - case.ci))
    gp = F.pad(cot.double(), (0, 0, 0, 0, 0, cop - case.co))
    wp = F.pad(i["w"].double(), (0, 0, 0, 0, 0, cip - case.ci, 0, cop - case.co))
    bp = F.pad(i["b"].double(), (0, cop - case.co))
    return xp, wp, bp, gp


def exact(case, half, weights="fp32"):
    """F.conv2d and its autograd in float64 -> dict y, dx, dw, db.  weights = "f16": on the f16-rounded weights (one-plane tier)."""
    i = inputs_of(case)
    x, cot = ((i["xh"], i["coth"]) if half else (i["x"], i["cot"]))
    w = f16(i["w"].double()) if weights == "f16" else i["w"].double()
    xd, wd, bd = x.double().requires_grad_(), w.clone().requires_grad_(), i["b"].double().requires_grad_()
    y = F.conv2d(xd, wd, bd, padding=case.k // 2)
    dx, dw, db = torch.autograd.grad(y, [xd, wd, bd], cot.double())
    return dict(y=y.detach(), dx=dx, dw=dw, db=db)


# ---- the weight gradient's loop

class WgradPlan(NamedTuple):
    slices: int
    rows_per_wg: int


def wgrad_plan(case):
    """Slices and rows per slice as conv._run_wgrad / linear.wgrad_x3 ask for them (conv_wgrad_any / wgrad_x3_any: rows_per_wg)."""
    lib = _lib.load()
    cip, cop = _up64(case.ci), _up64(case.co)
    if case.dense:
        s = lib.h3d_wgrad_x3_slices(case.P, case.co, case.ci)
    else:
        s = max(1, lib.h3d_conv_wgrad_x3_slices(case.B, case.H, case.W, cop, cip, case.k))
    per = (case.P + s - 1) // s
    return WgradPlan(s, (per + 15) // 16 * 16)


def wgrad_units(case, plan):
    """-> {unit kind: [(row mask [P], tap or None = every tap), ...]}"""
    P, taps = case.P, case.k * case.k
    units = {}
    bounds = [(z * plan.rows_per_wg, min((z + 1) * plan.rows_per_wg, P)) for z in range(plan.slices)]
    bounds = [(a, b) for a, b in bounds if b > a]
    a, b = bounds[-1]
    m = torch.zeros(P, dtype=torch.bool)
    m[a + (b - a - 1) // 16 * 16:b] = True                   # the last k-step of the last slice: the ragged one
    units["kstep"] = [(m, None)]
    if len(bounds) > 1:
        units["slice"] = []
        for a, b in bounds:
            m = torch.zeros(P, dtype=torch.bool)
            m[a:b] = True
            units["slice"].append((m, None))
    if taps > 1:
        units["tap"] = [(torch.ones(P, dtype=torch.bool), t) for t in range(taps)]
    return units


def wgrad(cols, g2, terms):
    """dW [Co, taps, Ci] = sum over the rows of the planes' products in float64; terms: name -> (dY plane [P, Co], X plane
    [P, taps, Ci])."""
    P, taps, Ci = cols.shape
    out = torch.zeros(g2.shape[1], taps * Ci, dtype=torch.float64)
    for name, (gp, xp) in terms.items():
        out = out + gp.t() @ xp.reshape(P, -1)
    return out.reshape(-1, taps, Ci)


def wgrad_without(healthy, terms, drop, mask, tap):
    """`healthy` [Co, taps, Ci] without the term `drop` in the rows `mask` -- of tap `tap`, or (None) of every tap."""
    gp, xp = terms[drop]
    out = healthy.clone()
    if tap is None:
        out -= (gp[mask].t() @ xp[mask].reshape(int(mask.sum()), -1)).reshape(out.shape)
    else:
        out[:, tap] -= gp[mask].t() @ xp[mask][:, tap]
    return out


def wgrad_fp32(cols, g2, terms, plan):
    """The same upper-bound model for the weight gradient (accumulate_fp32: one rounding per product): a
    slice's workgroup goes through its rows k-step after k-step (16 rows per matrix instruction), the terms in Frag::mul's order;
    h3d_wgrad_reduce then sums every fourth slice in fp32 and adds the four sums ((s0 + s1) + s2) + s3.  -> [Co, taps, Ci] float32."""
    P, taps, Ci = cols.shape
    Co, Z, rpw = g2.shape[1], plan.slices, plan.rows_per_wg
    rows = Z * rpw
    planes = [(F.pad(gp, (0, 0, 0, rows - P)).reshape(Z, rpw, Co).float(),
               F.pad(xp.reshape(P, -1), (0, 0, 0, rows - P)).reshape(Z, rpw, taps * Ci).float()) for gp, xp in terms.values()]
    acc = torch.zeros(Z, Co, taps * Ci, dtype=torch.float32)
    for j in range(0, min(rpw, (P + 15) // 16 * 16), 16):
        for gp, xp in planes:
            for r in range(j, j + 16):
                acc.addcmul_(gp[:, r, :, None], xp[:, r, None, :])
    if Z > 1:
        groups = []
        for grp in range(4):
            v = torch.zeros(Co, taps * Ci, dtype=torch.float32)
            for z in range(grp, Z, 4):
                v = v + acc[z]
            groups.append(v)
        acc = (((groups[0] + groups[1]) + groups[2]) + groups[3])[None]
    return acc[0].reshape(Co, taps, Ci)


# ---- metrics, one number per group

def out_errors(got, ref, name):
    """y / dx [B, C, H, W] -> whole-tensor max-norm and worst channel"""
    return {name: rel_err(got, ref), name + "_ch": rel_err_channels(got, ref, dim=1)}


def dw_errors(got, ref):
    """dW [Co, Ci, k, k] -> whole tensor, worst output row, worst tap"""
    co, ci = ref.shape[:2]
    return {"dw": rel_err(got, ref), "dw_row": rel_err_channels(got, ref, dim=0),
            "dw_tap": rel_err_channels(got.reshape(co, ci, -1), ref.reshape(co, ci, -1), dim=2)}


def f16_of_f64(v):
    """float64 -> the nearest f16 in ONE rounding (torch converts through float32: a double rounding near ties), as float64."""
    return torch.from_numpy(v.detach().cpu().double().numpy().astype(np.float16).astype(np.float64))


def share(stored, ref64):
    """Fraction of the f16-stored elements that are not the f16 rounding of the float64 result."""
    return float((stored.detach().cpu().double() != f16_of_f64(ref64)).double().mean())


OUT_GROUPS = {"y": ("y", "y_ch"), "dx": ("dx", "dx_ch"), "dw": ("dw", "dw_row", "dw_tap")}


def _image(rows, case, C, keep):
    """[P, Cpadded] -> [B, keep, H, W]"""
    return rows.reshape(case.B, case.H, case.W, C).permute(0, 3, 1, 2)[:, :keep]


def _outputs(case, tier):
    """The tier's emulations of y and dx: healthy in float64, healthy with fp32 accumulation, and every single defect."""
    i = inputs_of(case)
    half = tier != "f32"
    xp, wp, bp, gp = padded(case, i, half)
    cip, cop, k = _up64(case.ci), _up64(case.co), case.k
    res = {}
    for prim, act, wmat, c_in, c_out, real_in, real_out, bias in (
            ("y", xp, wp, cip, cop, case.ci, case.co, bp),
            ("dx", gp, conv._transposed(wp), cop, cip, case.co, case.ci, None)):
        plan = conv_plan(c_in, c_out, k, case.P)
        cols, Wm = columns(act, k), weight_matrix(wmat)
        terms = tier_terms(tier, cols, Wm)
        add = 0.0 if bias is None else bias
        base = contraction(cols, Wm, terms) + add
        out = {"plan": plan, "healthy": _image(base, case, c_out, real_out)}
        y32 = accumulate_fp32(cols, Wm, terms, plan, bias)
        if half:
            y32 = y32.half()                                 # ... and rounds once to f16
        out["fp32acc"] = _image(y32.double(), case, c_out, real_out)
        out["defects"] = {}
        for kind, masks in conv_units(plan, c_in, k, real_in).items():
            for n, m in enumerate(masks):
                for d, term in DEFECTS[tier].items():
                    out["defects"][f"{d}@{kind}{n}"] = _image(base - lost(terms, term, m), case, c_out, real_out)
        res[prim] = out
    return res


def _wgrad_outputs(case, half):
    """Emulations of dW: the fp32 tier's split products, or (half) the exact f16 product with the x3 class's defects."""
    i = inputs_of(case)
    xp, _, _, gp = padded(case, i, half)
    cip, cop, k = _up64(case.ci), _up64(case.co), case.k
    cols = columns(xp, k)
    g2 = gp.permute(0, 2, 3, 1).reshape(case.P, cop)
    (gh, gl), (xh, xl) = split_bf16(g2), split_bf16(cols)
    split = {"lo_hi": (gl, xh), "hi_lo": (gh, xl), "hi_hi": (gh, xh)}          # Frag<false>::mul: a.l b.h, a.h b.l, a.h b.h
    healthy = {"one": (g2, cols)} if half else split        # Frag<true>::mul: the f16 values themselves
    plan = wgrad_plan(case)

    def shape(t):
        return t.reshape(cop, k, k, cip).permute(0, 3, 1, 2)[:case.co, :case.ci].double()

    out = {"plan": plan, "healthy": shape(wgrad(cols, g2, healthy)), "fp32acc": shape(wgrad_fp32(cols, g2, healthy, plan)),
           "defects": {}}
    base = wgrad(cols, g2, split)
    for kind, units in wgrad_units(case, plan).items():
        for n, (m, tap) in enumerate(units):
            for d, term in DEFECTS["f32"].items():
                out["defects"][f"{d}@{kind}{n}"] = shape(wgrad_without(base, split, term, m, tap))
    return out


def db_bar(case, half):
    """The bias gradient is a plain fp32 sum of dY's columns (wgrad_x3_kernel: add_colsum keeps a running sum per thread over the
    slice's k-steps, 16 rows are folded through LDS, h3d_wgrad_reduce adds the slices): first-order bound of that tree,
    (k-steps per slice + 16 + slices) x 2^-24 x max_o sum_p |dY[p, o]|, relative to max |db|."""
    i = inputs_of(case)
    g = (i["coth"] if half else i["cot"]).double()
    plan = wgrad_plan(case)
    depth = plan.rows_per_wg // 16 + 16 + plan.slices
    return depth * 2.0 ** -24 * float(g.abs().sum((0, 2, 3)).max() / g.sum((0, 2, 3)).abs().max())


def _declared(case, prim, tier, name):
    kind = name.split("@")[1].rstrip("0123456789")
    scope = "amp" if (tier == "f16x2" and prim in ("y", "dx")) else prim
    return (scope, kind) not in case.undeclared and (prim, kind) not in case.undeclared


def ladder_of(case, tier):
    """-> dict: ref {y, dx, dw, db} (the float64 results the tier is compared with); bars {group: bar}; healthy {group: the healthy
    fp32-accumulated emulation's figure (accumulate_fp32: the upper-bound model)}; x3 {group: the defect-free emulation summed in float64
    against float64}; defects {group: {defect name: figure}} (declared units only); plans."""
    key = (case.name, tier)
    if key in _LADDER:
        return _LADDER[key]
    half = tier != "f32"
    ref = exact(case, half, "f16" if tier == "f16x1" else "fp32")
    bars, healthy, defects, x3 = {}, {}, {}, {}
    plans = {}
    if tier != "f16w":
        emu = _outputs(case, tier)
        for prim in ("y", "dx"):
            e, r = emu[prim], ref[prim]
            plans[prim] = e["plan"]
            healthy.update(out_errors(e["fp32acc"], r, prim))
            x3.update(out_errors(e["healthy"], r, prim))
            table = {n: out_errors(o, r, prim) for n, o in e["defects"].items() if _declared(case, prim, tier, n)}
            if tier == "f32":
                for g in OUT_GROUPS[prim]:
                    defects[g] = {n: t[g] for n, t in table.items()}
                    bars[g] = min(defects[g].values()) / MARGIN
            else:
                s = prim + "_share"
                healthy[s] = share(e["fp32acc"], r)
                for g in OUT_GROUPS[prim]:
                    bars[g] = MARGIN * healthy[g]
                if tier == "f16x2":
                    defects[s] = {n: share(f16_of_f64(o), r) for n, o in e["defects"].items() if _declared(case, prim, tier, n)}
                    bars[s] = min(defects[s].values()) / MARGIN
                else:
                    bars[s] = MARGIN * healthy[s]
    w = _wgrad_outputs(case, half)
    plans["dw"] = w["plan"]
    healthy.update(dw_errors(w["fp32acc"], ref["dw"]))
    x3.update(dw_errors(w["healthy"], ref["dw"]))
    table = {n: dw_errors(o, ref["dw"]) for n, o in w["defects"].items() if _declared(case, "dw", tier, n)}
    for g in OUT_GROUPS["dw"]:
        defects[g] = {n: t[g] for n, t in table.items()}
        bars[g] = min(defects[g].values()) / MARGIN
    i = inputs_of(case)
    bars["db"] = db_bar(case, half)
    healthy["db"] = rel_err((i["coth"] if half else i["cot"]).float().sum((0, 2, 3)), ref["db"])
    _LADDER[key] = dict(ref=ref, bars=bars, healthy=healthy, defects=defects, x3=x3, plans=plans)
    return _LADDER[key]
