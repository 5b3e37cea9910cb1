"""The compositing step of the six kernels restated on the CPU, the edge rays that drive them, a list of single defects and the
accuracy bars derived from both ("compositing edge rays").  No GPU, no kernel.

    edge_rays(S)             named rays: opaque samples on tile boundaries, empty rays, softplus's threshold, equal depths ...
    composite(...)           csrc/composite.hpp's step in tiles of `width` lanes (segments for S < width, carries for S > width),
                             in float64 (== the oracle) or float32 ("the reference's arithmetic in the kernels' order"), healthy
                             or with ONE defect of FORWARD_DEFECTS
    composite_backward(...)  the phases of ray_integrate_bwd_kernel (csrc/train_ops.hip), healthy or with ONE of BACKWARD_DEFECTS
    bars(S, width, mode)     10 x the float32 restatement's error against the float64 oracle on these rays, floor 1e-6

tests/test_composite_edges_cpu.py checks that every defect exceeds 3 x its bar on some named ray wherever it applies and that
the float32 restatement stays a factor 3 under; tests/test_gpu_composite_edges.py holds the kernels to the bars."""
import functools

import torch

import h3d_oracle as O

B = 2
MODES = tuple((c, lb, wb) for c in ("relu", "softplus") for lb in (False, True) for wb in (False, True))
BAR_FACTOR, BAR_FLOOR, MARGIN = 10.0, 1e-6, 3.0
OPAQUE_AT = (31, 32, 63, 64)                 # besides 0, S // 2 and S - 2: the lanes on both sides of a 32- and a 64-lane tile boundary
SOFTPLUS_VALUES = (19.999, 20.0, 20.001, 25.0, -25.0, -90.0, -104.0, 0.5)
FORWARD_QUANTITIES, BACKWARD_QUANTITIES = ("weights", "depth", "feats"), ("dsigma", "dfeats")


# ---- the rays

def is_opaque(name):
    return name.startswith("opaque_at_") or name == "five_opaque"


def edge_rays(S):
    """-> (names, sigma_pattern [R, S], z [R, S]), float32, deterministic in S.  z = 11 + 0.25 (r mod 3) + s / S except on `zero_delta`.  Every
    opaque ray is directly followed by a semi-transparent one (`after_<name>`), the list ends on a ray that is not opaque (so
    the rule survives a roll), and |sigma_last| >= 5 on every ray."""
    g = torch.Generator().manual_seed(4000 + S)
    z0 = 11.0 + torch.arange(S, dtype=torch.float64) / S
    big = 300.0 * S
    rays = []

    def uniform(lo, hi):
        return lo + (hi - lo) * torch.rand(S, generator=g, dtype=torch.float64)

    def add(name, sig, last, z=None):
        sig = sig.clone()
        sig[-1] = last
        rays.append((name, sig, z0 if z is None else z))

    def add_opaque(name, ks, last):
        sig = uniform(0.5, 2.5)
        for k in ks:
            sig[k] = big
        add(name, sig, last)
        add("after_" + name, uniform(0.5, 2.5), 5.0 if len(rays) % 4 == 1 else -5.0)

    for k in sorted({k for k in (0, S // 2, S - 2) + OPAQUE_AT if 0 <= k < S - 1}):
        add_opaque(f"opaque_at_{k}", (k,), 5.0)
        add_opaque(f"opaque_at_{k}_lastneg", (k,), -5.0)
    if S >= 8:
        add_opaque("five_opaque", range(1, 6), 5.0)
    add("empty", uniform(-3.5, -0.5), -5.0)
    add("empty_then_last_hit", uniform(-3.5, -0.5), 5.0)
    if S >= 2:
        add("dense_lastneg", uniform(0.0, 0.2 * S), -5.0)
        add("dense_lastpos", uniform(0.0, 0.2 * S), 5.0)
        add("thin_lastneg", torch.full((S,), 1e-6, dtype=torch.float64), -5.0)
        thr = torch.tensor([SOFTPLUS_VALUES[i % len(SOFTPLUS_VALUES)] for i in range(S)], dtype=torch.float64)
        add("softplus_thr", thr, -30.0)
        add("softplus_thr_scaled", thr * (S / 20.0), -max(30.0 * S / 20.0, 5.0))
    add("softplus_tail", torch.full((S,), -25.0, dtype=torch.float64), -22.0)
    if S >= 4:
        k = S // 2
        sig, z = uniform(0.5, 2.5), z0.clone()
        sig[k] = big
        z[k + 1] = z[k]
        add("zero_delta", sig, 5.0, z)
    names = [r[0] for r in rays]
    # neighbouring rays start at different depths (delta stays 1 / S): a z_last taken from another ray of the tile shows
    z = torch.stack([r[2] + 0.25 * (i % 3) for i, r in enumerate(rays)])
    return names, torch.stack([r[1] for r in rays]).float(), z.float()


@functools.lru_cache(maxsize=None)
def case_inputs(S, C=7, only=None):
    """The stand-alone kernels' inputs for the rays of edge_rays(S) (only: a tuple of names, those rays alone), shared and never
    modified: B = 2 items, item 1 = the list rolled by one ray.  -> dict: names [B][R], field [B,R,S,C+1] (features randn, density 0.05 randn), z, noise (= the pattern)
    [B,R,S,1] and the cotangents pf [B,R,C], pd [B,R,1], pw [B,R,S,1]."""
    names, pat, z = edge_rays(S)
    if only is not None:
        keep = [names.index(n) for n in only]
        names, pat, z = list(only), pat[keep], z[keep]
    R = len(names)
    g = torch.Generator().manual_seed(S * 1000 + C)
    field = torch.randn(B, R, S, C + 1, generator=g)
    field[..., -1] *= 0.05
    pf, pd, pw = (torch.randn(s, generator=g) for s in ((B, R, C), (B, R, 1), (B, R, S, 1)))
    roll = lambda t: torch.stack([t, t.roll(1, 0)]).unsqueeze(-1)
    return dict(names=[names, names[-1:] + names[:-1]], field=field, z=roll(z), noise=roll(pat), pf=pf, pd=pd, pw=pw, R=R)


# ---- the step

FORWARD_DEFECTS = ("carry_reset", "sumw_carry_dropped", "tile_product_early", "scan_unsegmented", "z_last_of_tile", "last_delta_previous",
                   "softplus_no_threshold", "bg_after_fixup", "depth_without_bg", "inclusive_weight")
BACKWARD_DEFECTS = ("no_epsilon", "suffix_carry_dropped", "no_a_last", "no_go_sum")


def segmented(S, width):
    """S < width puts several rays into a tile only for the sample counts the fused renders accept (a power of two >= 8); the
    stand-alone kernels keep one ray per tile at every S."""
    return 8 <= S < width and S & (S - 1) == 0


def applies(defect, S, width, mode):
    """Where a defect changes the arithmetic at all.  The tile product is consumed only by a ray that continues in a next tile,
    so reading it a lane early applies for S > width like the carries; bg read after the fix-up differs from bg only when the
    fix-up ran (last_back) and bg is used (white_back); the unthresholded softplus overflows only where zero_delta (S >= 4)
    multiplies its inf by 0 -- elsewhere inf gives the alpha = 1 the healthy code gives."""
    clamp, last_back, white_back = mode
    # with last_back and without white_back the last sample's own weight and gradient cancel (w_last + bg = 1 - the others):
    # a carry that reaches only that sample (S = width + 1) cannot show
    hidden_last = last_back and not white_back
    if defect in ("carry_reset", "tile_product_early"):
        return S > width and not (hidden_last and (S - 1) % width == 0)
    if defect == "sumw_carry_dropped":
        return S > width
    if defect in ("scan_unsegmented", "z_last_of_tile"):
        return segmented(S, width)
    if defect == "last_delta_previous":
        return S >= 2 and not hidden_last
    if defect == "softplus_no_threshold":
        return clamp == "softplus" and S >= 4
    if defect == "bg_after_fixup":
        return last_back and white_back
    if defect == "suffix_carry_dropped":
        return S > 64 and not (hidden_last and (S - 1) % 64 == 0)
    if defect == "no_a_last":
        return last_back
    if defect == "no_go_sum":
        return white_back
    if defect == "no_epsilon":
        return S >= 2
    if defect == "inclusive_weight":                       # a one-sample ray with last_back has the weight 1 whatever the product
        return S >= 2 or white_back or not last_back
    return True


def _density(x, clamp, defect):
    if clamp != "softplus":
        return torch.relu(x)
    if defect == "softplus_no_threshold":
        return torch.log1p(torch.exp(x.float())).to(x.dtype)        # in fp32: inf above 88
    return torch.where(x > 20, x, torch.log1p(torch.exp(x.clamp(max=20.0))))


def _density_deriv(x, clamp):
    if clamp != "softplus":
        return (x > 0).to(x.dtype)
    return torch.where(x > 20, torch.ones_like(x), 1.0 / (1.0 + torch.exp(-x)))


def _samples(sigma, z, noise, clamp, dtype, defect=None):
    """composite_sample for every sample: -> z, delta, sg, e, alpha, f (all [N, S])."""
    z = z.to(dtype)
    sg = sigma.to(dtype) if noise is None else sigma.to(dtype) + noise.to(dtype)
    last = torch.full_like(z[:, :1], 1e9)
    if defect == "last_delta_previous" and z.shape[1] >= 2:
        last = z[:, -1:] - z[:, -2:-1]
    delta = torch.cat([z[:, 1:] - z[:, :-1], last], dim=1)
    e = torch.exp(-delta * _density(sg, clamp, defect))
    alpha = 1.0 - e
    eps = 0.0 if defect == "no_epsilon" else torch.tensor(1e-12, dtype=dtype)
    return z, delta, sg, e, alpha, (1.0 - alpha) + eps


def composite(sigma, z, feats, clamp, last_back, white_back, width, dtype, defect=None, noise=None):
    """sigma, z [N, S] (noise [N, S]: added to sigma in `dtype`, as the kernels do), feats [N, S, C] -> (features [N, C], depth
    [N], weights [N, S]) by composite_step<width>: S < width (a power of two) puts width / S rays into one tile as segments,
    S > width carries T, sum(w) and sum(w z) of one ray across its tiles; a ragged last tile holds lanes without a sample
    (alpha = 0, f = 1) and takes z_last from the ray (the stand-alone kernel's form -- the fused ones never see one)."""
    assert defect is None or defect in FORWARD_DEFECTS, defect
    N, S = sigma.shape
    zz, _, _, _, alpha, f = _samples(sigma, z, noise, clamp, dtype, defect)
    seg = segmented(S, width)
    rpt, T = (width // S, 1) if seg else (1, -(-S // width))
    seglen = S if seg else width
    Sp, Np = T * width // rpt, -(-N // rpt) * rpt
    G = Np // rpt

    def lanes(x, fill):
        p = torch.full((Np, Sp), fill, dtype=dtype)
        p[:N, :S] = x
        return p.reshape(G, rpt, T, Sp // T).permute(0, 2, 1, 3).reshape(G, T, width)

    al, fl, zl = lanes(alpha, 0.0), lanes(f, 1.0), lanes(zz, 0.0)
    lane = torch.arange(width)
    sl = lane & (seglen - 1)
    scan_sl, scan_len = (lane, width) if defect == "scan_unsegmented" else (sl, seglen)
    cT, cW, cD = torch.ones(G, width, dtype=dtype), torch.zeros(G, width, dtype=dtype), torch.zeros(G, width, dtype=dtype)
    ws = []
    for t in range(T):
        incl = fl[:, t]
        off = 1
        while off < scan_len:
            u = torch.cat([incl[:, :off], incl[:, :-off]], dim=1)              # __shfl_up: lanes below `off` get their own value
            incl = torch.where(scan_sl >= off, incl * u, incl)
            off <<= 1
        excl = torch.cat([incl[:, :1], incl[:, :-1]], dim=1)
        excl = torch.where(scan_sl == 0, torch.ones_like(excl), excl)
        if defect == "inclusive_weight":
            excl = incl
        w = al[:, t] * (cT * excl)
        wsum, dsum = w, w * zl[:, t]
        off = seglen >> 1
        while off > 0:
            wsum, dsum = wsum + wsum[:, lane ^ off], dsum + dsum[:, lane ^ off]
            off >>= 1
        tp = incl[:, width - 2 if defect == "tile_product_early" else width - 1].unsqueeze(1)
        cT = torch.ones_like(cT) if defect == "carry_reset" else cT * tp
        cW = wsum if defect == "sumw_carry_dropped" else cW + wsum
        cD = cD + dsum
        ws.append(w)
    end = (S - 1) - (T - 1) * width if not seg else S - 1                     # the ray_end lanes of the last tile: sl == end
    if seg:
        z_last = zl[:, T - 1][:, (torch.full_like(lane, width - 1) if defect == "z_last_of_tile" else lane | (seglen - 1))]
    else:
        z_last = torch.cat([zz[:, -1], torch.ones(Np - N, dtype=dtype)]).unsqueeze(1).expand(G, width)
    bg = 1.0 - cW
    depth = cD if defect == "depth_without_bg" else cD + bg * z_last
    ray_end = (sl == end).expand(G, width)
    if last_back:
        ws[-1] = torch.where(ray_end, ws[-1] + bg, ws[-1])

    def rays(x):                                                               # [G, T, width] -> [N, S]
        return x.reshape(G, T, rpt, Sp // T).permute(0, 2, 1, 3).reshape(Np, Sp)[:N, :S]

    weights = rays(torch.stack(ws, dim=1))
    per_ray = lambda x: x.reshape(G, rpt, width // rpt)[:, :, end].reshape(Np)[:N]      # the value on each ray's ray_end lane
    bg_r, depth_r = per_ray(bg), per_ray(depth)
    out = (weights.unsqueeze(-1) * feats.to(dtype)).sum(1)
    if white_back:
        add = 1.0 - weights.sum(1) if defect == "bg_after_fixup" else bg_r
        out = out + add.unsqueeze(-1)
    return out, depth_r, weights


def composite_backward(sigma, z, feats, g_feats, g_depth, g_weights, clamp, last_back, white_back, dtype, defect=None, noise=None):
    """The phases of ray_integrate_bwd_kernel: sigma, z [N, S], feats [N, S, C], cotangents g_feats [N, C], g_depth [N],
    g_weights [N, S] -> (d sigma [N, S], d feats [N, S, C])."""
    assert defect is None or defect in BACKWARD_DEFECTS, defect
    N, S = sigma.shape
    # 1: the forward scan again
    zz, delta, sg, e, alpha, f = _samples(sigma, z, noise, clamp, dtype, defect)
    T = torch.cumprod(torch.cat([torch.ones_like(f[:, :1]), f[:, :-1]], dim=1), dim=1)
    w = alpha * T
    da = delta * e * _density_deriv(sg, clamp)
    bg = 1.0 - w.sum(1)
    gO, gD, gW, F = g_feats.to(dtype), g_depth.to(dtype), g_weights.to(dtype), feats.to(dtype)
    # 2: a_s = sum_c gO[c] F[s][c]
    a = (F * gO.unsqueeze(1)).sum(-1)
    # 3: dL/dw_s, suffix sums in chunks of 64 from the far end, dL/dsigma_s
    g = a + gW
    if last_back and defect != "no_a_last":
        g = g - g[:, -1:].clone()
    if white_back and defect != "no_go_sum":
        g = g - gO.sum(-1, keepdim=True)
    g = g + gD.unsqueeze(1) * (zz - zz[:, -1:])
    gw = g * w
    after = torch.zeros_like(gw)
    carry = torch.zeros(N, 1, dtype=dtype)
    for c0 in reversed(range(0, S, 64)):
        chunk = gw[:, c0:c0 + 64]
        incl = chunk.flip(1).cumsum(1).flip(1)
        after[:, c0:c0 + 64] = carry + incl - chunk
        if defect != "suffix_carry_dropped":
            carry = carry + incl[:, :1]
    dsig = (g * T - after / f) * da
    # 4: dF[s][c] = w'_s gO[c]
    wp = w.clone()
    if last_back:
        wp[:, -1] = wp[:, -1] + bg
    return dsig, wp.unsqueeze(-1) * gO.unsqueeze(1)


# ---- error measures: one number per ray

def _nonfinite_is_inf(err, got):
    bad = ~torch.isfinite(got.double().reshape(got.shape[0], -1)).all(1)
    return torch.where(bad | torch.isnan(err), torch.full_like(err, float("inf")), err)


def forward_errors(got, ref, z, feat_scale):
    """got, ref = (features [N, C], depth [N], weights [N, S]), z [N, S], feat_scale [N] = max |features of the ray's samples|
    -> {quantity: error per ray [N]}: weights absolute (they lie in [0, 1]), depth over z_last, features over max(1, feat_scale);
    a non-finite output counts as infinite."""
    (gf, gd, gw), (rf, rd, rw) = ([t.detach().cpu().double() for t in got], [t.double() for t in ref])
    N = rw.shape[0]
    z_last = z.double().reshape(N, -1)[:, -1]
    out = {"weights": (gw.reshape(N, -1) - rw.reshape(N, -1)).abs().amax(1),
           "depth": (gd.reshape(N) - rd.reshape(N)).abs() / z_last,
           "feats": (gf - rf).abs().amax(1) / feat_scale.double().clamp_min(1.0)}
    return {k: _nonfinite_is_inf(v, g) for (k, v), g in zip(out.items(), (gw, gd, gf))}


def backward_errors(got, ref):
    """got, ref = (d sigma [N, S], d feats [N, S, C]) -> {quantity: error per ray}: |diff| over max(max |ref| on the ray,
    1e-2 max |ref| of the case)."""
    out = {}
    for name, g, r in zip(BACKWARD_QUANTITIES, got, ref):
        g, r = g.detach().cpu().double().reshape(r.shape[0], -1), r.double().reshape(r.shape[0], -1)
        scale = torch.maximum(r.abs().amax(1), 1e-2 * r.abs().max()).clamp_min(1e-300)
        out[name] = _nonfinite_is_inf((g - r).abs().amax(1) / scale, g)
    return out


def worst(err, names):
    """{quantity: per-ray errors [B * R]} -> {quantity: (largest error, "item:name" of the ray)}."""
    flat = [f"{b}:{n}" for b in range(len(names)) for n in names[b]]
    return {q: (float(v.max()), flat[int(v.argmax())]) for q, v in err.items()}


# ---- the float64 reference, the restatements on the shared inputs, the bars

def _flat(i, S):
    N = B * i["R"]
    return i["field"][..., -1].reshape(N, S), i["z"].reshape(N, S), i["field"][..., :-1].reshape(N, S, -1), i["noise"].reshape(N, S)


@functools.lru_cache(maxsize=None)
def oracle_forward(S, mode, C=7, only=None):
    """O.ray_integration in float64 on case_inputs(S, C), flattened to rays: (features [N, C], depth [N], weights [N, S])."""
    i = case_inputs(S, C, only)
    f, d, w = O.ray_integration(i["field"].double(), i["z"].double(), i["noise"].double(), *mode)
    N = B * i["R"]
    return f.reshape(N, -1), d.reshape(N), w.reshape(N, S)


@functools.lru_cache(maxsize=None)
def oracle_backward(S, mode, C=7, only=None):
    """Autograd through the float64 oracle with the cotangents of case_inputs: (d sigma [N, S], d feats [N, S, C])."""
    i = case_inputs(S, C, only)
    fr = i["field"].double().requires_grad_(True)
    of, od, ow = O.ray_integration(fr, i["z"].double(), i["noise"].double(), *mode)
    ((of * i["pf"]).sum() + (od * i["pd"]).sum() + (ow * i["pw"]).sum()).backward()
    N = B * i["R"]
    return fr.grad[..., -1].reshape(N, S), fr.grad[..., :-1].reshape(N, S, -1)


def restated_forward(S, width, mode, dtype, defect=None, C=7, only=None):
    """composite() item by item (every item's rays start at lane 0 of a tile, as in the fused kernels), flattened to rays."""
    i = case_inputs(S, C, only)
    R = i["R"]
    sigma, z, feats, noise = _flat(i, S)
    parts = [composite(sigma[b * R:(b + 1) * R], z[b * R:(b + 1) * R], feats[b * R:(b + 1) * R], *mode, width, dtype, defect,
                       noise[b * R:(b + 1) * R]) for b in range(B)]
    return tuple(torch.cat(p) for p in zip(*parts))


def restated_backward(S, mode, dtype, defect=None, C=7, only=None):
    i = case_inputs(S, C, only)
    sigma, z, feats, noise = _flat(i, S)
    N = B * i["R"]
    return composite_backward(sigma, z, feats, i["pf"].reshape(N, -1), i["pd"].reshape(N), i["pw"].reshape(N, S), *mode, dtype, defect, noise)


def feat_scale(S, C=7, only=None):
    i = case_inputs(S, C, only)
    return i["field"][..., :-1].abs().reshape(B * i["R"], -1).amax(1)


def forward_errors_of(got, S, mode, C=7, only=None):
    return forward_errors(got, oracle_forward(S, mode, C, only), case_inputs(S, C, only)["z"].reshape(-1, S), feat_scale(S, C, only))


@functools.lru_cache(maxsize=None)
def float32_errors(S, width, mode, C=7, only=None):
    """The float32 restatement against the float64 oracle on the rays of case_inputs(S, C, only): {quantity: (error, ray)}."""
    names = case_inputs(S, C, only)["names"]
    err = dict(forward_errors_of(restated_forward(S, width, mode, torch.float32, None, C, only), S, mode, C, only))
    if S <= 2048:
        err.update(backward_errors(restated_backward(S, mode, torch.float32, None, C, only), oracle_backward(S, mode, C, only)))
    return worst(err, names)


@functools.lru_cache(maxsize=None)
def bars(S, width, mode, C=7, only=None):
    """{quantity: bar}: 10 x the float32 restatement's error against the float64 oracle on these same rays, floor 1e-6.  From
    the reference alone, never from a kernel; the factor covers another rounding order (the tree scan against the linear one,
    the sums of the feature channels) and the device's expf / log1pf."""
    return {q: max(BAR_FLOOR, BAR_FACTOR * e) for q, (e, _) in float32_errors(S, width, mode, C, only).items()}


# ---- the fused renders: the same rays through `noise`, a field whose own density stays within +-0.05

FUSED_SIGMA = 0.05
ENGINE_WIDTH = {"f16x2": 32, "f16x3": 32, "f16x2t": 64, "f16x3t": 64, "f32": 64}


def _rays_flat(out, S):
    f, d, w = out
    return f.reshape(-1, f.shape[-1]), d.reshape(-1), w.reshape(-1, S)


@functools.lru_cache(maxsize=None)
def fused_case(S, hidden, feature, geo=False):
    """Inputs of net.render for the rays of edge_rays(S), shared and never modified: the weights of random_state(hidden, feature,
    seed = S + hidden) (tests/test_gpu_field.py) with the density head scaled so that the float64 oracle's own density stays within
    +-0.05 -- the pattern decides every ray.  -> dict: state, seed, names, R, pts, geo, freq, phase, z, noise, field (float64
    oracle, [B,R,S,F+4]), sigma_max, feat_scale [B * R], feat_max.  geo: the 31 geometry features are the oracle's own for a synthetic body
    (cond, the harness of tests/test_gpu_fused_geo.py) instead of random numbers."""
    import _field_arithmetic as A
    names, pat, z = edge_rays(S)
    R = len(names)
    N = R * S
    seed = S + hidden
    state, _ = A.make_state(hidden, feature, seed)
    g = torch.Generator().manual_seed(R * 1000 + S)
    pts = torch.rand(B, N, 3, generator=g) * 2 - 1
    cond = None
    if geo:
        import importlib
        cond = importlib.import_module("3dhumangan_amd.synthetic").make_conditions(B, n_vertices=500, seed=R)
        geo = O.geo_features(pts, cond["skeletons_xyz"], cond["vertices"], cond["tpose_vertices"], cond["fk_matrices"], cond["lbs_weights"], False)
    else:
        geo = torch.rand(B, N, 31, generator=g) * 2 - 1
    freq = torch.randn(B, 4 * hidden, generator=g) * 0.5
    phase = torch.randn(B, 4 * hidden, generator=g)
    dirs = torch.zeros(B, N, 3, dtype=torch.float64)
    dirs[..., 2] = -1

    def oracle_field():
        sd = {k: v.double() for k, v in state.items()}
        return O.neural_field(sd, pts.double(), freq.double(), phase.double(), geo.double(), dirs, 0.7).reshape(B, R, S, -1)

    gain = 0.9 * FUSED_SIGMA / float(oracle_field()[..., -1].abs().max())
    for k in ("neural_field.sigma_layer.weight", "neural_field.sigma_layer.bias"):
        state[k] = state[k] * gain
    field = oracle_field()
    sigma_max = float(field[..., -1].abs().max())
    assert sigma_max <= FUSED_SIGMA
    roll = lambda t: torch.stack([t, t.roll(1, 0)]).unsqueeze(-1)
    return dict(state=state, seed=seed, names=[names, names[-1:] + names[:-1]], R=R, pts=pts, geo=geo, freq=freq, phase=phase, z=roll(z),
                noise=roll(pat), field=field, cond=cond, sigma_max=sigma_max, feat_scale=field[..., :-1].abs().reshape(B * R, -1).amax(1),
                feat_max=float(field[..., :-1].abs().max()))


@functools.lru_cache(maxsize=None)
def fused_reference(S, hidden, feature, mode, geo=False):
    """The oracle field followed by O.ray_integration in float64, flattened to rays."""
    c = fused_case(S, hidden, feature, geo)
    return _rays_flat(O.ray_integration(c["field"], c["z"].double(), c["noise"].double(), *mode), S)


def fused_errors(got, S, hidden, feature, mode, geo=False):
    c = fused_case(S, hidden, feature, geo)
    return forward_errors(_rays_flat(got, S), fused_reference(S, hidden, feature, mode, geo), c["z"].reshape(-1, S), c["feat_scale"])


@functools.lru_cache(maxsize=None)
def engine_ladder(hidden, feature):
    """The field engines' own bars for a field of these widths (tests/_field_arithmetic.py, ladder_of on an unfused field case with
    random_state's initialisation): {"x3" | "x2": {group: max-norm relative bar}}."""
    import _field_arithmetic as A
    case = A.Case(f"edges-field-h{hidden}-f{feature}", "field", hidden, feature, seed=hidden, gseed=77, N=77)
    return A.ladder_of(case)["bars"]


@functools.lru_cache(maxsize=None)
def fused_bars(S, hidden, feature, engine, mode, geo=False):
    """{quantity: bar} of a fused render: weights and depth get bars(S, width, mode) plus the change of the float64 result when
    every density moves by the engine's density bar (both signs, the larger); the features the larger of that and the engine's own
    colour / feature bar.  From the reference and the CPU emulations alone."""
    import _field_arithmetic as A
    c = fused_case(S, hidden, feature, geo)
    ladder = engine_ladder(hidden, feature)["x2" if A.engine_class(engine) == "x2" else "x3"]
    eps = ladder["sigma"] * c["sigma_max"]
    ref = fused_reference(S, hidden, feature, mode, geo)
    moved = {q: 0.0 for q in FORWARD_QUANTITIES}
    for sign in (1.0, -1.0):
        field = c["field"].clone()
        field[..., -1] += sign * eps
        out = _rays_flat(O.ray_integration(field, c["z"].double(), c["noise"].double(), *mode), S)
        for q, v in forward_errors(out, ref, c["z"].reshape(-1, S), c["feat_scale"]).items():
            moved[q] = max(moved[q], float(v.max()))
    base = bars(S, ENGINE_WIDTH[engine], mode)
    bar = {q: base[q] + moved[q] for q in FORWARD_QUANTITIES}
    bar["feats"] = max(bar["feats"], max(ladder["rgb"], ladder["feat"]) * max(1.0, c["feat_max"]))
    return bar


# ---- every defect against the bars

def defect_ratios(S, width, backward):
    """-> [(mode, defect, ratio, quantity, ray)]: for every mode and every defect that applies there, the float32 restatement with
    that one defect against the float64 oracle -- its largest error / bar over the quantities, and the ray it occurs on."""
    names = case_inputs(S)["names"]
    out = []
    for mode in MODES:
        bar = bars(S, width, mode)
        for defect in FORWARD_DEFECTS + (BACKWARD_DEFECTS if backward else ()):
            if not applies(defect, S, width, mode):
                continue
            if defect in FORWARD_DEFECTS:
                err = forward_errors_of(restated_forward(S, width, mode, torch.float32, defect), S, mode)
            else:
                err = backward_errors(restated_backward(S, mode, torch.float32, defect), oracle_backward(S, mode))
            ratio, q, ray = max((e / bar[q], q, ray) for q, (e, ray) in worst(err, names).items())
            out.append((mode, defect, ratio, q, ray))
    return out
