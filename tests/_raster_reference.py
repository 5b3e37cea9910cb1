"""Brute-force float64 restatement of the mesh-rasteriser contract (include/h3d.h, h3d_mesh_rasterize; pytorch3d 0.6.2's
MeshRasterizer with faces_per_pixel=1 as the reference's preprocessor sets it up).  Test-side only: the product never imports it.

Per item: every face is tested against every pixel centre inside its (one-pixel widened) bounding box; the winner of each pixel is
the covered face with the smallest (pz, face index).  Besides the fragments it reports which pixels are "near": pixels where float
rounding of an edge or of a depth tie may decide the result --
  * some face whose box holds the pixel has |min w'| < 1e-5 (the pixel lies on an edge: of the winner, or of a face that barely
    misses it);
  * the runner-up's depth is within 1e-5 * pz of the winner's;
  * the winner's two largest w' are within 1e-5 (the argmax of the semantics lookup).
"""
import torch

NEAR = 1e-5


def pixel_centres(H, W):
    """NDC centres: +x to the left, +y up, the shorter side spans [-1, 1].  -> xs [W], ys [H] (float64)."""
    s = float(min(H, W))
    c = torch.arange(W, dtype=torch.float64)
    r = torch.arange(H, dtype=torch.float64)
    return W / s - (2 * c + 1) / s, H / s - (2 * r + 1) / s


def project(vertices, R, T, focal):
    """vertices [V,3], R [3,3], T [3] -> NDC x, y and view depth Z [V] (float64): X = v @ R + T, x = focal X / Z."""
    X = vertices.double() @ R.double() + T.double()
    return focal * X[:, 0] / X[:, 2], focal * X[:, 1] / X[:, 2], X[:, 2]


def _edge(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def rasterize_one(vertices, faces, R, T, focal, H, W):
    """One item -> pix_to_face [H,W] int64, zbuf [H,W], bary [H,W,3] (-1 on background), near [H,W] bool."""
    V = vertices.shape[0]
    faces = faces.long()
    focal = float(torch.tensor(focal, dtype=torch.float32))         # the kernel takes the focal length as an fp32 argument
    x, y, z = project(vertices, R, T, focal)
    ok_idx = ((faces >= 0) & (faces < V)).all(1)
    fi = faces.clamp(0, V - 1)
    fx, fy, fz = x[fi], y[fi], z[fi]                                            # [F,3]
    area = _edge(fx[:, 0], fy[:, 0], fx[:, 1], fy[:, 1], fx[:, 2], fy[:, 2])
    ok = ok_idx & (fz > 0).all(1) & (area.abs() > 1e-8) & torch.isfinite(area)
    s = float(min(H, W))
    c_lo = torch.ceil((W - s * fx.max(1).values - 1) / 2) - 1
    c_hi = torch.floor((W - s * fx.min(1).values - 1) / 2) + 1
    r_lo = torch.ceil((H - s * fy.max(1).values - 1) / 2) - 1
    r_hi = torch.floor((H - s * fy.min(1).values - 1) / 2) + 1
    ok &= (c_hi >= 0) & (c_lo <= W - 1) & (r_hi >= 0) & (r_lo <= H - 1)
    f_ids = torch.nonzero(ok).flatten()
    c_lo = c_lo[f_ids].clamp(0, W - 1).long()
    c_hi = c_hi[f_ids].clamp(0, W - 1).long()
    r_lo = r_lo[f_ids].clamp(0, H - 1).long()
    r_hi = r_hi[f_ids].clamp(0, H - 1).long()
    nw, nh = c_hi - c_lo + 1, r_hi - r_lo + 1
    counts = nw * nh
    pf = torch.repeat_interleave(torch.arange(len(f_ids)), counts)              # pair -> index into f_ids
    start = torch.cumsum(counts, 0) - counts
    local = torch.arange(int(counts.sum())) - start[pf]
    col = c_lo[pf] + local % nw[pf]
    row = r_lo[pf] + local // nw[pf]
    xs, ys = pixel_centres(H, W)
    px, py = xs[col], ys[row]
    f = f_ids[pf]
    X0, X1, X2 = fx[f, 0], fx[f, 1], fx[f, 2]
    Y0, Y1, Y2 = fy[f, 0], fy[f, 1], fy[f, 2]
    A = _edge(X2, Y2, X0, Y0, X1, Y1) + 1e-8
    w = torch.stack([_edge(px, py, X1, Y1, X2, Y2), _edge(px, py, X2, Y2, X0, Y0), _edge(px, py, X0, Y0, X1, Y1)], 1) / A[:, None]
    wz = w / fz[f]
    wp = wz / wz.sum(1, keepdim=True)
    covered = (wp > 0).all(1)
    pz = (wp * fz[f]).sum(1)
    pix = row * W + col
    near = torch.zeros(H * W, dtype=torch.bool)
    near[pix[wp.min(1).values.abs() < NEAR]] = True
    # winners: sort the covered pairs by (pixel, pz, face)
    cp, cz, cf, cw = pix[covered], pz[covered], f[covered], wp[covered]
    o = torch.argsort(cf, stable=True)
    o = o[torch.argsort(cz[o], stable=True)]
    o = o[torch.argsort(cp[o], stable=True)]
    cp, cz, cf, cw = cp[o], cz[o], cf[o], cw[o]
    first = torch.ones_like(cp, dtype=torch.bool)
    first[1:] = cp[1:] != cp[:-1]
    second = torch.zeros_like(first)
    second[1:] = first[:-1] & ~first[1:]
    p2f = torch.full((H * W,), -1, dtype=torch.int64)
    zbuf = torch.full((H * W,), -1.0, dtype=torch.float64)
    bary = torch.full((H * W, 3), -1.0, dtype=torch.float64)
    p2f[cp[first]] = cf[first]
    zbuf[cp[first]] = cz[first]
    bary[cp[first]] = cw[first]
    # runner-up depth tie
    tie = (cz[second] - zbuf[cp[second]]).abs() <= NEAR * zbuf[cp[second]].abs()
    near[cp[second][tie]] = True
    top2 = bary.sort(1, descending=True).values
    near |= (p2f >= 0) & ((top2[:, 0] - top2[:, 1]) < NEAR)
    return p2f.view(H, W), zbuf.view(H, W), bary.view(H, W, 3), near.view(H, W)


def rasterize(vertices, faces, R, T, focal, H, W, face_labels=None, table=None):
    """Batch: vertices [B,V,3], faces [F,3], R [B,3,3], T [B,3] (CPU) -> dict of pix_to_face [B,H,W] int64, zbuf [B,H,W],
    bary [B,H,W,3], near [B,H,W] and, when given face_labels [F] / table [V,3], the reference's derived maps
    (preprocessor.py:156-174): segments [B,H,W] int64 and semantics [B,3,H,W]."""
    outs = [rasterize_one(vertices[b].cpu(), faces.cpu(), R[b].cpu(), T[b].cpu(), float(focal), H, W)
            for b in range(vertices.shape[0])]
    p2f, zbuf, bary, near = (torch.stack(t) for t in zip(*outs))
    out = {"pix_to_face": p2f, "zbuf": zbuf, "bary": bary, "near": near}
    bg = p2f < 0
    f = p2f.clamp_min(0)
    if face_labels is not None:
        seg = face_labels.cpu().long()[f] + 2
        seg[bg] = 1
        out["segments"] = seg
    if table is not None:
        verts = faces.cpu().long()[f]                                              # [B,H,W,3]
        k = torch.argmax(bary, dim=-1, keepdim=True)
        vi = torch.gather(verts, -1, k)[..., 0]
        sem = table.cpu().double()[vi]
        sem[bg] = 0
        out["semantics"] = sem.permute(0, 3, 1, 2)
    return out
