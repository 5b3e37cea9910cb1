"""Float64 restatement of the dataset ingest (include/h3d.h, h3d_ingest): numpy, exact integer source coordinates.  Also the
published definitions of the two third-party boundaries it stands on: torchvision 0.10.1's tensor Resize is
F.interpolate(mode="bilinear", align_corners=False) without antialiasing, and cv2.resize(INTER_NEAREST) reads floor(x * src / dst)."""
import numpy as np

# (Hs, Ws) -> (H, W): the data's 2:1, odd sizes at a non-integer ratio, identity, upsampling (the edge clamps at both ends), rows wider
# than a wavefront's worth with a width off every vector multiple, a general reduction
SHAPES = [((8, 4), (4, 2)), ((7, 5), (3, 3)), ((4, 4), (4, 4)), ((3, 2), (7, 5)), ((66, 130), (33, 65)), ((37, 53), (16, 8))]


def taps(n_out, n_src):
    """-> i0, i1 (int64 [n_out]) and lambda (float64 [n_out]) of align_corners=False bilinear sampling"""
    o = np.arange(n_out, dtype=np.int64)
    num, den = np.maximum((2 * o + 1) * n_src - n_out, 0), 2 * n_out
    i0 = num // den
    return i0, np.minimum(i0 + 1, n_src - 1), (num - i0 * den).astype(np.float64) / den


def nearest(n_out, n_src):
    return np.minimum(np.arange(n_out, dtype=np.int64) * n_src // n_out, n_src - 1)


def bilinear_f64(v, size):
    """v [..., Hs, Ws] float64 -> [..., H, W]"""
    y0, y1, ly = taps(size[0], v.shape[-2])
    x0, x1, lx = taps(size[1], v.shape[-1])
    top = v[..., y0, :][..., x0] * (1 - lx) + v[..., y0, :][..., x1] * lx
    bot = v[..., y1, :][..., x0] * (1 - lx) + v[..., y1, :][..., x1] * lx
    return top * (1 - ly)[:, None] + bot * ly[:, None]


def ingest_f64(rgb, mask, seg, size, geo_only=False):
    """uint8 numpy rgb [B,Hs,Ws,3], mask, seg [B,Hs,Ws] -> images [B,3,H,W], masks [B,1,H,W] float64, body_segments [B,H,W] int64"""
    rgb, mask, seg = np.asarray(rgb), np.asarray(mask), np.asarray(seg)
    m = mask[:, None].astype(np.float64)
    u = np.where(mask[:, None] == 0, 255.0, np.moveaxis(rgb, -1, 1).astype(np.float64))
    if geo_only:
        u = np.repeat(m, 3, axis=1)
    images = bilinear_f64(u * 2.0 / 255.0 - 1.0, size)
    masks = bilinear_f64(m * 2.0 / 255.0 - 1.0, size)
    s = seg[:, nearest(size[0], seg.shape[1])][:, :, nearest(size[1], seg.shape[2])].astype(np.int64)
    return images, masks, np.where(s == 0, 1, s + 1)


def make_inputs(B, Hs, Ws, seed, mask_kind="random"):
    """seeded uint8 inputs; mask_kind: "zero", "full" (all 255) or "random" (a third 0, a third 255, the rest anything); labels 0..24"""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (B, Hs, Ws, 3), dtype=np.uint8)
    seg = rng.integers(0, 25, (B, Hs, Ws), dtype=np.uint8)
    if mask_kind == "zero":
        mask = np.zeros((B, Hs, Ws), np.uint8)
    elif mask_kind == "full":
        mask = np.full((B, Hs, Ws), 255, np.uint8)
    else:
        pick = rng.integers(0, 3, (B, Hs, Ws))
        mask = np.where(pick == 0, 0, np.where(pick == 1, 255, rng.integers(0, 256, (B, Hs, Ws)))).astype(np.uint8)
    return rgb, mask, seg
