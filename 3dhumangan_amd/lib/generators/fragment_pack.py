"""The matrix-core weight formats of the inference engines, as plain functions on dense [n_out, n_in] matrices.

  pack_matrix        fp32 MFMA B fragments (the fp32 engines; same bytes as h3d_pack_matrix)
  pack_stream_bf16   bf16 / f16 hi + lo weight-stream stages (the split-product engines)
  pack_stream_x2     f16 hi fragments + block-scaled fp6 records (the x2 engines)
  pack_tiles_x2c     the x2 tier of the LDS-resident engine: pack_stream_x2 without the stored hi codes, tile-major

The split formats share two things, written once here: the accumulator-register order of the K dimension (acc_columns)
and the zero-padded staging matrix with its columns in k-slot order (_staged)."""
import torch


def pack_matrix(w_out_in, KB, NT):
    """[n_out, n_in] (reference layout) -> packed [NT*KB*64*4] fp32, same bytes as h3d_pack_matrix."""
    n_out, n_in = w_out_in.shape
    wt = torch.zeros(8 * KB, 32 * NT, dtype=torch.float32, device=w_out_in.device)
    wt[:n_in, :n_out] = w_out_in.t().float()
    return wt.view(KB, 2, 4, NT, 32).permute(3, 0, 1, 4, 2).contiguous().flatten()


def _pad(v, n):
    out = torch.zeros(n, dtype=torch.float32, device=v.device)
    out[: v.numel()] = v.flatten().float()
    return out


def acc_columns(KS, device=None):
    """Feature index of every k-slot [ks][h][e] (k-step, lane half, element) in accumulator-register order:
    32*(ks//2) + (e & 3) + 8*(2*(ks & 1) + (e >> 2)) + 4*h, so that a lane's accumulator registers are its B-fragment elements
    (csrc/field_pack.hpp: acc_k) -> int64 [16 KS]."""
    ks = torch.arange(KS, device=device).view(KS, 1, 1)
    hh = torch.arange(2, device=device).view(1, 2, 1)
    e = torch.arange(8, device=device).view(1, 1, 8)
    return (32 * (ks // 2) + (e & 3) + 8 * (2 * (ks & 1) + (e >> 2)) + 4 * hh).reshape(-1)


def _staged(w_out_in, KS, NT, acc_order):
    """[n_out, n_in] -> fp32 [32 NT, 16 KS], zero padded, columns in k-slot order [ks][h][e]: accumulator-register order
    (every matrix whose input is a previous accumulator), otherwise the natural order 16*ks + 8*h + e, which already is."""
    n_out, n_in = w_out_in.shape
    wp = torch.zeros(32 * NT, 16 * KS, dtype=torch.float32, device=w_out_in.device)
    wp[:n_out, :n_in] = w_out_in.float()
    return wp[:, acc_columns(KS, wp.device)] if acc_order else wp


def _fragments(t, KS, NT):
    """[N, K] in k-slot order -> [KS, NT, 64 lanes, 8]; lane = 32*h + j, element e: n = 32 nt + j, k-slot (ks, h, e)."""
    return t.view(NT, 32, KS, 2, 8).permute(2, 0, 3, 1, 4).reshape(KS, NT, 64, 8)


def pack_stream_bf16(w_out_in, KS, NT, acc_order=True, dtype=torch.bfloat16):
    """[n_out, n_in] -> bf16 (or `dtype`) hi/lo weight-stream stages [KS][NT][2][64][8] (as int16 bit patterns); K in
    accumulator-register order (every matrix of the x3 synthesis engine, csrc/synthesis_x3.hip) or in natural order."""
    wp = _staged(w_out_in, KS, NT, acc_order)
    hi = wp.to(dtype)
    lo = (wp - hi.float()).to(dtype)
    return torch.stack([_fragments(hi, KS, NT), _fragments(lo, KS, NT)], dim=2).contiguous().view(torch.int16).flatten()


def e2m3_codes(v):
    """fp32 tensor -> 6-bit e2m3 codes (int64): round-to-nearest-even on the code grid, saturating at 7.5 (the same
    arithmetic as csrc/field_pack.hpp: e2m3_code and as v_cvt_scalef32_pk32_fp6_f16)."""
    a = v.abs().clamp(max=7.5)
    step = torch.where(a < 2, torch.full_like(a, 0.125), torch.where(a < 4, torch.full_like(a, 0.25), torch.full_like(a, 0.5)))
    q = torch.round(a / step) * step
    code = torch.where(q < 2, q * 8, torch.where(q < 4, 16 + (q - 2) * 4, 24 + (q - 4) * 2)).to(torch.int64)
    return code | ((v < 0).to(torch.int64) << 5)


def pack_stream_x2(w_out_in, KS, NT, acc_order=True, dense=True):
    """[n_out, n_in] -> weight-stream stages of the x2 engines, [KS][NT][1 KiB f16 hi fragment | 1 KiB half of the fp6
    records] as int16 bit patterns (csrc/x3_common.hpp).  K in accumulator-register order.  The fp6 record of a lane
    (output row n = 32 nt + lane % 32, half h = lane // 32) and K-tile T holds, for the lane's 16 input features (k-steps
    2T, 2T+1), slots 0-15 = q6(hi * alpha), slots 16-31 = q6(lo * 2^12 * alpha) (alpha the largest power of two with
    max|hi| * alpha <= 7.5 and no saturated lo code), six bits per slot, then the e8m0 byte of 1 / alpha four times: 7 dwords.
    Code dwords 0-3 travel in the even k-step's stage, 16 B per lane.  The odd k-step's KiB holds, `dense` (the register
    engine, csrc/x3_common.hpp: gemm_x2_roll reads it with one 64-bit and one 32-bit LDS load per lane, bank-conflict-free in
    this layout), code dwords 4-5 as [64 lanes][8 B], the scale dwords as [64 lanes][4 B] and 256 B of zeros; otherwise (the
    LDS-resident engine, which pulls 16 B per lane straight from L2) dwords 4-7 = codes, scale, scale at 16 B per lane."""
    assert KS % 2 == 0
    wp = _staged(w_out_in, KS, NT, acc_order)
    dev = wp.device
    hi16 = wp.to(torch.float16)
    hi = hi16.float()
    lo = wp - hi
    N, T = 32 * NT, KS // 2
    hi_frag = _fragments(hi16, KS, NT).contiguous().view(torch.int16)
    # slot groups: [N, T, j, h, e] -> [N, T, h, (j, e)]
    grp = lambda t: t.view(N, T, 2, 2, 8).permute(0, 1, 3, 2, 4).reshape(N, T, 2, 16)
    gh, gl = grp(hi), grp(lo)
    mx = gh.abs().amax(dim=-1)
    ea = torch.where(mx > 0, torch.floor(torch.log2(7.5 / mx.clamp_min(1e-38))), torch.zeros_like(mx)).clamp(-100, 100)
    # no saturated lo code: one step for normal hi values (|lo| <= 2^-11 |hi|), several when hi is an f16 subnormal
    lo_max = gl.abs().amax(dim=-1) * 4096.0
    need = torch.where(lo_max > 0, torch.ceil(torch.log2(lo_max.clamp_min(1e-38) / 7.5)), torch.full_like(lo_max, -200.0))
    ea = torch.minimum(ea, -need).clamp(-100, 100)
    alpha = torch.exp2(ea).unsqueeze(-1)
    codes = e2m3_codes(torch.cat([gh * alpha, gl * alpha * 4096.0], dim=-1))    # [N, T, 2, 32]
    c = codes.view(N, T, 2, 8, 4)
    b0 = c[..., 0] | ((c[..., 1] & 3) << 6)
    b1 = (c[..., 1] >> 2) | ((c[..., 2] & 15) << 4)
    b2 = (c[..., 2] >> 4) | (c[..., 3] << 2)
    rec = torch.zeros(N, T, 2, 32, dtype=torch.uint8, device=dev)
    rec[..., :24] = torch.stack([b0, b1, b2], dim=-1).reshape(N, T, 2, 24).to(torch.uint8)
    rec[..., 24:32] = (127 - ea).to(torch.uint8).unsqueeze(-1)      # dword 6, and again in dword 7 (the register engine reads it there)
    # [N = (nt, j32), T, h, (half, 16 B)] -> stage [ks = 2T + half][nt][lane = 32 h + j32][16 B]
    rec = rec.view(NT, 32, T, 2, 2, 16).permute(2, 4, 0, 3, 1, 5).reshape(KS, NT, 64 * 16)
    if dense:
        odd = rec[1::2].reshape(T, NT, 64, 16)
        rec[1::2] = torch.cat([odd[..., 0:8].reshape(T, NT, 512), odd[..., 8:12].reshape(T, NT, 256),
                               odd.new_zeros(T, NT, 256)], dim=-1)
    out = torch.empty(KS, NT, 2, 1024, dtype=torch.uint8, device=dev)
    out[:, :, 0] = hi_frag.reshape(KS, NT, 64 * 8).view(torch.uint8).reshape(KS, NT, 1024)
    out[:, :, 1] = rec
    return out.view(torch.int16).flatten()


def pack_tiles_x2c(w_out_in, KS, NT, acc_order=True):
    """[n_out, n_in] -> the x2 tier's weights of the LDS-resident engine in the x2c format (csrc/x3t_common.hpp), tile-major
    [NT][K-tile T][3 KiB] as int16 bit patterns: +0 the f16 hi fragment of k-step 2T, +1024 the lo record -- 16 B per lane: the
    16 six-bit codes of lo * 2^12 * alpha (dwords 3-5 of the fp6 A operand) and a dword holding the lane's block-scale byte --, +2048 the hi
    fragment of k-step 2T + 1.  The 16 hi codes (dwords 0-2) are not stored: the kernel converts them from the hi fragments
    (v_cvt_scalef32_pk32_fp6_f16, the lane's scale), so a weight costs 3 bytes of the vector-memory path instead of 4."""
    st = pack_stream_x2(w_out_in, KS, NT, acc_order=acc_order, dense=False).view(torch.uint8).view(KS, NT, 2, 64, 16)
    ev, od = st[0::2], st[1::2]                                   # [T, NT, plane, 64 lanes, 16 B]
    rec = torch.cat([ev[:, :, 1, :, 12:16], od[:, :, 1, :, 0:9], torch.zeros_like(od[:, :, 1, :, 0:3])], dim=-1)   # dwords 3 | 4, 5 | scale byte, 0, 0, 0
    out = torch.stack([ev[:, :, 0], rec, od[:, :, 0]], dim=2)     # [T, NT, 3, 64, 16]
    return out.permute(1, 0, 2, 3, 4).contiguous().view(torch.int16).flatten()       # [NT][T][3][64][16 B]
