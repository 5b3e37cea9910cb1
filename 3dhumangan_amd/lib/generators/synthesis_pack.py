"""Host-side preparation of the SPADE synthesis network for the fused HIP kernel (csrc/synthesis.hip).

Everything here is *exact* algebra on the reference's eval-mode forward
(lib/generators/map3d_generator.py:58-97, lib/components/map3d_layers.py:176-238):

  static, once per weight version (build_plan):
    conv weight  = weight_orig / (u . (W v))                (nn.utils.spectral_norm in eval, stored u/v)
    BatchNorm    = x * sc + sh,  sc = weight * rsqrt(running_var + eps),  sh = bias - running_mean * sc
    all matrices packed into MFMA B-fragment order (include/h3d.h)
  per forward (per_forward_tables), a handful of tiny library GEMMs on the device:
    shared-MLP pre-activations of the fixed style for all SPADEs:   fixed @ Ws^T + bs
    constant-style SPADEs -> per-(sample, channel) affine  ab = (sc * (1+gamma), sh * (1+gamma) + beta)
    per-pixel-style SPADEs -> low-resolution maps  G = feature_maps @ Ws^T  (the 1x1 conv commutes with the
    bilinear resize that follows it) and the per-sample constant cst
"""
import ctypes
import os

import torch

from ... import _lib
from ..._stages import stage

SHARED = 128
EPS_BN = 1e-5


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


def _grow(t, n):
    """t with zero rows appended up to n of them."""
    return torch.cat([t, t.new_zeros((n - t.shape[0],) + tuple(t.shape[1:]))], dim=0)


class _Table:
    """A flat fp32 table under construction: add() appends a tensor and returns its offset in floats.  align = 4 pads every
    entry to whole float4s (the x3 / x3t kernels read their tables 16 bytes at a time), align = 1 leaves the fp32 engine's blob
    as it is."""

    def __init__(self, align):
        self.align, self.chunks, self.floats = align, [], 0

    def add(self, t):
        o = self.floats
        t = t.flatten().float()
        pad = (-t.numel()) % self.align
        if pad:
            t = torch.cat([t, t.new_zeros(pad)])
        self.chunks.append(t)
        self.floats += t.numel()
        return o

    def cat(self):
        return torch.cat(self.chunks).contiguous()


def _add_coord_input(tab, desc, w_in, b_in, HdP):
    """The coordinate input's tables: w_in [C, 2] as two vectors, b_in; their offsets go into the descriptor."""
    desc.w_in = tab.add(torch.cat([_pad(w_in[:, 0], HdP), _pad(w_in[:, 1], HdP)]))
    desc.b_in = tab.add(_pad(b_in, HdP))


def _rgb_table(wr, br, HdP):
    """A ToRGB layer's table: the three weight rows padded to HdP, then the bias padded to 4."""
    return torch.cat([_pad(wr[0], HdP), _pad(wr[1], HdP), _pad(wr[2], HdP), _pad(br, 4)])


def _copy_layout(src, dst):
    """The fields of the base descriptor that every engine's descriptor shares: per block skip / to_rgb, per SPADE its style
    kind and its indices into the per-forward tables."""
    for k in range(src.n_blocks):
        dst.block[k].skip, dst.block[k].to_rgb = src.block[k].skip, src.block[k].to_rgb
        for s in range(2):
            d, so = dst.block[k].spade[s], src.block[k].spade[s]
            d.pixel_style, d.g_offset, d.cst_index, d.ab_index = so.pixel_style, so.g_offset, so.cst_index, so.ab_index


class SpadeDesc(ctypes.Structure):
    _fields_ = [("pixel_style", ctypes.c_int32), ("g_offset", ctypes.c_int32), ("cst_index", ctypes.c_int32),
                ("ab_index", ctypes.c_int32), ("w_gamma", ctypes.c_int64), ("w_beta", ctypes.c_int64),
                ("vec", ctypes.c_int64), ("w_conv", ctypes.c_int64), ("b_conv", ctypes.c_int64)]


class BlockDesc(ctypes.Structure):
    _fields_ = [("spade", SpadeDesc * 2), ("skip", ctypes.c_int32), ("to_rgb", ctypes.c_int32),
                ("w_rgb", ctypes.c_int64)]


class SynthDesc(ctypes.Structure):
    _fields_ = [("n_blocks", ctypes.c_int32), ("C", ctypes.c_int32), ("w_in", ctypes.c_int64),
                ("b_in", ctypes.c_int64), ("block", BlockDesc * 16)]


class SynthesisPlan:
    """Packed weights + launch descriptor + the small dense matrices used by per_forward_tables."""

    def __init__(self, state, prefix, input_prefix, n_blocks, mod_blocks, map3d_mode, device):
        g = lambda k: state[k].detach().to(device=device, dtype=torch.float32)
        if map3d_mode not in ("all", "mixed", "isolated"):
            raise ValueError("invalid map3d_mode")
        self.mode = map3d_mode
        self.n_blocks = n_blocks
        C, Cin = g(f"{prefix}.network.m3d_0.conv_0.weight_orig").shape[:2]
        F = g(f"{prefix}.network.m3d_0.spade_0.mlp_shared.0.weight").shape[1]
        if Cin > C or g(f"{input_prefix}.network.0.weight").shape[:2] != (Cin, 2):
            raise NotImplementedError("the fused synthesis engines take the coordinate input alone, input_dim <= hidden_dim wide "
                                      "(a wider input, the label map or the latent as inputs run layer by layer: "
                                      "differentiable.synthesis_forward)")
        # input_dim < hidden_dim (feature_dim narrower than the network): block 0's input side is zero-padded to C, exactly --
        # w_in / b_in rows zero (the in-kernel sin(0) = 0), the first SPADE's scale / shift, gamma / beta rows and biases zero on
        # the padded channels (its table holds 1 + gamma's bias: that entry is zero as well), conv_0's padded K columns zero.
        # Every engine then sees an ordinary C-wide network.
        self.C, self.F, self.Cin = C, F, Cin
        HdP = (C + 31) // 32 * 32
        self.HdP = HdP
        NT, KBH = HdP // 32, HdP // 8
        tab = _Table(1)
        add = tab.add
        desc = SynthDesc()
        desc.n_blocks, desc.C = n_blocks, C
        self._w_in = _grow(g(f"{input_prefix}.network.0.weight").reshape(Cin, 2), C)
        self._b_in = _grow(g(f"{input_prefix}.network.0.bias"), C)
        _add_coord_input(tab, desc, self._w_in, self._b_in, HdP)
        ws_all, bs_all, self.pixel_ids, self.const_ids = [], [], [], []
        self._raw = []          # per SPADE: dict of dense fp32 tensors (consumed by the x3 builder)
        self._rgb = {}
        wg_c, bg_c, wb_c, bb_c, sc_c, sh_c = [], [], [], [], [], []
        for k in range(n_blocks):
            pixel = map3d_mode == "all" or k in mod_blocks
            bd = desc.block[k]
            bd.skip = int(k >= n_blocks // 2)
            bd.to_rgb = int(k >= n_blocks // 2 - 1)
            for s in range(2):
                sp = f"{prefix}.network.m3d_{k}.spade_{s}"
                cv = f"{prefix}.network.m3d_{k}.conv_{s}"
                sid = 2 * k + s
                ws_all.append(g(sp + ".mlp_shared.0.weight").reshape(SHARED, F))
                bs_all.append(g(sp + ".mlp_shared.0.bias"))
                sc = g(sp + ".first_norm.weight") * torch.rsqrt(g(sp + ".first_norm.running_var") + EPS_BN)
                sh = g(sp + ".first_norm.bias") - g(sp + ".first_norm.running_mean") * sc
                cin = Cin if sid == 0 else C
                wgam = g(sp + ".mlp_gamma.weight").reshape(cin, SHARED)
                wbet = g(sp + ".mlp_beta.weight").reshape(cin, SHARED)
                bgam, bbet = g(sp + ".mlp_gamma.bias"), g(sp + ".mlp_beta.bias")
                w = g(cv + ".weight_orig").reshape(C, cin)
                sigma = torch.dot(g(cv + ".weight_u"), torch.mv(w, g(cv + ".weight_v")))
                if cin < C:
                    sc, sh, wgam, wbet, bbet = (_grow(t, C) for t in (sc, sh, wgam, wbet, bbet))
                    bgam = torch.cat([bgam, bgam.new_full((C - cin,), -1.0)])      # 1 + bias is what the tables hold
                    w = torch.cat([w, w.new_zeros(C, C - cin)], dim=1)
                self._raw.append(dict(pixel=pixel, conv_w=w / sigma, conv_b=g(cv + ".bias"), wgam=wgam, bgam=bgam,
                                      wbet=wbet, bbet=bbet, sc=sc, sh=sh))
                d = bd.spade[s]
                d.w_conv = add(pack_matrix(w / sigma, KBH, NT))
                d.b_conv = add(_pad(g(cv + ".bias"), HdP))
                if pixel:
                    d.pixel_style = 1
                    d.g_offset = SHARED * len(self.pixel_ids)
                    d.cst_index = len(self.pixel_ids)
                    self.pixel_ids.append(sid)
                    d.w_gamma = add(pack_matrix(wgam, SHARED // 8, NT))
                    d.w_beta = add(pack_matrix(wbet, SHARED // 8, NT))
                    d.vec = add(torch.cat([_pad(bgam + 1.0, HdP), _pad(bbet, HdP), _pad(sc, HdP), _pad(sh, HdP)]))
                else:
                    d.pixel_style = 0
                    d.ab_index = len(self.const_ids)
                    self.const_ids.append(sid)
                    wg_c.append(wgam.t().contiguous()); bg_c.append(bgam)
                    wb_c.append(wbet.t().contiguous()); bb_c.append(bbet)
                    sc_c.append(sc); sh_c.append(sh)
            if bd.to_rgb:
                tr = f"{prefix}.to_rgbs.m3d_{k}.linear"
                wr = g(tr + ".weight").reshape(3, C)
                self._rgb[k] = (wr, g(tr + ".bias"))
                bd.w_rgb = add(_rgb_table(*self._rgb[k], HdP))
        self.desc = desc
        self.blob = tab.cat()
        self.ws_all = torch.stack(ws_all)                                 # [2*nb, 128, F]
        self.bs_all = torch.stack(bs_all)                                 # [2*nb, 128]
        pix = torch.tensor(self.pixel_ids, dtype=torch.long, device=device)
        self.pix_index = pix
        self.con_index = torch.tensor(self.const_ids, dtype=torch.long, device=device)
        # [F, 128 * n_pixel]: low-res shared conv for every per-pixel SPADE in one GEMM
        self.ws_pixel_t = (self.ws_all[pix].reshape(-1, F).t().contiguous() if len(self.pixel_ids) else None)
        self.ws_pixel = (self.ws_all[pix].reshape(-1, F).contiguous() if len(self.pixel_ids) else None)       # [128 np, F] rows = outputs
        if self.const_ids:
            self.wg_c, self.bg_c = torch.stack(wg_c), torch.stack(bg_c)   # [nc,128,C], [nc,C]
            self.wb_c, self.bb_c = torch.stack(wb_c), torch.stack(bb_c)
            self.sc_c, self.sh_c = torch.stack(sc_c), torch.stack(sh_c)
        self.g_channels = SHARED * len(self.pixel_ids)
        self.device = device
        self._x3 = None
        self._x2 = None
        self._x3t = None
        # Arithmetic engine: "f16x2" one f16 product + one block-scaled fp6 product (both cross terms) per contraction,
        # register-resident activations (C <= 256); "bf16x3" split-bf16 matrix cores, register-resident activations (C <= 256);
        # "bf16x3t" split-bf16 matrix cores, LDS-resident activations (C <= 448: MAP3DBN 384, MAP3DBN512L 420);
        # "f32" fp32 matrix cores (anything else).  Opt-in reduced-precision tiers on the bf16x3t kernel (NOT within the
        # 1e-3 budget; BASELINE config 5's "fp16 MFMA path"): "f16w2t" weights f16 hi + lo, activations one f16 value (two
        # products); "f16x1t" plain f16 products.
        default = ("f16x2" if self.x2_supported() else "bf16x3" if self.x3_supported()
                   else ("f16x2t" if self.x2_weights_in_range() else "bf16x3t") if self.x3t_supported() else "f32")
        self._x2_flag = None          # int32 [B] on the device: the x2 engine's per-item range / monitor flags of the LAST run (see run())
        self.x2_guard = os.environ.get("H3D_SYNTH_GUARD", "1") != "0"
        # Sampled error monitor of the x2 register engine (round 5): every forward re-evaluates `x2_monitor_tiles` of its
        # 128-pixel tiles per image on the fp32-class engine and raises the item's device flag (the range guard's) when a sampled
        # pixel differs by more than `x2_monitor_tol` of the image's channel maximum -- the bf16 engine behind it then redoes THAT
        # ITEM (round 6: one flag per item; rounds 4-5 redid the batch, so an image depended on its batch mates).
        # The tolerance carries the sampling factor (round 6): over 192 bench-size images the full-image maximum of |x2 - x3| was
        # 1.2 - 1.65 times the maximum over a 16-tile sample (profiles/r5_x2_fullimage_error.txt: 9.6e-4 full vs 6.6e-4 sampled,
        # 5.7e-4 vs 3.5e-4, 5.2e-4 vs 3.2e-4), so a sample is held to X2_MONITOR_BUDGET / X2_SAMPLING_FACTOR = 6e-4 / 1.7 = 3.5e-4:
        # an item whose sample passes has a full-image error of <= 6e-4 by that ratio, 40 % inside the 1e-3 budget.
        # H3D_SYNTH_MONITOR=0 switches the monitor off, H3D_SYNTH_MONITOR_TOL / _TILES override the two numbers.
        self.x2_monitor = os.environ.get("H3D_SYNTH_MONITOR", "1") != "0"
        self.x2_monitor_tol = float(os.environ.get("H3D_SYNTH_MONITOR_TOL", self.X2_MONITOR_BUDGET / self.X2_SAMPLING_FACTOR))
        self.x2_monitor_tiles = int(os.environ.get("H3D_SYNTH_MONITOR_TILES", "32"))
        self._x2_monitor_buf = None   # (scratch image [B,3,H,W], per-item sampled error [B]) of the last run
        self.engine = os.environ.get("H3D_SYNTH_PRECISION", default)

    X2_MONITOR_BUDGET = 6e-4      # full-image |x2 - x3| an item may carry, relative to its channel maximum (budget 1e-3)
    X2_SAMPLING_FACTOR = 1.7      # largest measured (full-image maximum) / (sampled maximum) of that error, rounded up

    # ------------------------------------------------------------------ split-bf16 ("x3") engine
    def x3_supported(self):
        """C <= 256, per-pixel styles only in a leading run of whole blocks before the first skip block, every block after
        the first skip block has a skip connection too (csrc/synthesis_x3.hip)."""
        if self.C > 256:
            return False
        seen_skip, seen_const = False, False
        for k in range(self.n_blocks):
            if seen_skip and not self.desc.block[k].skip:
                return False
            seen_skip = seen_skip or bool(self.desc.block[k].skip)
            px = [bool(self.desc.block[k].spade[s].pixel_style) for s in range(2)]
            if seen_skip and any(px):
                return False
            if any(px) and (seen_const or not all(px)):          # per-pixel styles: a leading run of whole blocks
                return False
            seen_const = seen_const or not any(px)
        # LDS budget of csrc/synthesis_x3.hip (tables, per-sample tables, descriptor copy, 4-deep weight ring): the kernel's own count
        return self._x3_fits(False)

    def _x3_fits(self, x2):
        x3 = self.build_x3(bool(x2))           # the plan that would run: an x2 plan with ToRGB heads has its own table set
        return self._x3_lds_bytes(x3, (3 if x3["heads"] else 1) if x2 else 0) <= 160 * 1024

    def _x3_lds_bytes(self, x3, kind):
        return _lib.load().h3d_synthesis_x3_lds_bytes(x3["tables"].numel(), len(self.const_ids), len(self.pixel_ids), self.C, kind)

    # |x| < 2^15 keeps both f16 planes of the x2 arithmetic finite (hi = f16(x); lo * 2^12 <= ulp(hi) * 2^11): csrc/synthesis_x3.hip
    X2_LIMIT = 32768.0

    def x2_weights_in_range(self):
        """Every matrix the x2 engines carry as f16 hi planes (conv, gamma, beta) is finite and below the f16 planes' range.
        A network whose spectral-norm vectors were never normalised (sigma = u . W v can be tiny) fails this and
        stays on the bf16 engines, which have the fp32 exponent range."""
        for raw in self._raw:
            for k in ("conv_w", "wgam", "wbet"):
                w = raw[k]
                if not bool(torch.isfinite(w).all()) or float(w.abs().max()) >= self.X2_LIMIT:
                    return False
        return True

    def x2_supported(self):
        """x3_supported with room for the x2 kernel's fifth ring buffer and weights inside the f16 planes' range."""
        if not self.x3_supported():
            return False
        return self._x3_fits(True) and self.x2_weights_in_range()

    @staticmethod
    def pack_stream_bf16(w_out_in, KS, NT, acc_order=True, dtype=torch.bfloat16):
        """[n_out, n_in] -> bf16 (or `dtype`) hi/lo weight-stream stages [KS][NT][2][64][8] (as int16 bit patterns).

        acc_order (every matrix of the x3 synthesis engine: its inputs are always previous accumulators): the K dimension
        runs in accumulator-register order, feature of k-slot (h, e) of k-step ks =
        32*(ks//2) + (e & 3) + 8*(2*(ks & 1) + (e >> 2)) + 4*h, so that a lane's accumulator registers are its B-fragment
        elements (csrc/synthesis_x3.hip); otherwise the natural order 16*ks + 8*h + e."""
        n_out, n_in = w_out_in.shape
        dev = w_out_in.device
        wp = torch.zeros(32 * NT, 16 * KS, dtype=torch.float32, device=dev)
        wp[:n_out, :n_in] = w_out_in.float()
        if acc_order:
            ks = torch.arange(KS, device=dev).view(KS, 1, 1)
            hh = torch.arange(2, device=dev).view(1, 2, 1)
            e = torch.arange(8, device=dev).view(1, 1, 8)
            k = 32 * (ks // 2) + (e & 3) + 8 * (2 * (ks & 1) + (e >> 2)) + 4 * hh          # [KS, 2, 8]
            wp = wp[:, k.reshape(-1)]
        hi = wp.to(dtype)
        lo = (wp - hi.float()).to(dtype)

        def frag(t):        # [N, K] -> [KS, NT, 64 lanes, 8]; lane = 32*h + j, element e: n = 32nt + j, k-slot (ks, h, e)
            return t.view(NT, 32, KS, 2, 8).permute(2, 0, 3, 1, 4).reshape(KS, NT, 64, 8)

        return torch.stack([frag(hi), frag(lo)], dim=2).contiguous().view(torch.int16).flatten()

    @staticmethod
    def e2m3_codes(v):
        """fp32 tensor -> 6-bit e2m3 codes (int64): round-to-nearest-even on the code grid, saturating at 7.5 (the same
        arithmetic as csrc/field_pack.hpp: e2m3_code and as v_cvt_scalef32_pk32_fp6_f16)."""
        a = v.abs().clamp(max=7.5)
        step = torch.where(a < 2, torch.full_like(a, 0.125), torch.where(a < 4, torch.full_like(a, 0.25), torch.full_like(a, 0.5)))
        q = torch.round(a / step) * step
        code = torch.where(q < 2, q * 8, torch.where(q < 4, 16 + (q - 2) * 4, 24 + (q - 4) * 2)).to(torch.int64)
        return code | ((v < 0).to(torch.int64) << 5)

    @classmethod
    def pack_stream_x2(cls, w_out_in, KS, NT, acc_order=True, dense=True):
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
        n_out, n_in = w_out_in.shape
        dev = w_out_in.device
        wp = torch.zeros(32 * NT, 16 * KS, dtype=torch.float32, device=dev)
        wp[:n_out, :n_in] = w_out_in.float()
        ks = torch.arange(KS, device=dev).view(KS, 1, 1)
        hh = torch.arange(2, device=dev).view(1, 2, 1)
        e = torch.arange(8, device=dev).view(1, 1, 8)
        k = 32 * (ks // 2) + (e & 3) + 8 * (2 * (ks & 1) + (e >> 2)) + 4 * hh          # [KS, 2, 8]
        if acc_order:
            wp = wp[:, k.reshape(-1)]                                                  # columns now [ks][h][e]
        # (natural order, k = 16 ks + 8 h + e, already is [ks][h][e])
        hi16 = wp.to(torch.float16)
        hi = hi16.float()
        lo = wp - hi
        N, T = 32 * NT, KS // 2
        hi_frag = hi16.view(NT, 32, KS, 2, 8).permute(2, 0, 3, 1, 4).reshape(KS, NT, 64, 8).contiguous().view(torch.int16)
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
        codes = cls.e2m3_codes(torch.cat([gh * alpha, gl * alpha * 4096.0], dim=-1))    # [N, T, 2, 32]
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

    @classmethod
    def pack_tiles_x2c(cls, w_out_in, KS, NT, acc_order=True):
        """[n_out, n_in] -> the x2 tier's weights of the LDS-resident engine in the x2c format (round 6, csrc/x3t_common.hpp), tile-major
        [NT][K-tile T][3 KiB] as int16 bit patterns: +0 the f16 hi fragment of k-step 2T, +1024 the lo record -- 16 B per lane: the
        16 six-bit codes of lo * 2^12 * alpha (dwords 3-5 of the fp6 A operand) and a dword holding the lane's block-scale byte --, +2048 the hi
        fragment of k-step 2T + 1.  The 16 hi codes (dwords 0-2) are not stored: the kernel converts them from the hi fragments
        (v_cvt_scalef32_pk32_fp6_f16, the lane's scale), so a weight costs 3 bytes of the vector-memory path instead of 4."""
        st = cls.pack_stream_x2(w_out_in, KS, NT, acc_order=acc_order, dense=False).view(torch.uint8).view(KS, NT, 2, 64, 16)
        T = KS // 2
        ev, od = st[0::2], st[1::2]                                   # [T, NT, plane, 64 lanes, 16 B]
        rec = torch.cat([ev[:, :, 1, :, 12:16], od[:, :, 1, :, 0:9], torch.zeros_like(od[:, :, 1, :, 0:3])], dim=-1)   # dwords 3 | 4, 5 | scale byte, 0, 0, 0
        out = torch.stack([ev[:, :, 0], rec, od[:, :, 0]], dim=2)     # [T, NT, 3, 64, 16]
        return out.permute(1, 0, 2, 3, 4).contiguous().view(torch.int16).flatten()       # [NT][T][3][64][16 B]

    # ------------------------------------------------------------------ split-bf16 engine with LDS-resident activations
    def x3t_supported(self):
        """C <= 448, per-pixel styles only in blocks without skip connection, no plain block after the first skip block
        (csrc/synthesis_x3t.hip)."""
        if _lib.load().h3d_synthesis_x3t_tiles(self.C) < 0:
            return False
        seen_skip = False
        for k in range(self.n_blocks):
            blk = self.desc.block[k]
            if seen_skip and not blk.skip:
                return False
            seen_skip = seen_skip or bool(blk.skip)
            if blk.skip and (blk.spade[0].pixel_style or blk.spade[1].pixel_style):
                return False
        return True

    # engine -> (element type of the hi halves, dtype code, products code of h3d_synthesis_x3t_tier, weight format)
    X3T_TIERS = {"bf16x3t": (torch.bfloat16, 0, 3, "x3"), "f16x2t": (torch.float16, 1, 4, "x2"),
                 "f16w2t": (torch.float16, 1, 2, "x3"), "f16x1t": (torch.float16, 1, 1, "x3")}

    def build_x3t(self, dtype=torch.bfloat16, fmt="x3"):
        """Weights as bf16 (f16 for the reduced-precision tiers) hi/lo MFMA A fragments, tile-major [tile][k-step][hi|lo][64 lanes][8] (conv matrices with K in
        accumulator-register order, gamma / beta in natural order: their input is assembled from memory), fp32 tables
        padded to the engine's width 32 * tiles, and a descriptor whose w_* offsets are BYTES into the fragment blob and
        whose vec / b_conv / w_rgb / w_in / b_in offsets are FLOATS into the tables."""
        if self._x3t is None:
            self._x3t = {}
        if (dtype, fmt) in self._x3t:
            return self._x3t[(dtype, fmt)]
        C = self.C
        NT = _lib.load().h3d_synthesis_x3t_tiles(C)
        HdP, KS = 32 * NT, 2 * NT
        wchunks, woff, tab = [], [0], _Table(4)
        add_t = tab.add

        def add_w(w_out_in, ks, acc_order):
            o = woff[0]
            if fmt == "x2":        # x2c: f16 hi fragments + lo records, [NT][K-tile][3 KiB]
                wchunks.append(self.pack_tiles_x2c(w_out_in, ks, NT, acc_order=acc_order))
            else:
                frag = self.pack_stream_bf16(w_out_in, ks, NT, acc_order=acc_order, dtype=dtype).view(ks, NT, 2 * 64 * 8)
                wchunks.append(frag.transpose(0, 1).contiguous().flatten())      # [NT][ks][2][64][8]
            woff[0] += wchunks[-1].numel() * 2
            return o

        desc = SynthDesc()
        desc.n_blocks, desc.C = self.n_blocks, C
        _add_coord_input(tab, desc, self._w_in, self._b_in, HdP)
        _copy_layout(self.desc, desc)
        for k in range(self.n_blocks):
            dst = desc.block[k]
            for s in range(2):
                raw = self._raw[2 * k + s]
                d = dst.spade[s]
                if raw["pixel"]:
                    d.w_gamma = add_w(raw["wgam"], SHARED // 16, False)
                    d.w_beta = add_w(raw["wbet"], SHARED // 16, False)
                    d.vec = add_t(torch.cat([_pad(raw["bgam"] + 1.0, HdP), _pad(raw["bbet"], HdP), _pad(raw["sc"], HdP),
                                             _pad(raw["sh"], HdP)]))
                d.w_conv = add_w(raw["conv_w"], KS, True)
                d.b_conv = add_t(_pad(raw["conv_b"], HdP))
            if dst.to_rgb:
                dst.w_rgb = add_t(_rgb_table(*self._rgb[k], HdP))
        self._x3t[(dtype, fmt)] = dict(desc=desc, wblob=torch.cat(wchunks).contiguous(), tables=tab.cat(), NT=NT, HdP=HdP)
        return self._x3t[(dtype, fmt)]

    def build_x3(self, x2=False):
        """The plan of the register engine: its descriptor, fp32 tables and one weight stream in consumption order (bf16 hi/lo
        stages; x2: f16 hi fragments + fp6 records).  x2 plans carry the ToRGB head tables (_torgb_heads) when X2_HEADS asks
        for them and they fit: plan["heads"] says whether they are there."""
        cache = "_x2" if x2 else "_x3"
        if getattr(self, cache) is None:
            plan = self._build_x3(x2, x2 and self.X2_HEADS)
            # the head tables are 4 KB per skip block (minus the 3 KB zero table): a plan they push past the 160 KB of LDS keeps
            # the riding ToRGB instead (the kernel would refuse the launch, and the plan would otherwise fall to the x3 engine)
            if plan["heads"] and self._x3_lds_bytes(plan, 3) > 160 * 1024:
                plan = self._build_x3(x2, False)
            setattr(self, cache, plan)
        return getattr(self, cache)

    def _build_x3(self, x2, heads):
        pack = self.pack_stream_x2 if x2 else self.pack_stream_bf16
        C = self.C
        NT = 8 if C > 128 else 4
        HdP = NT * 32
        # Conv biases are folded on the host (the x3 kernel never adds one): the kernel's activations are the true ones
        # minus a per-channel "carry" -- the bias of the conv that produced them plus, along a skip chain, the carry of
        # the block input.  Every consumer is affine in its input, so the carry moves into its shift:
        #   SPADE  y = lrelu(sc * (x + c) + sh)  ->  sh' = sh + sc * c      (per-sample ab tables: run(); vec: here)
        #   ToRGB  rgb += Wr (x + c) + br        ->  br' = br + Wr c
        carry = torch.zeros(HdP, device=self.device, dtype=torch.float32)
        ab_carry = torch.zeros(max(1, len(self.const_ids)), HdP, device=self.device, dtype=torch.float32)
        tab = _Table(4)
        desc = SynthDesc()
        desc.n_blocks, desc.C = self.n_blocks, C
        _add_coord_input(tab, desc, self._w_in, self._b_in, HdP)
        _copy_layout(self.desc, desc)
        stream, stages = [], 0
        rgb_tables = {}                                         # block k -> (Wr [3, C], br' [3]) as written to the tables
        for k in range(self.n_blocks):
            src = self.desc.block[k]
            c_in = carry
            # the constant-style blocks between the per-pixel blocks and the first skip block (block 3 of the shipped configs)
            mid_block = (not src.skip and not any(self.desc.block[q].skip for q in range(k))
                         and not self._raw[2 * k]["pixel"] and not self._raw[2 * k + 1]["pixel"])
            for s in range(2):
                raw = self._raw[2 * k + s]
                d = desc.block[k].spade[s]
                if raw["pixel"]:
                    stream.append(pack(raw["wgam"], SHARED // 16, NT))
                    stream.append(pack(raw["wbet"], SHARED // 16, NT))
                    stages += 2 * (SHARED // 16)
                    sc, sh = _pad(raw["sc"], HdP), _pad(raw["sh"], HdP)
                    d.vec = tab.add(torch.cat([_pad(raw["bgam"] + 1.0, HdP), _pad(raw["bbet"], HdP), sc, sh + sc * carry]))
                else:
                    ab_carry[d.ab_index] = carry
                if x2 and self.X2_MID_X3 and mid_block:
                    # round 6: this convolution on three bf16 products inside the x2 kernel (csrc/synthesis_x3.hip: MIDX3): its
                    # stages in the x3 format, the SPADE marked through its (otherwise unused) g_offset
                    stream.append(self.pack_stream_bf16(raw["conv_w"], 2 * NT, NT))
                    d.g_offset = 1
                else:
                    stream.append(pack(raw["conv_w"], 2 * NT, NT))
                stages += 2 * NT
                d.b_conv = -1                                   # folded: the kernel has no bias add
                carry = _pad(raw["conv_b"], HdP)
                if s == 1 and src.skip:
                    carry = carry + c_in
            if src.to_rgb:
                wr, br = self._rgb[k]
                rgb_tables[k] = (wr.float(), br.float() + wr.float() @ carry[: wr.shape[1]])
        # ToRGB tables: one per block -- or, x2 plans with heads, the head tiles of the skip blocks (_torgb_heads), which replace
        # the tables of the skip blocks and of the block in front of them (the LDS has no room for both)
        merged = self._torgb_heads(desc, rgb_tables, tab, NT, HdP) if heads else ()
        for k, (wr, br) in rgb_tables.items():
            if k not in merged:
                desc.block[k].w_rgb = tab.add(_rgb_table(wr, br, HdP))
        return dict(desc=desc, tables=tab.cat(), stream=torch.cat(stream).contiguous(), stages=stages, NT=NT, HdP=HdP,
                    ab_carry=ab_carry, heads=bool(merged))

    # Requests (the outcome is build_x3(True)["heads"]): ToRGB head tables in x2 plans
    X2_HEADS = True
    # x2 plans: the base of the residual stream (the constant-style block in front of the first skip block) on three bf16 products
    # -- the per-contraction attribution's largest contributor (b3.conv1 4.8e-4, b3.conv0 2.3e-4 of an all-x2 7.9e-4)
    X2_MID_X3 = True

    def _torgb_heads(self, desc, rgb_tables, tab, NT, HdP):
        """x2 register engine, round 5: the ToRGB layers of the skip blocks as a NINTH output tile of each block's second
        convolution (csrc/synthesis_x3.hip: conv_progressive HEAD).  With x_k = x_{k-1} + W1_k y_k along the skip chain (biases
        live in the carries, build_x3), sum_k Wr_k x_k over the skip blocks k >= fs that feed ToRGB is

            (sum_k Wr_k) x_{fs-1}  +  sum_{j >= fs} M_j y_j,      M_j = (sum_{k >= j} Wr_k) W1_j   [3, C]

        -- exact algebra on the reference's graph (lib/generators/map3d_generator.py:82-86: rgb accumulates ToRGB of every block's
        output).  The first term joins the ToRGB table of block fs - 1 (weights summed, biases of all the later ToRGBs added);
        M_j travels as a 4 KB table per block, [k-step][f16 hi fragment | half of the fp6 record][4 rows x 2 lane halves][16 B] --
        the 8 lanes (rows 0-3, both halves) of a one-tile x2 stream of M_j padded to 32 rows -- at the float offset stored in the
        block's spade[1].b_conv (unused by this engine otherwise: biases are folded); the skip blocks' to_rgb flags are cleared."""
        n = desc.n_blocks
        fs = next((j for j in range(n) if desc.block[j].skip), None)
        if fs is None or fs == 0 or not any(j in rgb_tables for j in range(fs, n)):
            return ()
        C = self.C
        V = torch.zeros(3, C, dtype=torch.float64, device=self.device)
        bias = torch.zeros(3, dtype=torch.float64, device=self.device)
        heads = {}
        for j in range(n - 1, fs - 1, -1):
            if j in rgb_tables:
                V = V + rgb_tables[j][0].double()
                bias = bias + rgb_tables[j][1].double()
            w1 = self._raw[2 * j + 1]["conv_w"].double()                              # [C_out, C_in] of the block's second convolution
            heads[j] = V @ w1                                                          # [3, C_in]
        # entry term: block fs - 1's table takes (its own ToRGB, if any) + V x_{fs-1} and every later bias
        w0, b0 = rgb_tables.get(fs - 1, (torch.zeros(3, C, device=self.device), torch.zeros(3, device=self.device)))
        wm, bm = (w0.double() + V).float(), (b0.double() + bias).float()
        desc.block[fs - 1].to_rgb = 1
        desc.block[fs - 1].w_rgb = tab.add(_rgb_table(wm, bm, HdP))
        lanes = torch.tensor([0, 1, 2, 3, 32, 33, 34, 35], device=self.device)
        for j in range(fs, n):
            st = self.pack_stream_x2(heads[j].float(), 2 * NT, 1, acc_order=True, dense=False)            # [KS][1][2][64][8] int16
            head = st.view(2 * NT, 2, 64, 8)[:, :, lanes].contiguous()                                    # [KS][hi | rec][8 lanes][16 B]
            desc.block[j].to_rgb = 0
            desc.block[j].spade[1].b_conv = tab.add(head.view(torch.float32))
        return set(range(fs - 1, n))               # blocks whose own ToRGB table is superseded

    def per_forward_tables(self, feature_maps, fixed_style, HdP=None):
        """feature_maps [B,R,F] (rendered, channels last), fixed_style [B,F] -> (G, cst, ab)."""
        HdP = self.HdP if HdP is None else HdP
        B = fixed_style.shape[0]
        dev = fixed_style.device
        pre_fixed = torch.einsum("bf,skf->bsk", fixed_style, self.ws_all)          # [B, 2nb, 128]
        G = cst = ab = None
        if self.pixel_ids:
            G = self._shared_first_layer(feature_maps)                              # [B,R,128*np]
            cst = self.bs_all[self.pix_index].unsqueeze(0).expand(B, -1, -1)
            if self.mode in ("all", "mixed"):                                       # style = feature map + fixed style
                cst = cst + pre_fixed[:, self.pix_index]
            cst = cst.contiguous()
        if self.const_ids:
            a = torch.relu(pre_fixed[:, self.con_index] + self.bs_all[self.con_index])         # [B,nc,128]
            gamma1 = 1.0 + torch.einsum("bsk,skc->bsc", a, self.wg_c) + self.bg_c
            beta = torch.einsum("bsk,skc->bsc", a, self.wb_c) + self.bb_c
            ab = torch.zeros(B, len(self.const_ids), 2, HdP, device=dev, dtype=torch.float32)
            ab[:, :, 0, : self.C] = self.sc_c * gamma1
            ab[:, :, 1, : self.C] = self.sh_c * gamma1 + beta
        return G, cst, ab

    def _shared_first_layer(self, feature_maps):
        """The SPADEs' shared 1x1 convolution at LOW resolution (it commutes with the bilinear resize): [B,R,F] x [F, 128 np].
        58 GFLOP at the bench size -- on the package's own split-bf16 matrix-core GEMM (ops/linear.py: gemm_x3, fp32-class: 16 significant bits per operand, ~2e-5 worst case, ~1e-6 typical)
        when the widths are multiples of 64 and the rows are many (round 5: the last library GEMM of the inference path that was not
        a GEMV); the library's fp32 GEMM otherwise (CPU plans of the host-logic tests, hidden 420)."""
        B, R, F = feature_maps.shape
        # (the choice looks at the rows of ONE item, never at the batch: a batch and its items alone take the same kernel and stay
        # bit-identical -- the x2 arithmetic behind it turns a 1e-6 difference of its input into 1e-4 of quantisation noise; every
        # shipped geometry has R >= 2048)
        if feature_maps.is_cuda and R >= 1024:
            from ..components.ops import linear
            if linear._native_ok(self.ws_pixel.shape[0], F):
                # the rendered maps arrive as a channel slice [.., 3:] of the [B,R,F+3] render output (row stride F + 3, 12 bytes
                # in): _rows makes the aligned [M, F] copy the kernel's 16-byte loads need (151 MB at the bench size, ~0.06 ms)
                return linear.gemm_x3(linear._rows(feature_maps), self.ws_pixel).view(B, R, -1)
        return torch.matmul(feature_maps, self.ws_pixel_t).contiguous()

    def x3_forward_tables(self, feature_maps, fixed_style, x2=False):
        """per_forward_tables for the x3 engine: the conv biases folded into the constant-style shifts (build_x3) and
        `ab` in the kernel's layout [B, n_ab, HdP/2, 4] = sc[n], sc[n+1], sh[n], sh[n+1] (one 16-byte LDS read per two
        channels), both times 0.4: the kernel evaluates lrelu(t) = 0.6 t + 0.4 |t| as fma(u, 1.5, |u|) on u = 0.4 t (two
        instructions per activation instead of three)."""
        x3 = self.build_x3(x2)
        G, cst, ab = self.per_forward_tables(feature_maps, fixed_style, x3["HdP"])
        if ab is not None:
            ab[:, :, 1] += ab[:, :, 0] * x3["ab_carry"][None, : ab.shape[1]]
            ab = ab * 0.4
            Bq, nq, _, Hq = ab.shape
            ab = ab.view(Bq, nq, 2, Hq // 2, 2).permute(0, 1, 3, 2, 4).contiguous()
        return G, cst, ab

    def _resolve(self, H, W, Hr, Wr):
        """-> (family, plan, tier) that run() launches for this geometry: "x3" (the register engines, plan = build_x3), "x3t"
        (the LDS-resident engine, plan = build_x3t of `tier`) or "f32" (the fp32 engine on self.blob, plan None)."""
        if self.engine not in ("bf16x3", "f16x2", "f32") and self.engine not in self.X3T_TIERS:
            raise ValueError(f"unknown synthesis engine {self.engine!r}")
        name = self.engine
        if name in ("bf16x3", "f16x2"):
            x3 = self.build_x3(name == "f16x2")
            if not self.pixel_ids or _lib.load().h3d_synthesis_x3_geometry_ok(H, W, Hr, Wr):
                return "x3", x3, None
            # the x3 engine's matrix-core resize does not cover this geometry: the LDS-resident engine does
            # (f16x2 falls back to the x2 tier of that engine, bf16x3 to its three-product tier)
            name = ("f16x2t" if name == "f16x2" else "bf16x3t") if self.x3t_supported() else "f32"
        if name == "f32":
            return "f32", None, None
        tier = self.X3T_TIERS[name]
        return "x3t", self.build_x3t(tier[0], tier[3]), tier

    def _args(self, plan, G, cst, ab, rgb, B, Hr, Wr, H, W):
        """The arguments every x3 (stream, stages, tables, table floats, ..) and x3t (weight blob, tables, ..) entry point starts
        with, up to the image and its shape."""
        head = ((_lib.ptr(plan["stream"]), plan["stages"], _lib.ptr(plan["tables"]), plan["tables"].numel()) if "stream" in plan
                else (_lib.ptr(plan["wblob"]), _lib.ptr(plan["tables"])))
        return head + (ctypes.byref(plan["desc"]), _lib.ptr(G), self.g_channels, Hr, Wr, _lib.ptr(cst), len(self.pixel_ids),
                       _lib.ptr(ab), len(self.const_ids), _lib.ptr(rgb), B, H, W)

    def run(self, feature_maps, fixed_style, render_hw, out_hw, owner=None):
        """-> rgb [B,3,H,W]."""
        B = fixed_style.shape[0]
        Hr, Wr = render_hw
        H, W = out_hw
        family, plan, tier = self._resolve(H, W, Hr, Wr)
        x2 = family == "x3" and self.engine == "f16x2"
        with stage(owner, "synthesis_tables"):
            if family == "x3":
                G, cst, ab = self.x3_forward_tables(feature_maps.float(), fixed_style.float(), x2)
            else:
                G, cst, ab = self.per_forward_tables(feature_maps.float(), fixed_style.float(), plan["HdP"] if plan else None)
        rgb = torch.empty(B, 3, H, W, device=fixed_style.device, dtype=torch.float32)
        what = {"x3": "h3d_synthesis_x2" if x2 else "h3d_synthesis_x3", "x3t": "h3d_synthesis_x3t", "f32": "h3d_synthesis"}[family]
        lib, st = _lib.load(), _lib.stream_handle()
        args = lambda p, img=rgb: self._args(p, G, cst, ab, img, B, Hr, Wr, H, W)
        with stage(owner, "synthesis"):
            if family == "x3t" and tier[2] == 4 and self.x2_guard:
                # the x2 tier of the LDS-resident engine, range-guarded like the register engine below: the bf16 tier runs
                # behind it on the same flag and only does work when the x2 launch left its f16 range
                alt_tier = self.X3T_TIERS["bf16x3t"]
                alt = self.build_x3t(alt_tier[0], alt_tier[3])
                flag = _lib.ptr(self._flags(B, fixed_style.device))
                rc = lib.h3d_synthesis_x3t_tier_guarded(*args(plan), tier[1], tier[2], flag, st) or \
                    lib.h3d_synthesis_x3t_tier_guarded(*args(alt), alt_tier[1], alt_tier[2], flag, st)
            elif family == "x3t":
                rc = lib.h3d_synthesis_x3t_tier(*args(plan), tier[1], tier[2], st)
            elif x2 and self.x2_guard:
                # Range-guarded x2: the kernel raises an item's device flag when an activation of that item leaves the range
                # its f16 planes carry (|x| >= 2^15, inf, NaN upstream); the bf16 engine, launched right behind it on the same
                # stream, skips the items whose flag is clear and recomputes the others.  No host synchronisation; the x3
                # stream shares descriptor, tables and per-forward tables with the x2 one (only the weight format differs).
                alt = self.build_x3(False)
                flag = _lib.ptr(self._flags(B, fixed_style.device))
                rc = lib.h3d_synthesis_x2_guarded(*args(plan), flag, st)
                if not rc and self.x2_monitor:
                    what = "h3d_synthesis_x3_tiles / h3d_synthesis_check"
                    first, step = self.monitor_tiles(H, W)
                    buf = self._monitor_buf(rgb)
                    rc = lib.h3d_synthesis_x3_tiles(*args(alt, buf[0]), first, step, st)
                    rc = rc or lib.h3d_synthesis_check(_lib.ptr(rgb), _lib.ptr(buf[0]), B, H, W, first, step, self.x2_monitor_tol,
                                                       flag, _lib.ptr(buf[1]), _lib.ptr(buf[2]), st)
                if not rc:
                    what = "h3d_synthesis_x3_if"
                    rc = lib.h3d_synthesis_x3_if(*args(alt), flag, st)
            elif family == "x3":
                rc = (lib.h3d_synthesis_x2 if x2 else lib.h3d_synthesis_x3)(*args(plan), st)
            else:
                rc = self._launch(G, cst, ab, rgb, B, Hr, Wr, H, W)
        _lib.check(rc, what)
        return rgb

    def _monitor_buf(self, rgb):
        """(scratch image, per-item sampled error [B], work [6 B]) of the x2 monitor, kept between runs of one shape."""
        buf = self._x2_monitor_buf
        if buf is None or buf[0].shape != rgb.shape or buf[0].device != rgb.device:
            B = rgb.shape[0]
            buf = (torch.empty_like(rgb), torch.zeros(B, device=rgb.device, dtype=torch.float32),
                   torch.zeros(6 * B, device=rgb.device, dtype=torch.float32))
            self._x2_monitor_buf = buf
        return buf

    def _flags(self, B, device):
        """The per-item flags of a guarded run, zeroed on the current stream."""
        if self._x2_flag is None or self._x2_flag.device != device or self._x2_flag.numel() != B:
            self._x2_flag = torch.zeros(B, dtype=torch.int32, device=device)
        else:
            self._x2_flag.zero_()
        return self._x2_flag

    def monitor_tiles(self, H, W):
        """(first, step) of the 128-pixel tiles the x2 monitor samples: ~x2_monitor_tiles of them, an odd step so that the
        samples walk through the columns of the image as well as down its rows."""
        n_tiles = (H * W + 127) // 128
        step = max(1, n_tiles // max(1, self.x2_monitor_tiles)) | 1
        return min(step // 2, n_tiles - 1), step

    def monitor_tile_count(self, H, W):
        first, step = self.monitor_tiles(H, W)
        return len(range(first, (H * W + 127) // 128, step))

    def x2_monitor_errors(self):
        """Per-item sampled error of the LAST guarded x2 run (device tensor [B]; reading it synchronises), or None."""
        return None if self._x2_monitor_buf is None else self._x2_monitor_buf[1]

    def x2_fell_back(self):
        """True when ANY item of the last run() of the guarded x2 engine left its f16 range (or its sampled error tolerance) and
        came from the bf16 engine (reads the device flags: synchronises; for tests and diagnostics)."""
        return self._x2_flag is not None and bool(int(self._x2_flag.max().item()))   # register engine and LDS-resident x2 tier alike

    def x2_fallback_items(self):
        """Batch indices the bf16 engine redid in the last guarded run (synchronises)."""
        return [] if self._x2_flag is None else torch.nonzero(self._x2_flag).flatten().tolist()

    def _launch(self, G, cst, ab, rgb, B, Hr, Wr, H, W):
        return _lib.load().h3d_synthesis(_lib.ptr(self.blob), ctypes.byref(self.desc), _lib.ptr(G), self.g_channels, Hr, Wr,
                                       _lib.ptr(cst), len(self.pixel_ids), _lib.ptr(ab), len(self.const_ids),
                                       _lib.ptr(rgb), B, H, W, _lib.stream_handle())
