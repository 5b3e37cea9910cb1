"""Host-side preparation of the SPADE synthesis network for the fused HIP kernel (csrc/synthesis.hip).

Everything here is *exact* algebra on the reference's eval-mode forward
(lib/generators/map3d_generator.py:58-97, lib/components/map3d_layers.py:176-238):

  static, once per weight version (SynthesisPlan: one parse of the state dict, one lazily built plan per engine family):
    conv weight  = weight_orig / (u . (W v))                (nn.utils.spectral_norm in eval, stored u/v)
    BatchNorm    = x * sc + sh,  sc = weight * rsqrt(running_var + eps),  sh = bias - running_mean * sc
    all matrices packed into the engine's MFMA fragment format (fragment_pack.py, include/h3d.h)
  per forward (per_forward_tables), a handful of tiny library GEMMs on the device:
    shared-MLP pre-activations of the fixed style for all SPADEs:   fixed @ Ws^T + bs
    constant-style SPADEs -> per-(sample, channel) affine  ab = (sc * (1+gamma), sh * (1+gamma) + beta)
    per-pixel-style SPADEs -> low-resolution maps  G = feature_maps @ Ws^T  (the 1x1 conv commutes with the
    bilinear resize that follows it) and the per-sample constant cst
"""
import ctypes
import os
from typing import NamedTuple, Optional

import torch

from ... import _lib
from ..._stages import stage
from .fragment_pack import _pad, pack_matrix, pack_stream_bf16, pack_stream_x2, pack_tiles_x2c

SHARED = 128
EPS_BN = 1e-5


class _Engine(NamedTuple):
    """One arithmetic engine of the synthesis network: the plan it runs on and its entry points of the C ABI (include/h3d.h)."""
    name: str
    family: str                    # "register" (build_x3), "lds" (LDS-resident activations: build_x3t) or "f32" (build_f32)
    elem: torch.dtype              # element type of the weights' hi halves
    fmt: str                       # weight format: "x3" hi + lo halves, "x2" f16 hi + fp6 records, "f32"
    tier: tuple                    # (dtype code, products code): trailing arguments of the LDS-resident entry points
    entry: str                     # the plain launch
    flagged: Optional[str]         # the launch that takes the per-item flags: an x2 engine raises them, any other runs where one is up
    behind: Optional[str]          # x2 engines: the engine launched behind it on those flags
    elsewhere: Optional[str]       # register engines: the engine that takes a geometry h3d_synthesis_x3_geometry_ok rejects


_T, _TG = "h3d_synthesis_x3t_tier", "h3d_synthesis_x3t_tier_guarded"
# "f16x2" one f16 product + one block-scaled fp6 product (both cross terms) per contraction, register-resident activations
# (C <= 256); "bf16x3" split-bf16 matrix cores, register-resident activations (C <= 256); "bf16x3t" / "f16x2t" the same two
# arithmetics with LDS-resident activations (C <= 448: MAP3DBN 384, MAP3DBN512L 420); "f32" fp32 matrix cores (anything else).
# Opt-in reduced-precision tiers on the LDS-resident kernel (NOT within the 1e-3 budget; BASELINE config 5's "fp16 MFMA path"):
# "f16w2t" weights f16 hi + lo, activations one f16 value (two products); "f16x1t" plain f16 products.
_ENGINES = {e.name: e for e in (
    _Engine("f16x2", "register", torch.float16, "x2", (), "h3d_synthesis_x2", "h3d_synthesis_x2_guarded", "bf16x3", "f16x2t"),
    _Engine("bf16x3", "register", torch.bfloat16, "x3", (), "h3d_synthesis_x3", "h3d_synthesis_x3_if", None, "bf16x3t"),
    _Engine("f16x2t", "lds", torch.float16, "x2", (1, 4), _T, _TG, "bf16x3t", None),
    _Engine("bf16x3t", "lds", torch.bfloat16, "x3", (0, 3), _T, _TG, None, None),
    _Engine("f16w2t", "lds", torch.float16, "x3", (1, 2), _T, _TG, None, None),
    _Engine("f16x1t", "lds", torch.float16, "x3", (1, 1), _T, _TG, None, None),
    _Engine("f32", "f32", torch.float32, "f32", (), "h3d_synthesis", None, None, None),
)}


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


def _rgb_table(wr, br, HdP):
    """A ToRGB layer's table: the three weight rows padded to HdP, then the bias padded to 4."""
    return torch.cat([_pad(wr[0], HdP), _pad(wr[1], HdP), _pad(wr[2], HdP), _pad(br, 4)])


def _vec_table(raw, HdP, carry=None):
    """A per-pixel-style SPADE's table: 1 + gamma bias, beta bias, BatchNorm scale, BatchNorm shift (with the carry of a folded
    conv bias moved into it: build_x3), each padded to HdP."""
    sc, sh = _pad(raw["sc"], HdP), _pad(raw["sh"], HdP)
    return torch.cat([_pad(raw["bgam"] + 1.0, HdP), _pad(raw["bbet"], HdP), sc, sh if carry is None else sh + sc * carry])


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
    """The parsed network (dense tensors + layout descriptor), the small dense matrices used by per_forward_tables, and one
    packed plan per engine family, built on first use: build_x3 / build_x3t / build_f32."""

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
        self.HdP = (C + 31) // 32 * 32
        self._w_in = _grow(g(f"{input_prefix}.network.0.weight").reshape(Cin, 2), C)
        self._b_in = _grow(g(f"{input_prefix}.network.0.bias"), C)
        # the layout descriptor: per block skip / to_rgb, per SPADE its style kind and its indices into the per-forward tables;
        # every builder copies it and adds its own offsets
        self.desc = desc = SynthDesc()
        desc.n_blocks, desc.C = n_blocks, C
        ws_all, bs_all, self.pixel_ids, self.const_ids = [], [], [], []
        self._raw = []          # per SPADE: dict of dense fp32 tensors (what the builders pack)
        self._rgb = {}          # block -> ToRGB (weight [3, C], bias [3])
        for k in range(n_blocks):
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
                pixel = map3d_mode == "all" or k in mod_blocks
                self._raw.append(dict(pixel=pixel, conv_w=w / sigma, conv_b=g(cv + ".bias"), wgam=wgam, bgam=bgam,
                                      wbet=wbet, bbet=bbet, sc=sc, sh=sh))
                d = bd.spade[s]
                if pixel:
                    d.pixel_style, d.g_offset, d.cst_index = 1, SHARED * len(self.pixel_ids), len(self.pixel_ids)
                    self.pixel_ids.append(sid)
                else:
                    d.pixel_style, d.ab_index = 0, len(self.const_ids)
                    self.const_ids.append(sid)
            if bd.to_rgb:
                tr = f"{prefix}.to_rgbs.m3d_{k}.linear"
                self._rgb[k] = (g(tr + ".weight").reshape(3, C), g(tr + ".bias"))
        self.ws_all = torch.stack(ws_all)                                 # [2*nb, 128, F]
        self.bs_all = torch.stack(bs_all)                                 # [2*nb, 128]
        pix = torch.tensor(self.pixel_ids, dtype=torch.long, device=device)
        self.pix_index = pix
        self.con_index = torch.tensor(self.const_ids, dtype=torch.long, device=device)
        # [F, 128 * n_pixel]: low-res shared conv for every per-pixel SPADE in one GEMM
        self.ws_pixel_t = (self.ws_all[pix].reshape(-1, F).t().contiguous() if len(self.pixel_ids) else None)
        self.ws_pixel = (self.ws_all[pix].reshape(-1, F).contiguous() if len(self.pixel_ids) else None)       # [128 np, F] rows = outputs
        if self.const_ids:
            const = lambda key: torch.stack([self._raw[i][key] for i in self.const_ids])
            self.wg_c, self.bg_c = const("wgam").transpose(1, 2).contiguous(), const("bgam")    # [nc,128,C], [nc,C]
            self.wb_c, self.bb_c = const("wbet").transpose(1, 2).contiguous(), const("bbet")
            self.sc_c, self.sh_c = const("sc"), const("sh")
        self.g_channels = SHARED * len(self.pixel_ids)
        self.device = device
        self._x3 = self._x2 = self._x3t = self._f32 = None          # the plans, built on first use
        default = ("f16x2" if self.x2_supported() else "bf16x3" if self.x3_supported()
                   else ("f16x2t" if self.x2_weights_in_range() else "bf16x3t") if self.x3t_supported() else "f32")
        self._x2_flag = None          # int32 [B] on the device: the x2 engine's per-item range / monitor flags of the LAST run (see run())
        self.x2_guard = os.environ.get("H3D_SYNTH_GUARD", "1") != "0"
        # Sampled error monitor of the x2 register engine: every forward re-evaluates `x2_monitor_tiles` of its 128-pixel tiles
        # per image on the fp32-class engine and raises the item's device flag (the range guard's) when a sampled pixel differs by
        # more than `x2_monitor_tol` of the image's channel maximum -- the bf16 engine behind it then redoes THAT ITEM (one flag
        # per item: an image must not depend on its batch mates).
        # The tolerance carries the sampling factor: over 192 bench-size images the full-image maximum of |x2 - x3| was
        # 1.2 - 1.65 times the maximum over a 16-tile sample (profiles/r5_x2_fullimage_error.txt: 9.6e-4 full vs 6.6e-4 sampled,
        # 5.7e-4 vs 3.5e-4, 5.2e-4 vs 3.2e-4), so a sample is held to X2_MONITOR_BUDGET / X2_SAMPLING_FACTOR = 6e-4 / 1.7 = 3.5e-4:
        # an item whose sample passes has a full-image error of <= 6e-4 by that ratio, 40 % inside the 1e-3 budget.
        # H3D_SYNTH_MONITOR=0 switches the monitor off, H3D_SYNTH_MONITOR_TOL / _TILES override the two numbers.
        self.x2_monitor = os.environ.get("H3D_SYNTH_MONITOR", "1") != "0"
        self.x2_monitor_tol = float(os.environ.get("H3D_SYNTH_MONITOR_TOL", self.X2_MONITOR_BUDGET / self.X2_SAMPLING_FACTOR))
        self.x2_monitor_tiles = int(os.environ.get("H3D_SYNTH_MONITOR_TILES", "32"))
        self._x2_monitor_buf = None   # (scratch image [B,3,H,W], per-item sampled error [B]) of the last run
        self.engine = os.environ.get("H3D_SYNTH_PRECISION", default)          # a name of _ENGINES

    X2_MONITOR_BUDGET = 6e-4      # full-image |x2 - x3| an item may carry, relative to its channel maximum (budget 1e-3)
    X2_SAMPLING_FACTOR = 1.7      # largest measured (full-image maximum) / (sampled maximum) of that error, rounded up

    # ------------------------------------------------------------------ which engines take this network
    def x3_supported(self):
        """The register engines' structural rules (asked of the library that enforces them at launch: C <= 256, per-pixel
        styles only in a leading run of whole blocks before the first skip block, no plain block after it) and the LDS budget of
        csrc/synthesis_x3.hip (tables, per-sample tables, descriptor copy, weight ring): the kernel's own count."""
        return _lib.load().h3d_synthesis_x3_structure(ctypes.byref(self.desc), 0) == 0 and self._x3_fits(False)

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

    def x3t_supported(self):
        """The LDS-resident engine's structural rules, asked of the library: C <= 448, per-pixel styles only in blocks without
        skip connection, no plain block after the first skip block (csrc/synthesis_x3t.hip)."""
        return _lib.load().h3d_synthesis_x3t_structure(ctypes.byref(self.desc)) == 0

    # ------------------------------------------------------------------ the plans
    def _descriptor(self, tab, HdP):
        """A builder's descriptor: the layout of self.desc, and the coordinate input's tables (w_in [C, 2] as two vectors, b_in)
        as the first entries of `tab`."""
        desc = SynthDesc.from_buffer_copy(self.desc)
        desc.w_in = tab.add(torch.cat([_pad(self._w_in[:, 0], HdP), _pad(self._w_in[:, 1], HdP)]))
        desc.b_in = tab.add(_pad(self._b_in, HdP))
        return desc

    def build_f32(self):
        """The plan of the fp32 engine: every matrix as fp32 MFMA B fragments and every table in one blob, the descriptor's
        offsets in floats into it."""
        if self._f32 is None:
            HdP = self.HdP
            NT, tab = HdP // 32, _Table(1)
            desc = self._descriptor(tab, HdP)
            for k in range(self.n_blocks):
                for s in range(2):
                    raw, d = self._raw[2 * k + s], desc.block[k].spade[s]
                    d.w_conv = tab.add(pack_matrix(raw["conv_w"], HdP // 8, NT))
                    d.b_conv = tab.add(_pad(raw["conv_b"], HdP))
                    if raw["pixel"]:
                        d.w_gamma = tab.add(pack_matrix(raw["wgam"], SHARED // 8, NT))
                        d.w_beta = tab.add(pack_matrix(raw["wbet"], SHARED // 8, NT))
                        d.vec = tab.add(_vec_table(raw, HdP))
                if desc.block[k].to_rgb:
                    desc.block[k].w_rgb = tab.add(_rgb_table(*self._rgb[k], HdP))
            self._f32 = dict(desc=desc, blob=tab.cat(), HdP=HdP)
        return self._f32

    def build_x3t(self, dtype=torch.bfloat16, fmt="x3"):
        """The plan of the LDS-resident engine.  Weights as bf16 (f16 for the reduced-precision tiers) hi/lo MFMA A fragments, tile-major [tile][k-step][hi|lo][64 lanes][8] (conv matrices with K in
        accumulator-register order, gamma / beta in natural order: their input is assembled from memory), fp32 tables
        padded to the engine's width 32 * tiles, and a descriptor whose w_* offsets are BYTES into the fragment blob and
        whose vec / b_conv / w_rgb / w_in / b_in offsets are FLOATS into the tables."""
        if self._x3t is None:
            self._x3t = {}
        if (dtype, fmt) in self._x3t:
            return self._x3t[(dtype, fmt)]
        NT = _lib.load().h3d_synthesis_x3t_tiles(self.C)
        HdP, KS = 32 * NT, 2 * NT
        wchunks, woff, tab = [], [0], _Table(4)

        def add_w(w_out_in, ks, acc_order):
            o = woff[0]
            if fmt == "x2":        # x2c: f16 hi fragments + lo records, [NT][K-tile][3 KiB]
                wchunks.append(pack_tiles_x2c(w_out_in, ks, NT, acc_order=acc_order))
            else:
                frag = pack_stream_bf16(w_out_in, ks, NT, acc_order=acc_order, dtype=dtype).view(ks, NT, 2 * 64 * 8)
                wchunks.append(frag.transpose(0, 1).contiguous().flatten())      # [NT][ks][2][64][8]
            woff[0] += wchunks[-1].numel() * 2
            return o

        desc = self._descriptor(tab, HdP)
        for k in range(self.n_blocks):
            for s in range(2):
                raw, d = self._raw[2 * k + s], desc.block[k].spade[s]
                if raw["pixel"]:
                    d.w_gamma = add_w(raw["wgam"], SHARED // 16, False)
                    d.w_beta = add_w(raw["wbet"], SHARED // 16, False)
                    d.vec = tab.add(_vec_table(raw, HdP))
                d.w_conv = add_w(raw["conv_w"], KS, True)
                d.b_conv = tab.add(_pad(raw["conv_b"], HdP))
            if desc.block[k].to_rgb:
                desc.block[k].w_rgb = tab.add(_rgb_table(*self._rgb[k], HdP))
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
        pack = pack_stream_x2 if x2 else pack_stream_bf16
        NT = 8 if self.C > 128 else 4
        HdP = NT * 32
        # Conv biases are folded on the host (the x3 kernel never adds one): the kernel's activations are the true ones
        # minus a per-channel "carry" -- the bias of the conv that produced them plus, along a skip chain, the carry of
        # the block input.  Every consumer is affine in its input, so the carry moves into its shift:
        #   SPADE  y = lrelu(sc * (x + c) + sh)  ->  sh' = sh + sc * c      (per-sample ab tables: run(); vec: here)
        #   ToRGB  rgb += Wr (x + c) + br        ->  br' = br + Wr c
        carry = torch.zeros(HdP, device=self.device, dtype=torch.float32)
        ab_carry = torch.zeros(max(1, len(self.const_ids)), HdP, device=self.device, dtype=torch.float32)
        tab = _Table(4)
        desc = self._descriptor(tab, HdP)
        stream, stages = [], 0
        rgb_tables = {}                                         # block k -> (Wr [3, C], br' [3]) as written to the tables
        for k in range(self.n_blocks):
            src = self.desc.block[k]
            c_in = carry
            # the constant-style blocks between the per-pixel blocks and the first skip block (block 3 of the shipped configs)
            mid_block = (not src.skip and not any(self.desc.block[q].skip for q in range(k))
                         and not self._raw[2 * k]["pixel"] and not self._raw[2 * k + 1]["pixel"])
            for s in range(2):
                raw, d = self._raw[2 * k + s], desc.block[k].spade[s]
                if raw["pixel"]:
                    stream.append(pack(raw["wgam"], SHARED // 16, NT))
                    stream.append(pack(raw["wbet"], SHARED // 16, NT))
                    stages += 2 * (SHARED // 16)
                    d.vec = tab.add(_vec_table(raw, HdP, carry))
                else:
                    ab_carry[d.ab_index] = carry
                if x2 and self.X2_MID_X3 and mid_block:
                    # this convolution on three bf16 products inside the x2 kernel (csrc/synthesis_x3.hip: MIDX3): its
                    # stages in the x3 format, the SPADE marked through its (otherwise unused) g_offset
                    stream.append(pack_stream_bf16(raw["conv_w"], 2 * NT, NT))
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
        """x2 register engine: the ToRGB layers of the skip blocks as a NINTH output tile of each block's second
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
            st = pack_stream_x2(heads[j].float(), 2 * NT, 1, acc_order=True, dense=False)                 # [KS][1][2][64][8] int16
            head = st.view(2 * NT, 2, 64, 8)[:, :, lanes].contiguous()                                    # [KS][hi | rec][8 lanes][16 B]
            desc.block[j].to_rgb = 0
            desc.block[j].spade[1].b_conv = tab.add(head.view(torch.float32))
        return set(range(fs - 1, n))               # blocks whose own ToRGB table is superseded

    # ------------------------------------------------------------------ per forward
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

    def _plan(self, eng):
        if eng.family == "register":
            return self.build_x3(eng.fmt == "x2")
        return self.build_x3t(eng.elem, eng.fmt) if eng.family == "lds" else self.build_f32()

    def _resolve(self, H, W, Hr, Wr):
        """-> the engine (a row of _ENGINES) that run() launches for this geometry, and its plan."""
        if self.engine not in _ENGINES:
            raise ValueError(f"unknown synthesis engine {self.engine!r}")
        eng = _ENGINES[self.engine]
        if eng.family == "register" and self.pixel_ids and not _lib.load().h3d_synthesis_x3_geometry_ok(H, W, Hr, Wr):
            # the register engines' matrix-core resize does not cover this geometry: the LDS-resident engine does
            eng = _ENGINES[eng.elsewhere if self.x3t_supported() else "f32"]
        return eng, self._plan(eng)

    def _args(self, plan, G, cst, ab, rgb, B, Hr, Wr, H, W):
        """The arguments every x3 (stream, stages, tables, table floats, ..), x3t (weight blob, tables, ..) and fp32 (blob, ..)
        entry point starts with, up to the image and its shape."""
        head = ((_lib.ptr(plan["stream"]), plan["stages"], _lib.ptr(plan["tables"]), plan["tables"].numel()) if "stream" in plan
                else (_lib.ptr(plan["wblob"]), _lib.ptr(plan["tables"])) if "wblob" in plan else (_lib.ptr(plan["blob"]),))
        return head + (ctypes.byref(plan["desc"]), _lib.ptr(G), self.g_channels, Hr, Wr, _lib.ptr(cst), len(self.pixel_ids),
                       _lib.ptr(ab), len(self.const_ids), _lib.ptr(rgb), B, H, W)

    def run(self, feature_maps, fixed_style, render_hw, out_hw, owner=None):
        """-> rgb [B,3,H,W]."""
        B = fixed_style.shape[0]
        Hr, Wr = render_hw
        H, W = out_hw
        eng, plan = self._resolve(H, W, Hr, Wr)
        with stage(owner, "synthesis_tables"):
            if eng.family == "register":
                G, cst, ab = self.x3_forward_tables(feature_maps.float(), fixed_style.float(), eng.fmt == "x2")
            else:
                G, cst, ab = self.per_forward_tables(feature_maps.float(), fixed_style.float(), plan["HdP"])
        rgb = torch.empty(B, 3, H, W, device=fixed_style.device, dtype=torch.float32)
        lib, st = _lib.load(), _lib.stream_handle()

        def call(name, *a):
            _lib.check(getattr(lib, name)(*a, st), name)          # the error names the call that failed

        def launch(name, p, *tail, img=rgb):
            call(name, *self._args(p, G, cst, ab, img, B, Hr, Wr, H, W), *tail)

        with stage(owner, "synthesis"):
            if eng.behind is None or not self.x2_guard:
                launch(eng.entry, plan, *eng.tier)
            else:
                # Range-guarded x2: the kernel raises an item's device flag when an activation of that item leaves the range
                # its f16 planes carry (|x| >= 2^15, inf, NaN upstream); the bf16 engine, launched right behind it on the same
                # stream, skips the items whose flag is clear and recomputes the others.  No host synchronisation; on the register
                # engines the x3 stream shares descriptor, tables and per-forward tables with the x2 one (only the weight format
                # differs).
                behind = _ENGINES[eng.behind]
                alt = self._plan(behind)
                flag = _lib.ptr(self._flags(B, fixed_style.device))
                launch(eng.flagged, plan, *eng.tier, flag)
                if eng.family == "register" and self.x2_monitor:
                    first, step = self.monitor_tiles(H, W)
                    buf = self._monitor_buf(rgb)
                    launch("h3d_synthesis_x3_tiles", alt, first, step, img=buf[0])
                    call("h3d_synthesis_check", _lib.ptr(rgb), _lib.ptr(buf[0]), B, H, W, first, step, self.x2_monitor_tol, flag,
                         _lib.ptr(buf[1]), _lib.ptr(buf[2]))
                launch(behind.flagged, alt, *behind.tier, flag)
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
