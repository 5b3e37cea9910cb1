// The synthesis network WITHOUT spatial normalisation (spatial_normalization="none") as ONE kernel per 64-pixel tile,
// for gfx950: resize + coordinate input + 9 x [two per-pixel modulated, demodulated 1x1 convolutions] + ToRGB.
//
// Reference semantics: lib/generators/map3d_generator.py:58-97 (SynthesisNetwork.forward, normalization == "none"),
// lib/components/map3d_layers.py:60-80 (SpatialStyleModLayer), :101-112 (SynthesisBlock), :260-275 (SynthesisInput),
// :346-352 (ToRGB on nn.Linear); bilinear F.interpolate at map3d_generator.py:244-245.
//
// One layer:   m = A style + (b_A + 1);   y = lrelu_0.2( ((x * m) W) * rsqrt((m^2) W^2 + eps) + b )
// What is folded on the host (exact algebra, lib/generators/modsynth_pack.py):
//   * a layer whose style is the per-image fixed style (blocks outside mod_blocks in "mixed" / "isolated" mode): m is a
//     per-image vector and so is the demodulation d = rsqrt((m^2) W^2 + eps) -- both are O(B*C) GEMVs per forward, and
//     the layer is ONE GEMM here with a pre-scale (m, on the way into LDS) and a post-scale (d, in the epilogue);
//   * a layer whose style is the rendered feature map: A is linear and the bilinear weights sum to one, so
//     A bilinear(G) + c = bilinear(A G + c): the modulation map M = A G + (A fixed + b_A + 1) is one library GEMM at
//     RENDER resolution; here its HdP channels are bilinearly sampled per output pixel.  Such a layer is TWO GEMMs here
//     ((x*m) W and (m^2) W^2), not three, and no style tile or affine matrix is ever staged.
// What runs here per tile, on the fp32 matrix cores (tile engine of field_common.hpp), activations on chip throughout:
//   x0 = sin(W_in (i, j) + b)                      VALU, straight into the accumulator layout
//   per layer: [sample m ->] x*m -> LDS (K operand) -> GEMM(s) -> epilogue in registers; skip add; ToRGB accumulated
// Register plan: the activation tile lives in the accumulator layout (xr, 32 * NTW VGPRs) and is itself the GEMM
// accumulator of the next layer (it is dead once x*m sits in LDS); a per-pixel layer holds m^2 in a second set until the
// first GEMM has finished reading LDS, then that set accumulates the demodulation; a third set carries the skip input.
// LDS plan: ONE [HdP][68] operand buffer (x*m, then m^2) + 1.5 KB of geometry + 3 KB of ToRGB partials:
// 73 KB at width 256, 143 KB at 512 (one workgroup per CU in practice: the three register sets take more than half the
// register file at widths above 128).  Only the 3-channel image is written to HBM.
#include "field_common.hpp"

using namespace h3d;

namespace {

struct Args {
    const float* blob;
    h3d_modsynth_desc D;
    const float* M;      // [B, Hr*Wr, m_channels] low-resolution modulation maps (channels last)
    const float* md;     // [B, n_vec, 2, HdP] per-image modulation m, demodulation d
    float* rgb;          // [B, 3, H, W]
    int m_channels, Hr, Wr, n_vec, H, W, HdP, C;
};

__device__ __forceinline__ float lrelu(float v) { return fmaxf(v, 0.2f * v); }

template <int NTW>
__global__ __launch_bounds__(kFieldThreads) void synthesis_mod_kernel(Args A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int HdP = A.HdP, C = A.C;
    const int NT = HdP / 32, KBH = HdP / 8;
    float* actT = smem;                         // [HdP][MS]   K operand of the running GEMM
    float* part = actT + HdP * kMS;             // [4][3][64]  ToRGB partial sums
    float* ci = part + 768;                     // [64] pixel coordinate i (rows), then j
    float* cj = ci + 64;
    int* tap = reinterpret_cast<int*>(cj + 64); // [64][4] low-res tap offsets (pixel index); weights follow
    float* tw = reinterpret_cast<float*>(tap + 256);   // [64][2] (ty, tx)

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int b = blockIdx.y;
    const int64_t HW = (int64_t)A.H * A.W;
    const int64_t p0 = (int64_t)blockIdx.x * 64;
    const float* __restrict__ blob = A.blob;
    const h3d_modsynth_desc& D = A.D;

    // ---- per-pixel geometry: synthesis-input coordinates and bilinear taps into the low-res maps
    if (t < 64) {
        int64_t p = p0 + t;
        if (p >= HW) p = HW - 1;
        const int Y = (int)(p / A.W), X = (int)(p % A.W);
        ci[t] = linspace_pm1(A.H, Y);
        cj[t] = linspace_pm1(A.W, X);
        float sy = ((float)Y + 0.5f) * ((float)A.Hr / (float)A.H) - 0.5f;
        float sx = ((float)X + 0.5f) * ((float)A.Wr / (float)A.W) - 0.5f;
        sy = fmaxf(sy, 0.f);
        sx = fmaxf(sx, 0.f);
        const int y0 = min((int)sy, A.Hr - 1), x0 = min((int)sx, A.Wr - 1);
        const int y1 = min(y0 + 1, A.Hr - 1), x1 = min(x0 + 1, A.Wr - 1);
        tap[t * 4 + 0] = y0 * A.Wr + x0;
        tap[t * 4 + 1] = y0 * A.Wr + x1;
        tap[t * 4 + 2] = y1 * A.Wr + x0;
        tap[t * 4 + 3] = y1 * A.Wr + x1;
        tw[t * 2 + 0] = sy - (float)y0;
        tw[t * 2 + 1] = sx - (float)x0;
    }
    __syncthreads();

    // ---- x0[n][m] = sin(w[n][0]*i + w[n][1]*j + b[n]) straight into the accumulator layout
    f32x16 xr[2][NTW], xres[2][NTW];
    {
        const float* __restrict__ win = blob + D.w_in;
        const float* __restrict__ bin = blob + D.b_in;
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            const int nt = wave + 4 * i;
            const int n = min(nt, NT - 1) * 32 + j;
            const bool ok = nt < NT && n < C;
            const float w0 = ok ? win[n] : 0.f, w1 = ok ? win[HdP + n] : 0.f, bb = ok ? bin[n] : 0.f;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) {
                    const float4 vi = *reinterpret_cast<const float4*>(ci + mt * 32 + rg * 8 + 4 * h);
                    const float4 vj = *reinterpret_cast<const float4*>(cj + mt * 32 + rg * 8 + 4 * h);
                    xr[mt][i][rg * 4 + 0] = ok ? sin_accurate(w0 * vi.x + w1 * vj.x + bb) : 0.f;
                    xr[mt][i][rg * 4 + 1] = ok ? sin_accurate(w0 * vi.y + w1 * vj.y + bb) : 0.f;
                    xr[mt][i][rg * 4 + 2] = ok ? sin_accurate(w0 * vi.z + w1 * vj.z + bb) : 0.f;
                    xr[mt][i][rg * 4 + 3] = ok ? sin_accurate(w0 * vi.w + w1 * vj.w + bb) : 0.f;
                }
        }
    }
    zero_acc<NTW>(xres);
    float rgb_acc = 0.f;                 // threads < 192: (channel t>>6, pixel t&63)
    bool have_rgb = false;

    for (int blk = 0; blk < D.n_blocks; ++blk) {
        const h3d_modblock_desc& Bk = D.block[blk];
        if (Bk.skip) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int i = 0; i < NTW; ++i) xres[mt][i] = xr[mt][i];
        }
        for (int s = 0; s < 2; ++s) {
            const h3d_modlayer_desc& L = Bk.layer[s];
            const float* __restrict__ bc = blob + L.bias;
            const bool add_skip = s == 1 && Bk.skip;
            __syncthreads();             // every wave finished reading actT (previous GEMM or ToRGB)
            if (L.pixel_style) {
                // ---- modulation: bilinear sample of this layer's slice of M -> actT[n][m] (wave w: a quarter of the channels)
                {
                    const int m = lane, kq = HdP / 4, k0 = wave * kq;
                    const float* __restrict__ Mb = A.M + (int64_t)b * A.Hr * A.Wr * A.m_channels + L.map_offset + k0;
                    const float ty = tw[m * 2], tx = tw[m * 2 + 1];
                    const float tx1 = 1.f - tx, ty1 = 1.f - ty;
                    const float4* g00 = reinterpret_cast<const float4*>(Mb + (int64_t)tap[m * 4 + 0] * A.m_channels);
                    const float4* g01 = reinterpret_cast<const float4*>(Mb + (int64_t)tap[m * 4 + 1] * A.m_channels);
                    const float4* g10 = reinterpret_cast<const float4*>(Mb + (int64_t)tap[m * 4 + 2] * A.m_channels);
                    const float4* g11 = reinterpret_cast<const float4*>(Mb + (int64_t)tap[m * 4 + 3] * A.m_channels);
#pragma unroll 2
                    for (int q = 0; q < kq / 4; ++q) {
                        const float4 a = g00[q], bq = g01[q], c = g10[q], d = g11[q];
                        // same association as F.interpolate: lerp in x on both rows, then lerp in y
                        float* dst = actT + (k0 + q * 4) * kMS + m;
                        dst[0 * kMS] = (a.x * tx1 + bq.x * tx) * ty1 + (c.x * tx1 + d.x * tx) * ty;
                        dst[1 * kMS] = (a.y * tx1 + bq.y * tx) * ty1 + (c.y * tx1 + d.y * tx) * ty;
                        dst[2 * kMS] = (a.z * tx1 + bq.z * tx) * ty1 + (c.z * tx1 + d.z * tx) * ty;
                        dst[3 * kMS] = (a.w * tx1 + bq.w * tx) * ty1 + (c.w * tx1 + d.w * tx) * ty;
                    }
                }
                __syncthreads();
                // ---- x*m replaces m in place (each element has one owner lane in the accumulator layout); m^2 stays in registers
                f32x16 msq[2][NTW];
#pragma unroll
                for (int i = 0; i < NTW; ++i) {
                    const int nt = wave + 4 * i;
                    if (nt >= NT) continue;
                    const int n = nt * 32 + j;
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int rg = 0; rg < 4; ++rg) {
                            float4* p = reinterpret_cast<float4*>(actT + n * kMS + mt * 32 + rg * 8 + 4 * h);
                            const float4 mv = *p;
                            *p = make_float4(xr[mt][i][rg * 4 + 0] * mv.x, xr[mt][i][rg * 4 + 1] * mv.y,
                                             xr[mt][i][rg * 4 + 2] * mv.z, xr[mt][i][rg * 4 + 3] * mv.w);
                            msq[mt][i][rg * 4 + 0] = mv.x * mv.x;
                            msq[mt][i][rg * 4 + 1] = mv.y * mv.y;
                            msq[mt][i][rg * 4 + 2] = mv.z * mv.z;
                            msq[mt][i][rg * 4 + 3] = mv.w * mv.w;
                        }
                }
                __syncthreads();
                zero_acc<NTW>(xr);
                gemm_phase<NTW>(xr, actT, reinterpret_cast<const float4*>(blob + L.w), KBH, 0, KBH, NT, wave, lane);
                __syncthreads();         // every wave finished reading x*m
                store_act<NTW>(msq, actT, NT, C, wave, lane, [](int) { return 0; }, [](float v, int) { return v; });
                __syncthreads();
                zero_acc<NTW>(msq);
                gemm_phase<NTW>(msq, actT, reinterpret_cast<const float4*>(blob + L.w2), KBH, 0, KBH, NT, wave, lane);
#pragma unroll
                for (int i = 0; i < NTW; ++i) {
                    const int n = min(wave + 4 * i, NT - 1) * 32 + j;
                    const float bias = bc[n];
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            float v = lrelu(fmaf(xr[mt][i][r], rsqrtf(msq[mt][i][r] + D.eps), bias));
                            if (add_skip) v += xres[mt][i][r];
                            xr[mt][i][r] = v;
                        }
                }
            } else {
                // ---- per-image modulation: the pre-scale rides on the store, the demodulation on the epilogue
                const float* __restrict__ mv = A.md + ((int64_t)b * A.n_vec + L.vec_index) * 2 * HdP;
                const float* __restrict__ dv = mv + HdP;
                store_act<NTW>(xr, actT, NT, C, wave, lane, [&](int n) { return mv[n]; },
                               [](float v, float c) { return v * c; });
                __syncthreads();
                zero_acc<NTW>(xr);
                gemm_phase<NTW>(xr, actT, reinterpret_cast<const float4*>(blob + L.w), KBH, 0, KBH, NT, wave, lane);
#pragma unroll
                for (int i = 0; i < NTW; ++i) {
                    const int n = min(wave + 4 * i, NT - 1) * 32 + j;
                    const float bias = bc[n], dm = dv[n];
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            float v = lrelu(fmaf(xr[mt][i][r], dm, bias));
                            if (add_skip) v += xres[mt][i][r];
                            xr[mt][i][r] = v;
                        }
                }
            }
        }
        if (Bk.to_rgb) {
            __syncthreads();             // every wave finished reading actT in the block's last GEMM
            store_act<NTW>(xr, actT, NT, C, wave, lane, [](int) { return 0; }, [](float v, int) { return v; });
            __syncthreads();
            const float* __restrict__ wr = blob + Bk.w_rgb;
            const int kq = HdP / 4, k0 = wave * kq;
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
            for (int k = 0; k < kq; ++k) {
                const float x = actT[(k0 + k) * kMS + lane];
                s0 = fmaf(x, wr[k0 + k], s0);
                s1 = fmaf(x, wr[HdP + k0 + k], s1);
                s2 = fmaf(x, wr[2 * HdP + k0 + k], s2);
            }
            part[wave * 192 + lane] = s0;
            part[wave * 192 + 64 + lane] = s1;
            part[wave * 192 + 128 + lane] = s2;
            __syncthreads();
            if (t < 192) {
                const int c = t >> 6;
                const float v = ((part[t] + part[192 + t]) + (part[384 + t] + part[576 + t])) + wr[3 * HdP + c];
                rgb_acc = have_rgb ? v + rgb_acc : v;
            }
            have_rgb = true;
            // (part is written again only after the barriers of the next block's layers)
        }
    }
    if (t < 192) {
        const int c = t >> 6, m = t & 63;
        const int64_t p = p0 + m;
        if (p < HW) A.rgb[((int64_t)b * 3 + c) * HW + p] = rgb_acc;
    }
}

constexpr int kMaxWidth = 512;       // 4 column tiles per wave (NTW <= 4); its 143 KB plan fits the 160 KB LDS

size_t lds_bytes(int HdP) { return sizeof(float) * ((size_t)HdP * kMS + 768 + 128 + 256 + 128); }

template <int NTW>
int launch_one(const Args& A, int B, int64_t tiles, hipStream_t st) {
    H3D_ALLOW_MAX_LDS((synthesis_mod_kernel<NTW>));
    h3d::pre_launch();
    hipLaunchKernelGGL((synthesis_mod_kernel<NTW>), dim3((unsigned)tiles, (unsigned)B), dim3(kFieldThreads), lds_bytes(A.HdP), st, A);
    return h3d::launch_status("h3d_synthesis_mod");
}

}  // namespace

extern "C" int64_t h3d_synthesis_mod_lds_bytes(int C) {
    if (C < 1 || C > kMaxWidth) return -1;
    return (int64_t)lds_bytes(round_up(C, 32));
}

extern "C" int h3d_synthesis_mod(const void* blob, const h3d_modsynth_desc* desc, const float* M, int m_channels, int Hr,
                                 int Wr, const float* md, int n_vec, float* rgb, int B, int H, int W, h3d_stream_t stream) {
    H3D_REQUIRE(blob && desc && rgb, "h3d_synthesis_mod: null pointer");
    H3D_REQUIRE(h3d::aligned16(blob), "h3d_synthesis_mod: blob must be 16-byte aligned");
    H3D_REQUIRE(desc->n_blocks >= 1 && desc->n_blocks <= H3D_MAX_BLOCKS, "h3d_synthesis_mod: n_blocks=%d", desc->n_blocks);
    H3D_REQUIRE(desc->C >= 1, "h3d_synthesis_mod: C=%d", desc->C);
    H3D_REQUIRE(desc->eps > 0.f, "h3d_synthesis_mod: eps must be positive");
    H3D_REQUIRE(B >= 0 && B <= 65535 && H >= 1 && W >= 1, "h3d_synthesis_mod: bad output shape");
    if (desc->C > kMaxWidth) {
        h3d::set_error("h3d_synthesis_mod: width %d exceeds the %d the LDS plan holds", desc->C, kMaxWidth);
        return H3D_EUNSUPPORTED;
    }
    const int HdP = round_up(desc->C, 32);
    H3D_REQUIRE(lds_bytes(HdP) <= 160 * 1024, "h3d_synthesis_mod: width %d does not fit the 160 KB LDS", desc->C);
    bool any_pixel = false, any_vec = false;
    for (int k = 0; k < desc->n_blocks; ++k)
        for (int s = 0; s < 2; ++s) {
            const h3d_modlayer_desc& l = desc->block[k].layer[s];
            H3D_REQUIRE(l.w >= 0 && (l.w & 3) == 0 && l.bias >= 0, "h3d_synthesis_mod: block %d layer %d: bad blob offset", k, s);
            if (l.pixel_style) {
                any_pixel = true;
                H3D_REQUIRE(l.map_offset >= 0 && l.map_offset + HdP <= m_channels && (l.map_offset & 3) == 0,
                            "h3d_synthesis_mod: block %d layer %d map_offset out of range", k, s);
                H3D_REQUIRE(l.w2 >= 0 && (l.w2 & 3) == 0, "h3d_synthesis_mod: block %d layer %d needs the squared weights", k, s);
            } else {
                any_vec = true;
                H3D_REQUIRE(l.vec_index >= 0 && l.vec_index < n_vec, "h3d_synthesis_mod: vec_index out of range");
            }
        }
    H3D_REQUIRE(!any_pixel || (M && Hr >= 1 && Wr >= 1 && (m_channels & 3) == 0 && h3d::aligned16(M)),
                "h3d_synthesis_mod: per-pixel layers need the modulation map (16-byte aligned, channels %% 4 == 0)");
    H3D_REQUIRE(!any_vec || md, "h3d_synthesis_mod: per-image layers need the m / d table");
    H3D_REQUIRE(desc->block[desc->n_blocks - 1].to_rgb, "h3d_synthesis_mod: the last block must feed ToRGB");
    if (B == 0) return H3D_OK;
    Args A{};
    A.blob = static_cast<const float*>(blob);
    A.D = *desc;
    A.M = M; A.md = md; A.rgb = rgb;
    A.m_channels = m_channels; A.Hr = Hr; A.Wr = Wr; A.n_vec = n_vec; A.H = H; A.W = W;
    A.C = desc->C;
    A.HdP = HdP;
    const int64_t tiles = ((int64_t)H * W + 63) / 64;
    H3D_REQUIRE(tiles < (int64_t(1) << 31), "h3d_synthesis_mod: image too large");
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch ((HdP / 32 + 3) / 4) {
        case 1: return launch_one<1>(A, B, tiles, st);
        case 2: return launch_one<2>(A, B, tiles, st);
        case 3: return launch_one<3>(A, B, tiles, st);
        default: return launch_one<4>(A, B, tiles, st);
    }
}
