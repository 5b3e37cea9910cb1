// The style input of the generator WITHOUT the 3D render (disable_render=True) as ONE kernel per 64-pixel tile, for
// gfx950: rasterised body condition -> sine features -> one or two leaky-ReLU 1x1 convolutions -> the channels-last
// feature map the synthesis engines read as their low-resolution style map.
//
// Reference semantics: lib/components/map3d_layers.py:278-327 (SynthesisStyleInput), called at
// lib/generators/map3d_generator.py:224-236.  Per pixel, c the condition (1 or 3 channels) and z the latent:
//     f = sin(W_c c + b_c)                                          from_coords: Conv2d(Cc, L, 1) + SinAct
//     h = lrelu_0.2(W_0 [f ; normalize_2nd_moment(z)] + b_0)        network.0: Conv2d(2L, F, 1)
//     h = lrelu_0.2(W_1 h + b_1)                                    network.2: Conv2d(F, F, 1), when the module has it
// What is folded on the host (exact algebra, lib/generators/style_input_pack.py): the latent half of network.0 sees a
// per-image constant, so  bias0[b] = b_0 + W_0[:, L:2L] normalize_2nd_moment(z_b)  is a [B, F] table and the expand / cat
// of the reference is never materialised.
// What runs here per tile, on the fp32 matrix cores (tile engine of field_common.hpp): the sine features are written by
// the VALU straight into the K operand in LDS, the first GEMM contracts them (K = L), its activated result goes back
// into the same LDS buffer as the K operand of the second GEMM (K = F), and only the final [64, F] tile is written to HBM.
// No atomics, one fixed reduction order: two runs are bit-identical.
#include "field_common.hpp"

using namespace h3d;

namespace {

struct Args {
    const float* cond;     // [B, Cc, HW]
    const float* bias0;    // [B, F]  b_0 + latent half of network.0
    const float* wc;       // [Cc + 1][LP]  from_coords weight per input channel, then its bias (zero padded)
    const float* w0;       // packed [L -> F]
    const float* w1;       // packed [F -> F], null with one layer
    const float* b1;       // [FP]
    float* out;            // [B, HW, F]
    int64_t HW;
    int Cc, L, F, LP, FP, n_layers;
};

__device__ __forceinline__ float lrelu(float v) { return fmaxf(v, 0.2f * v); }

template <int NTW>
__global__ __launch_bounds__(kFieldThreads) void style_input_kernel(Args A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int rows = A.LP > A.FP ? A.LP : A.FP;
    float* actT = smem;                         // [max(LP, FP)][MS]  sine features, then the first layer's output
    float* cbuf = actT + rows * kMS;            // [3][64]            condition of the tile
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int b = blockIdx.y;
    const int64_t p0 = (int64_t)blockIdx.x * 64;
    const int NT = A.FP / 32;

    if (t < 64 * A.Cc) {
        const int64_t p = p0 + lane;
        cbuf[t] = p < A.HW ? A.cond[((int64_t)b * A.Cc + (t >> 6)) * A.HW + p] : 0.f;
    }
    __syncthreads();
    // ---- f[k][m] = sin(W_c[k] . c[m] + b_c[k]): wave w writes rows w, w + 4, ... (the weights are wave-uniform)
    {
        const float* __restrict__ wc = A.wc;
        const bool three = A.Cc == 3;
        const float c0 = cbuf[lane], c1 = three ? cbuf[64 + lane] : 0.f, c2 = three ? cbuf[128 + lane] : 0.f;
        for (int k = wave; k < A.LP; k += 4) {
            float v = 0.f;
            if (k < A.L) {
                float a = fmaf(wc[k], c0, wc[A.Cc * A.LP + k]);
                if (three) {
                    a = fmaf(wc[A.LP + k], c1, a);
                    a = fmaf(wc[2 * A.LP + k], c2, a);
                }
                v = sin_accurate(a);
            }
            actT[k * kMS + lane] = v;
        }
    }
    __syncthreads();
    f32x16 acc[2][NTW];
    zero_acc<NTW>(acc);
    gemm_phase<NTW>(acc, actT, reinterpret_cast<const float4*>(A.w0), A.LP / 8, 0, A.LP / 8, NT, wave, lane);
    const float* __restrict__ bias = A.bias0 + (int64_t)b * A.F;      // [F], unpadded: read below n < F only
    if (A.n_layers == 2) {
        __syncthreads();                 // every wave finished reading the sine features
        store_act<NTW>(acc, actT, NT, A.F, wave, lane, [&](int n) { return bias[n]; },
                       [](float v, float c) { return lrelu(v + c); });
        __syncthreads();
        zero_acc<NTW>(acc);
        gemm_phase<NTW>(acc, actT, reinterpret_cast<const float4*>(A.w1), A.FP / 8, 0, A.FP / 8, NT, wave, lane);
        bias = A.b1;
    }
    float* __restrict__ ob = A.out + (int64_t)b * A.HW * A.F;
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        const int nt = wave + 4 * i;
        const int n = nt * 32 + j;
        if (nt >= NT || n >= A.F) continue;
        const float bb = bias[n];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mt * 32 + (r >> 2) * 8 + 4 * h + (r & 3);
                const int64_t p = p0 + m;
                if (p < A.HW) ob[p * A.F + n] = lrelu(acc[mt][i][r] + bb);
            }
    }
}

constexpr int kMaxWidth = 512;       // as h3d_synthesis_mod: 4 column tiles per wave, [512][68] operand tile in the 160 KB LDS

size_t lds_bytes(int LP, int FP) { return sizeof(float) * ((size_t)(LP > FP ? LP : FP) * kMS + 192); }

template <int NTW>
int launch_one(const Args& A, int B, int64_t tiles, hipStream_t st) {
    H3D_ALLOW_MAX_LDS((style_input_kernel<NTW>));
    h3d::pre_launch();
    hipLaunchKernelGGL((style_input_kernel<NTW>), dim3((unsigned)tiles, (unsigned)B), dim3(kFieldThreads),
                       lds_bytes(A.LP, A.FP), st, A);
    return h3d::launch_status("h3d_style_input");
}

}  // namespace

extern "C" int64_t h3d_style_input_lds_bytes(int L, int F) {
    if (L < 1 || F < 1 || L > kMaxWidth || F > kMaxWidth) return -1;
    return (int64_t)lds_bytes(round_up(L, 32), round_up(F, 32));
}

extern "C" int h3d_style_input(const float* cond, const float* bias0, const float* w_coord, const float* w0_packed,
                               const float* w1_packed, const float* b1, float* out, int B, int Cc, int Hc, int Wc, int L,
                               int F, int n_layers, h3d_stream_t stream) {
    H3D_REQUIRE(cond && bias0 && w_coord && w0_packed && out, "h3d_style_input: null pointer");
    H3D_REQUIRE(n_layers == 1 || n_layers == 2, "h3d_style_input: one or two GEMM layers are built (got %d)", n_layers);
    H3D_REQUIRE(n_layers == 1 || (w1_packed && b1), "h3d_style_input: null pointer (second layer)");
    H3D_REQUIRE(Cc == 1 || Cc == 3, "h3d_style_input: the condition has 1 (segments) or 3 (semantics) channels (got %d)", Cc);
    H3D_REQUIRE(B >= 1 && B <= 65535 && Hc >= 1 && Wc >= 1 && L >= 1 && F >= 1, "h3d_style_input: bad shape B=%d %dx%d L=%d F=%d",
                B, Hc, Wc, L, F);
    if (L > kMaxWidth || F > kMaxWidth) {
        h3d::set_error("h3d_style_input: width %d exceeds the %d the LDS plan holds", L > F ? L : F, kMaxWidth);
        return H3D_EUNSUPPORTED;
    }
    H3D_REQUIRE(h3d::aligned16(w0_packed) && h3d::aligned16(w1_packed), "h3d_style_input: packed weights must be 16-byte aligned");
    Args A{};
    A.cond = cond; A.bias0 = bias0; A.wc = w_coord; A.w0 = w0_packed; A.w1 = w1_packed; A.b1 = b1; A.out = out;
    A.HW = (int64_t)Hc * Wc;
    A.Cc = Cc; A.L = L; A.F = F; A.n_layers = n_layers;
    A.LP = round_up(L, 32); A.FP = round_up(F, 32);
    const int64_t tiles = (A.HW + 63) / 64;
    H3D_REQUIRE(tiles < (int64_t(1) << 31), "h3d_style_input: map too large");
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch ((A.FP / 32 + 3) / 4) {
        case 1: return launch_one<1>(A, B, tiles, st);
        case 2: return launch_one<2>(A, B, tiles, st);
        case 3: return launch_one<3>(A, B, tiles, st);
        default: return launch_one<4>(A, B, tiles, st);
    }
}
