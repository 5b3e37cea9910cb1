// Dataset ingest: the item transform of the reference's SHHQDataset.__getitem__ (lib/data/datasets.py:282-309) for a batch of
// decoded uint8 images, one launch.  See include/h3d.h (h3d_ingest) for the definition.
//
// One thread owns kPix consecutive output pixels of one output row: it computes their 3 image channels, the mask and the label and
// stores each as one 16-byte vector when the output width is a multiple of kPix (every row then starts on a 16-byte boundary).
// Reads: the data's own 2:1 ratio (Hs = 2H, Ws = 2W, W % 4 == 0) is the fast path -- the 8 source pixels under the 4 outputs are
// 24 + 8 bytes per source row and 8 label bytes, read as 8-byte words; every other ratio gathers bytes through the integer source
// coordinates.  Both paths run the same per-tap arithmetic in the same order, so they agree bit for bit.  No atomics, no
// cross-thread reduction: a pixel's result depends on its own taps only.
#include "common.hpp"

namespace {

constexpr int kPix = 4;
constexpr int kThreads = 256;

struct Tap {
    int i0, i1;
    float lam;
};

// align_corners = False: source coordinate (o + 1/2) n_src / n_out - 1/2, clamped at 0, over the common denominator 2 n_out.
// The host has checked 2 n_out n_src <= INT32_MAX.
__device__ inline Tap tap(int o, int n_out, int n_src) {
    const int den = 2 * n_out;
    const int num = max((2 * o + 1) * n_src - n_out, 0);
    Tap t;
    t.i0 = num / den;
    t.i1 = min(t.i0 + 1, n_src - 1);
    t.lam = (float)(num - t.i0 * den) / (float)den;
    return t;
}

// u (2/255) - 1 as a product and a difference, each rounded: 255 maps to exactly 1 (a fused multiply-add gives 1 + 2^-23)
__device__ inline float normalise(unsigned u) { return __fsub_rn(__fmul_rn((float)u, 2.f / 255.f), 1.f); }

__device__ inline float bilerp(float v00, float v01, float v10, float v11, float lx, float ly) {
    const float top = fmaf(lx, v01 - v00, v00);
    const float bot = fmaf(lx, v11 - v10, v10);
    return fmaf(ly, bot - top, top);
}

// one output pixel from its four taps: c[k][3] colour bytes and m[k] mask bytes of tap k = (row, column) in {00, 01, 10, 11}
__device__ inline void pixel(const unsigned (&c)[4][3], const unsigned (&m)[4], float lx, float ly, bool geo_only, float (&out)[4]) {
    float vm[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) vm[k] = normalise(m[k]);
    out[3] = bilerp(vm[0], vm[1], vm[2], vm[3], lx, ly);
    if (geo_only) {
        out[0] = out[1] = out[2] = out[3];
        return;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = normalise(m[k] == 0 ? 255u : c[k][ch]);
        out[ch] = bilerp(v[0], v[1], v[2], v[3], lx, ly);
    }
}

__device__ inline unsigned byte_at(const uint32_t* w, int i) { return (w[i >> 2] >> ((i & 3) * 8)) & 255u; }

template <bool kFast>
__global__ __launch_bounds__(kThreads) void ingest_kernel(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ mask,
                                                          const uint8_t* __restrict__ seg, float* __restrict__ images,
                                                          float* __restrict__ masks, int64_t* __restrict__ segs, int B, int Hs, int Ws,
                                                          int H, int W, int groups, int geo_only, int vec_store) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= B * H * groups) return;
    const int g = t % groups, row = t / groups, y = row % H, b = row / H;
    const int x_base = g * kPix;
    const uint8_t* rgb_b = rgb + (size_t)b * Hs * Ws * 3;
    const uint8_t* mask_b = mask + (size_t)b * Hs * Ws;
    const uint8_t* seg_b = seg + (size_t)b * Hs * Ws;
    float out[kPix][4];
    int64_t lab[kPix];

    if constexpr (kFast) {
        // Hs = 2H, Ws = 2W: tap(o) = {2o, 2o + 1, 1/2} on both axes, and the nearest source of output (y, x) is (2y, 2x)
        uint32_t cw[2][6], mw[2][2], sw[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const size_t at = (size_t)(2 * y + r) * Ws + 8 * g;
            const uint2* pc = reinterpret_cast<const uint2*>(rgb_b + at * 3);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const uint2 q = pc[i];
                cw[r][2 * i] = q.x;
                cw[r][2 * i + 1] = q.y;
            }
            const uint2 q = *reinterpret_cast<const uint2*>(mask_b + at);
            mw[r][0] = q.x;
            mw[r][1] = q.y;
        }
        {
            const uint2 q = *reinterpret_cast<const uint2*>(seg_b + (size_t)(2 * y) * Ws + 8 * g);
            sw[0] = q.x;
            sw[1] = q.y;
        }
#pragma unroll
        for (int p = 0; p < kPix; ++p) {
            unsigned c[4][3], m[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int r = k >> 1, col = 2 * p + (k & 1);
                m[k] = byte_at(mw[r], col);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) c[k][ch] = byte_at(cw[r], col * 3 + ch);
            }
            pixel(c, m, 0.5f, 0.5f, geo_only != 0, out[p]);
            const unsigned s = byte_at(sw, 2 * p);
            lab[p] = s == 0 ? 1 : (int64_t)s + 1;
        }
    } else {
        const Tap ty = tap(y, H, Hs);
        const int ys = min((int)((int64_t)y * Hs / H), Hs - 1);
#pragma unroll
        for (int p = 0; p < kPix; ++p) {
            const int x = x_base + p;
            if (x >= W) {
                out[p][0] = out[p][1] = out[p][2] = out[p][3] = 0.f;
                lab[p] = 0;
                continue;
            }
            const Tap tx = tap(x, W, Ws);
            const int rows[2] = {ty.i0, ty.i1}, cols[2] = {tx.i0, tx.i1};
            unsigned c[4][3], m[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const size_t at = (size_t)rows[k >> 1] * Ws + cols[k & 1];
                m[k] = mask_b[at];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) c[k][ch] = rgb_b[at * 3 + ch];
            }
            pixel(c, m, tx.lam, ty.lam, geo_only != 0, out[p]);
            const int xs = min((int)((int64_t)x * Ws / W), Ws - 1);
            const unsigned s = seg_b[(size_t)ys * Ws + xs];
            lab[p] = s == 0 ? 1 : (int64_t)s + 1;
        }
    }

    const size_t plane = (size_t)H * W, at = (size_t)y * W + x_base;
    if (vec_store) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            *reinterpret_cast<float4*>(images + ((size_t)b * 3 + ch) * plane + at) =
                make_float4(out[0][ch], out[1][ch], out[2][ch], out[3][ch]);
        *reinterpret_cast<float4*>(masks + (size_t)b * plane + at) = make_float4(out[0][3], out[1][3], out[2][3], out[3][3]);
        longlong2* ps = reinterpret_cast<longlong2*>(segs + (size_t)b * plane + at);
        ps[0] = make_longlong2(lab[0], lab[1]);
        ps[1] = make_longlong2(lab[2], lab[3]);
    } else {
#pragma unroll
        for (int p = 0; p < kPix; ++p) {
            if (x_base + p >= W) break;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) images[((size_t)b * 3 + ch) * plane + at + p] = out[p][ch];
            masks[(size_t)b * plane + at + p] = out[p][3];
            segs[(size_t)b * plane + at + p] = lab[p];
        }
    }
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

extern "C" int h3d_ingest(const uint8_t* rgb, const uint8_t* mask, const uint8_t* seg, float* images, float* masks,
                          int64_t* body_segments, int B, int Hs, int Ws, int H, int W, int geo_only, h3d_stream_t stream) {
    H3D_REQUIRE(rgb && mask && seg && images && masks && body_segments, "h3d_ingest: null pointer");
    H3D_REQUIRE(B >= 1 && Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1, "h3d_ingest: bad shape B=%d Hs=%d Ws=%d H=%d W=%d", B, Hs, Ws, H, W);
    H3D_REQUIRE((int64_t)B * Hs * Ws * 3 <= INT32_MAX, "h3d_ingest: source element count B*Hs*Ws*3 = %lld overflows int32",
                (long long)B * Hs * Ws * 3);
    H3D_REQUIRE((int64_t)B * H * W * 3 <= INT32_MAX, "h3d_ingest: output element count B*3*H*W = %lld overflows int32",
                (long long)B * H * W * 3);
    H3D_REQUIRE(2 * (int64_t)H * Hs <= INT32_MAX && 2 * (int64_t)W * Ws <= INT32_MAX,
                "h3d_ingest: resize coordinates 2*H*Hs or 2*W*Ws overflow int32 (Hs=%d Ws=%d H=%d W=%d)", Hs, Ws, H, W);
    const int groups = (W + kPix - 1) / kPix;
    const int64_t threads = (int64_t)B * H * groups;
    const unsigned blocks = (unsigned)((threads + kThreads - 1) / kThreads);
    const int vec_store = W % kPix == 0 && h3d::aligned16(images) && h3d::aligned16(masks) && h3d::aligned16(body_segments);
    const bool fast = vec_store && Hs == 2 * H && Ws == 2 * W && aligned8(rgb) && aligned8(mask) && aligned8(seg);
    hipStream_t st = static_cast<hipStream_t>(stream);
    h3d::pre_launch();
    if (fast)
        hipLaunchKernelGGL(ingest_kernel<true>, dim3(blocks), dim3(kThreads), 0, st, rgb, mask, seg, images, masks, body_segments, B, Hs,
                           Ws, H, W, groups, geo_only, vec_store);
    else
        hipLaunchKernelGGL(ingest_kernel<false>, dim3(blocks), dim3(kThreads), 0, st, rgb, mask, seg, images, masks, body_segments, B,
                           Hs, Ws, H, W, groups, geo_only, vec_store);
    return h3d::launch_status("h3d_ingest");
}
