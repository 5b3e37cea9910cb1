// The synthesis network's block-0 input when it is more than "sine of the pixel coordinates": the label map as a third
// coordinate (2d_label_input) and / or the latent as extra channels (2d_latent_input), for gfx950.  HBM-bound: one write pass
// forward, one read pass backward.
//
// Reference semantics: lib/generators/map3d_generator.py:256-265 (forward) / :337-352 (staged_forward) --
//   coords = cat([get_2d_coords, rasterized_segments / label_dim * 2 - 1]);  x = sin(Conv2d(K, F, 1)(coords))
//   (lib/components/map3d_layers.py:241-275);  x = cat([x, latent expanded over the pixels]).
//
//   h3d_synth_input       out[b, p, n] = sin(w[n,0] i + w[n,1] j + w[n,2] lab + b[n])  (n < F),  out[b, p, F + l] = z[b, l]
//   h3d_synth_input_bwd   da = dx[..., :F] * cos(a) with the argument recomputed;  dw = sum da (i, j, lab),  db = sum da,
//                         dz[b, l] = sum_p dx[b, p, F + l].  Two stages, no atomics: per-workgroup partial sums, then a second
//                         pass that adds them in a fixed order -- two runs give the same bits.
#include "field_common.hpp"

using namespace h3d;

namespace {

constexpr int kThreads = 256;
constexpr int kRowsFwd = 128;     // pixels of one forward workgroup
constexpr int kRowsBwd = 512;     // pixels of one backward workgroup = one row of the partial-sum buffers
constexpr int kPlanes = 4;        // partial sums per sine channel: da * i, da * j, da * lab, da

// The three coordinates of the workgroup's pixels r0 .. r0 + n - 1 of image b -> LDS (one entry per pixel, read by every
// thread as a broadcast).  lab = seg / label_dim * 2 - 1 in this order, a true division; without a label map lab = 0.
__device__ __forceinline__ void stage_coords(float* ci, float* cj, float* cl, const int64_t* __restrict__ seg, int b, int r0,
                                             int n, int H, int W, int label_dim) {
    const int64_t P = (int64_t)H * W;
    for (int r = threadIdx.x; r < n; r += kThreads) {
        const int p = r0 + r;
        const int y = p / W, x = p - y * W;
        ci[r] = linspace_pm1(H, y);
        cj[r] = linspace_pm1(W, x);
        cl[r] = seg ? (float)seg[(int64_t)b * P + p] / (float)label_dim * 2.f - 1.f : 0.f;
    }
}

struct Column {        // what a thread keeps per sine channel
    float w0, w1, w2, bb;
};

__device__ __forceinline__ Column load_column(const float* __restrict__ w, const float* __restrict__ bias, int n, int K) {
    Column c;
    c.w0 = w[(int64_t)n * K];
    c.w1 = w[(int64_t)n * K + 1];
    c.w2 = K == 3 ? w[(int64_t)n * K + 2] : 0.f;
    c.bb = bias[n];
    return c;
}

__device__ __forceinline__ float argument(const Column& c, float i, float j, float lab) {
    return fmaf(c.w0, i, fmaf(c.w1, j, fmaf(c.w2, lab, c.bb)));
}

// A workgroup owns kRowsFwd consecutive pixels of one image; thread t owns V consecutive channels (quad q = t % QP) of the
// pixels g, g + G, ... (g = t / QP): its weights stay in registers, consecutive lanes store consecutive 16 bytes.  V == 4 needs
// F % 4 == 0 (a quad is all sine or all latent).
template <int V>
__global__ __launch_bounds__(kThreads) void synth_input_fwd(const float* __restrict__ w, const float* __restrict__ bias,
                                                            const int64_t* __restrict__ seg, const float* __restrict__ z,
                                                            float* __restrict__ out, int H, int W, int F, int L, int K,
                                                            int label_dim) {
    __shared__ float ci[kRowsFwd], cj[kRowsFwd], cl[kRowsFwd];
    const int C = F + L, P = H * W;
    const int Q = C / V, QP = Q < kThreads ? Q : kThreads, G = kThreads / QP;
    const int t = threadIdx.x, g = t / QP;
    const int b = blockIdx.y;
    const int r0 = blockIdx.x * kRowsFwd;
    const int n = P - r0 < kRowsFwd ? P - r0 : kRowsFwd;
    stage_coords(ci, cj, cl, seg, b, r0, n, H, W, label_dim);
    __syncthreads();
    if (g >= G) return;
    float* __restrict__ base = out + ((int64_t)b * P + r0) * C;
    for (int q = t - g * QP; q < Q; q += QP) {
        const int c0 = q * V;
        if (c0 < F) {
            Column col[V];
#pragma unroll
            for (int k = 0; k < V; ++k) col[k] = load_column(w, bias, c0 + k, K);
            for (int r = g; r < n; r += G) {
                const float i = ci[r], j = cj[r], lab = cl[r];
                float v[V];
#pragma unroll
                for (int k = 0; k < V; ++k) v[k] = sin_accurate(argument(col[k], i, j, lab));
                float* dst = base + (int64_t)r * C + c0;
                if constexpr (V == 4) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
                else dst[0] = v[0];
            }
        } else {
            float v[V];
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = z[(int64_t)b * L + (c0 - F) + k];
            for (int r = g; r < n; r += G) {
                float* dst = base + (int64_t)r * C + c0;
                if constexpr (V == 4) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
                else dst[0] = v[0];
            }
        }
    }
}

// Stage 1 of the backward: the same ownership over kRowsBwd pixels.  A thread sums its pixels' terms, the row groups of a quad
// are added in LDS in the order g = 0, 1, ...; partial [B, nblk, 4, F] and partial_z [B, nblk, L] take the workgroup's sums.
template <int V>
__global__ __launch_bounds__(kThreads) void synth_input_bwd(const float* __restrict__ w, const float* __restrict__ bias,
                                                            const int64_t* __restrict__ seg, const float* __restrict__ dx,
                                                            float* __restrict__ partial, float* __restrict__ partial_z,
                                                            int H, int W, int F, int L, int K, int label_dim) {
    __shared__ float ci[kRowsBwd], cj[kRowsBwd], cl[kRowsBwd];
    __shared__ float red[kPlanes][kThreads][V];
    const int C = F + L, P = H * W;
    const int Q = C / V, QP = Q < kThreads ? Q : kThreads, G = kThreads / QP;
    const int t = threadIdx.x, g = t / QP;
    const int b = blockIdx.y;
    const int r0 = blockIdx.x * kRowsBwd;
    const int n = P - r0 < kRowsBwd ? P - r0 : kRowsBwd;
    stage_coords(ci, cj, cl, seg, b, r0, n, H, W, label_dim);
    __syncthreads();
    const float* __restrict__ base = dx + ((int64_t)b * P + r0) * C;
    const int64_t slot = (int64_t)b * gridDim.x + blockIdx.x;
    float* __restrict__ out = partial + slot * kPlanes * F;
    float* __restrict__ out_z = partial_z ? partial_z + slot * L : nullptr;
    for (int q0 = 0; q0 < Q; q0 += QP) {
        const int q = q0 + t - g * QP, c0 = q * V;
        const bool on = g < G && q < Q;
        float acc[kPlanes][V];
#pragma unroll
        for (int s = 0; s < kPlanes; ++s)
#pragma unroll
            for (int k = 0; k < V; ++k) acc[s][k] = 0.f;
        if (on && c0 < F) {
            Column col[V];
#pragma unroll
            for (int k = 0; k < V; ++k) col[k] = load_column(w, bias, c0 + k, K);
            for (int r = g; r < n; r += G) {
                const float i = ci[r], j = cj[r], lab = cl[r];
                const float* src = base + (int64_t)r * C + c0;
                float d[V];
                if constexpr (V == 4) {
                    const float4 v = *reinterpret_cast<const float4*>(src);
                    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
                } else {
                    d[0] = src[0];
                }
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const float da = d[k] * cosf(argument(col[k], i, j, lab));
                    acc[0][k] = fmaf(da, i, acc[0][k]);
                    acc[1][k] = fmaf(da, j, acc[1][k]);
                    acc[2][k] = fmaf(da, lab, acc[2][k]);
                    acc[3][k] += da;
                }
            }
        } else if (on) {
            for (int r = g; r < n; r += G) {
                const float* src = base + (int64_t)r * C + c0;
                if constexpr (V == 4) {
                    const float4 v = *reinterpret_cast<const float4*>(src);
                    acc[3][0] += v.x; acc[3][1] += v.y; acc[3][2] += v.z; acc[3][3] += v.w;
                } else {
                    acc[3][0] += src[0];
                }
            }
        }
#pragma unroll
        for (int s = 0; s < kPlanes; ++s)
#pragma unroll
            for (int k = 0; k < V; ++k) red[s][t][k] = acc[s][k];
        __syncthreads();
        if (g == 0 && q < Q) {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                float sum[kPlanes] = {0.f, 0.f, 0.f, 0.f};
                for (int gg = 0; gg < G; ++gg)
#pragma unroll
                    for (int s = 0; s < kPlanes; ++s) sum[s] += red[s][gg * QP + t][k];
                const int c = c0 + k;
                if (c < F) {
#pragma unroll
                    for (int s = 0; s < kPlanes; ++s) out[(int64_t)s * F + c] = sum[s];
                } else if (out_z) {
                    out_z[c - F] = sum[3];
                }
            }
        }
        __syncthreads();
    }
}

// Stage 2: column sums of `rows` partial rows of `cols` floats, in a fixed order.  A workgroup owns 32 columns; its eight row
// groups add the rows g, g + 8, ... one after the other, then group 0 adds the eight sums in the order 0 .. 7.
constexpr int kRedCols = 32, kRedGroups = kThreads / kRedCols;

__device__ __forceinline__ float column_sum(const float* __restrict__ part, int64_t rows, int cols, int c, float (*red)[kRedCols]) {
    const int g = threadIdx.x / kRedCols, lc = threadIdx.x % kRedCols;
    float s = 0.f;
    if (c < cols) {
#pragma unroll 4
        for (int64_t r = g; r < rows; r += kRedGroups) s += part[r * cols + c];
    }
    red[g][lc] = s;
    __syncthreads();
    float total = 0.f;
    if (g == 0)
        for (int gg = 0; gg < kRedGroups; ++gg) total += red[gg][lc];
    return total;
}

// partial [rows, 4, F] -> dw [F, K] (planes 0 .. K-1) and db [F] (plane 3)
__global__ __launch_bounds__(kThreads) void synth_input_reduce_wb(const float* __restrict__ partial, float* __restrict__ dw,
                                                                  float* __restrict__ db, int64_t rows, int F, int K) {
    __shared__ float red[kRedGroups][kRedCols];
    const int cols = kPlanes * F;
    const int c = blockIdx.x * kRedCols + threadIdx.x % kRedCols;
    const float total = column_sum(partial, rows, cols, c, red);
    if (threadIdx.x < kRedCols && c < cols) {
        const int s = c / F, n = c - s * F;
        if (s == 3) db[n] = total;
        else if (s < K) dw[(int64_t)n * K + s] = total;
    }
}

// partial_z [B, rows, L] -> dz [B, L]
__global__ __launch_bounds__(kThreads) void synth_input_reduce_z(const float* __restrict__ partial_z, float* __restrict__ dz,
                                                                 int64_t rows, int L) {
    __shared__ float red[kRedGroups][kRedCols];
    const int b = blockIdx.y;
    const int c = blockIdx.x * kRedCols + threadIdx.x % kRedCols;
    const float total = column_sum(partial_z + (int64_t)b * rows * L, rows, L, c, red);
    if (threadIdx.x < kRedCols && c < L) dz[(int64_t)b * L + c] = total;
}

int check_shape(const char* what, int B, int H, int W, int F, int L, int K, int label_dim) {
    H3D_REQUIRE(B >= 0 && H >= 1 && W >= 1 && F >= 1 && L >= 0, "%s: bad shape B=%d H=%d W=%d F=%d L=%d", what, B, H, W, F, L);
    H3D_REQUIRE(K == 2 || K == 3, "%s: K=%d (2 = coordinates, 3 = coordinates + label)", what, K);
    H3D_REQUIRE(K == 2 || label_dim >= 1, "%s: label_dim=%d", what, label_dim);
    H3D_REQUIRE(B <= 65535, "%s: B=%d > 65535", what, B);
    H3D_REQUIRE((int64_t)H * W < (int64_t(1) << 31) - kRowsBwd, "%s: H*W=%lld out of range", what, (long long)H * W);
    H3D_REQUIRE((int64_t)F + L < (int64_t(1) << 24), "%s: F+L=%lld out of range", what, (long long)F + L);
    return H3D_OK;
}

}  // namespace

extern "C" int h3d_synth_input_rows(void) { return kRowsBwd; }

extern "C" int h3d_synth_input(const float* w, const float* b, const int64_t* seg, const float* z, float* out, int B, int H,
                               int W, int F, int L, int K, int label_dim, h3d_stream_t stream) {
    if (int rc = check_shape("h3d_synth_input", B, H, W, F, L, K, label_dim)) return rc;
    if (B == 0) return H3D_OK;
    H3D_REQUIRE(w && b && out && (L == 0 || z), "h3d_synth_input: null pointer");
    H3D_REQUIRE((K == 3) == (seg != nullptr), "h3d_synth_input: the label map goes with K == 3");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int P = H * W;
    const dim3 grid((unsigned)((P + kRowsFwd - 1) / kRowsFwd), (unsigned)B);
    const bool v4 = F % 4 == 0 && L % 4 == 0 && h3d::aligned16(out);
    h3d::pre_launch();
    if (v4) hipLaunchKernelGGL(synth_input_fwd<4>, grid, dim3(kThreads), 0, st, w, b, seg, z, out, H, W, F, L, K, label_dim);
    else hipLaunchKernelGGL(synth_input_fwd<1>, grid, dim3(kThreads), 0, st, w, b, seg, z, out, H, W, F, L, K, label_dim);
    return h3d::launch_status("h3d_synth_input");
}

extern "C" int h3d_synth_input_bwd(const float* w, const float* b, const int64_t* seg, const float* dx, float* partial,
                                   float* partial_z, float* dw, float* db, float* dz, int B, int H, int W, int F, int L,
                                   int K, int label_dim, h3d_stream_t stream) {
    if (int rc = check_shape("h3d_synth_input_bwd", B, H, W, F, L, K, label_dim)) return rc;
    H3D_REQUIRE(B >= 1, "h3d_synth_input_bwd: B=%d", B);
    H3D_REQUIRE(w && b && dx && partial && dw && db, "h3d_synth_input_bwd: null pointer");
    H3D_REQUIRE((partial_z == nullptr) == (dz == nullptr), "h3d_synth_input_bwd: partial_z and dz go together");
    H3D_REQUIRE(L > 0 || !dz, "h3d_synth_input_bwd: dz without latent channels");
    H3D_REQUIRE((K == 3) == (seg != nullptr), "h3d_synth_input_bwd: the label map goes with K == 3");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int P = H * W;
    const int nblk = (P + kRowsBwd - 1) / kRowsBwd;
    const dim3 grid((unsigned)nblk, (unsigned)B);
    const bool v4 = F % 4 == 0 && L % 4 == 0 && h3d::aligned16(dx);
    h3d::pre_launch();
    if (v4) hipLaunchKernelGGL(synth_input_bwd<4>, grid, dim3(kThreads), 0, st, w, b, seg, dx, partial, partial_z, H, W, F, L, K, label_dim);
    else hipLaunchKernelGGL(synth_input_bwd<1>, grid, dim3(kThreads), 0, st, w, b, seg, dx, partial, partial_z, H, W, F, L, K, label_dim);
    hipLaunchKernelGGL(synth_input_reduce_wb, dim3((unsigned)((kPlanes * F + kRedCols - 1) / kRedCols)), dim3(kThreads), 0, st,
                       (const float*)partial, dw, db, (int64_t)B * nblk, F, K);
    if (dz)
        hipLaunchKernelGGL(synth_input_reduce_z, dim3((unsigned)((L + kRedCols - 1) / kRedCols), (unsigned)B), dim3(kThreads), 0, st,
                           (const float*)partial_z, dz, (int64_t)nblk, L);
    return h3d::launch_status("h3d_synth_input_bwd");
}
