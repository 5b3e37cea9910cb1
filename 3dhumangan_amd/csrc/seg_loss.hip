// The segmentation loss of the discriminator's label head, fused: PhaseTrainer._calculate_segmentation_loss of the reference
// (lib/trainers/phase_trainer.py:203-256), all four segmentation_loss_mode values, with its two by-products (accuracy over the
// foreground classes, mean foreground probability).  The torch composition is ~15 operations with an int64 one_hot of [B,H,W,L];
// here the logits are read once forward and once backward.
//
//   h3d_seg_histogram   labels -> per-workgroup class counts (wave ballots, no atomics) -> occ [L] in a fixed order, and the
//                       per-class coefficient vector of "cross_entropy_balanced" built from it on the device
//   h3d_seg_loss_fwd    one thread per pixel, one online-softmax pass over its L logits -> per-workgroup partials
//                       {loss sum, correct count, sum of 1 - p0, 0} and, for the backward, the pixel's (max, 1 / sum exp)
//   h3d_seg_loss_bwd    dlogits, one pass
//
// Layouts.  The discriminator hands over y[:, semantic_dim:], a channel slice of a channels-last tensor: channel stride 1, pixel
// stride >= L, one pixel stride across rows and batch items.  A thread that walks its own pixel's channels would read with a
// stride of the pixel pitch between lanes, so that layout is STAGED: the workgroup copies its 256 x L tile to LDS with
// consecutive lanes on consecutive addresses, rows padded to an odd pitch (lane t reads word t * pitch + c: 32 distinct banks),
// and the backward writes its tile back the same way.  Any other strides take the DIRECT path, one strided load per channel:
// for contiguous NCHW consecutive lanes are consecutive pixels, so that is coalesced too.
#include "common.hpp"

namespace {

constexpr int kRows = 256;        // pixels per workgroup = per partial row
constexpr int kMaxL = 64;
constexpr int kCols = 4;          // partial columns: loss sum, correct, sum(1 - p0), unused (0)

enum Kind { kSoftmaxCE = 0, kMulticlassBCE = 1, kSoftplus = 2 };

struct Strides { int64_t b, c, h, w; };

__device__ inline float softplus_f(float y) { return fmaxf(y, 0.f) + log1pf(expf(-fabsf(y))); }
__device__ inline float sigmoid_f(float y) {
    if (y >= 0.f) return 1.f / (1.f + expf(-y));
    const float e = expf(y);
    return e / (1.f + e);
}
// the multi-label target of "cross_entropy_multiclass" / "softplus" (:225-226, :244-245): the one-hot, with channel 1 also set
// on every foreground pixel
__device__ inline bool target_set(int c, int64_t gt) { return c == gt || (c == 1 && gt > 0); }

// floor(e / L) for e < 2^16, 2 <= L <= 64, by one multiply: magic = floor(2^32 / L) + 1
__device__ inline unsigned div_small(unsigned e, unsigned magic) { return __umulhi(e, magic); }

struct PixelAddr {
    int64_t n, b;
    int h, w;
};
__device__ inline PixelAddr pixel_of(int64_t n, int64_t P, int W) {
    PixelAddr a;
    a.n = n;
    a.b = n / P;
    const int p = (int)(n - a.b * P);
    a.h = p / W;
    a.w = p - a.h * W;
    return a;
}

// tile[pix * LP + c] = x[(n0 + pix) * pitch + c] for the `count` pixels of this workgroup; consecutive lanes, consecutive words
__device__ inline void stage_in(float* tile, const float* __restrict__ x, int64_t n0, int count, int64_t pitch, int L, int LP) {
    const unsigned magic = 0xFFFFFFFFu / (unsigned)L + 1u;
    const float* base = x + n0 * pitch;
    for (unsigned e = threadIdx.x; e < (unsigned)(count * L); e += kRows) {
        const unsigned pix = div_small(e, magic), c = e - pix * L;
        tile[pix * LP + c] = base[(int64_t)pix * pitch + c];
    }
}

struct RowSums {
    float m, s, s_fg, x_gt, extra;
    int arg;
};

// one pass over a pixel's logits: running max with rescaled sums (all of exp(x - m), and of the foreground channels alone), the
// first maximum over c >= 1, the label's logit, and the mode's own per-channel sum
template <class Row>
__device__ inline RowSums row_pass(Row X, int L, int64_t gt, int kind) {
    RowSums r;
    r.m = -INFINITY; r.s = 0.f; r.s_fg = 0.f; r.x_gt = 0.f; r.extra = 0.f; r.arg = 1;
    float best = -INFINITY;
    const float tail = L > 2 ? 1.f / (float)(L - 2) : 0.f;
    for (int c = 0; c < L; ++c) {
        const float x = X(c);
        if (x > r.m) {
            const float k = expf(r.m - x);         // 0 at the first channel (m = -inf)
            r.s *= k; r.s_fg *= k; r.m = x;
        }
        const float e = expf(x - r.m);
        r.s += e;
        if (c >= 1) {
            r.s_fg += e;
            if (x > best || c == 1) { best = x; r.arg = c; }
        }
        if (c == gt) r.x_gt = x;
        if (kind == kMulticlassBCE) {
            r.extra += fmaxf(x, 0.f) - (target_set(c, gt) ? x : 0.f) + log1pf(expf(-fabsf(x)));
        } else if (kind == kSoftplus) {
            const float v = softplus_f(target_set(c, gt) ? -x : x);
            r.extra += c < 2 ? v : v * tail;
        }
    }
    return r;
}

// block sum of three per-thread values in fp64 (4 waves) -> thread 0 holds the totals; `scratch`: 12 doubles of LDS
__device__ inline void block_sum3(double& a, double& b, double& c, double* scratch) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a += __shfl_down(a, off, 64);
        b += __shfl_down(b, off, 64);
        c += __shfl_down(c, off, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { scratch[wave * 3] = a; scratch[wave * 3 + 1] = b; scratch[wave * 3 + 2] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = scratch[0] + scratch[3] + scratch[6] + scratch[9];
        b = scratch[1] + scratch[4] + scratch[7] + scratch[10];
        c = scratch[2] + scratch[5] + scratch[8] + scratch[11];
    }
}

template <bool STAGE>
__global__ __launch_bounds__(kRows) void seg_loss_fwd_kernel(const float* __restrict__ x, Strides xs, const int64_t* __restrict__ labels,
                                                             const float* __restrict__ coef, float* __restrict__ partial,
                                                             float2* __restrict__ stats, int64_t N, int64_t P, int W, int L, int kind) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int64_t n0 = (int64_t)blockIdx.x * kRows;
    const int count = (int)(N - n0 < kRows ? N - n0 : kRows);
    const int t = threadIdx.x;
    const bool live = t < count;
    const int LP = L | 1;
    if (STAGE) {
        stage_in(tile, x, n0, count, xs.w, L, LP);
        __syncthreads();
    }
    double v_loss = 0.0, v_ok = 0.0, v_fg = 0.0;
    if (live) {
        const PixelAddr a = pixel_of(n0 + t, P, W);
        const int64_t gt = labels[a.n];
        RowSums r;
        if (STAGE) {
            const float* row = tile + t * LP;
            r = row_pass([&](int c) { return row[c]; }, L, gt, kind);
        } else {
            const float* row = x + a.b * xs.b + a.h * xs.h + a.w * xs.w;
            const int64_t sc = xs.c;
            r = row_pass([&](int c) { return row[c * sc]; }, L, gt, kind);
        }
        const bool in_range = gt >= 0 && gt < L;
        float loss;
        if (kind == kSoftmaxCE) {
            const float wgt = coef ? (in_range ? coef[gt] : 0.f) : 1.f;
            loss = in_range ? wgt * ((r.m - r.x_gt) + logf(r.s)) : 0.f;
        } else {
            loss = r.extra;
        }
        const float inv = 1.f / r.s;
        if (stats) stats[a.n] = make_float2(r.m, inv);
        v_loss = (double)loss;
        v_ok = r.arg == gt ? 1.0 : 0.0;
        v_fg = (double)(r.s_fg * inv);
    }
    __syncthreads();                                     // the tile is read; its first words become the reduction scratch
    block_sum3(v_loss, v_ok, v_fg, reinterpret_cast<double*>(tile));
    if (t == 0) {
        float* out = partial + (int64_t)blockIdx.x * kCols;
        out[0] = (float)v_loss; out[1] = (float)v_ok; out[2] = (float)v_fg; out[3] = 0.f;
    }
}

// d loss / d x[c] of one pixel.  g: upstream gradient x the mode's 1 / count
__device__ inline float grad_of(float x, int c, int64_t gt, int kind, float g, float wgt, float m, float inv, float tail) {
    if (kind == kSoftmaxCE) return g * wgt * (expf(x - m) * inv - (c == gt ? 1.f : 0.f));
    if (kind == kMulticlassBCE) return g * (sigmoid_f(x) - (target_set(c, gt) ? 1.f : 0.f));
    const float sgn = target_set(c, gt) ? -1.f : 1.f;
    return g * (c < 2 ? 1.f : tail) * sgn * sigmoid_f(sgn * x);
}

// STAGE: x in the sliced channels-last layout (pitch xs.w) AND dx dense channels-last (pitch L); else both by their strides
template <bool STAGE>
__global__ __launch_bounds__(kRows) void seg_loss_bwd_kernel(const float* __restrict__ x, Strides xs, const int64_t* __restrict__ labels,
                                                             const float* __restrict__ coef, const float2* __restrict__ stats,
                                                             const float* __restrict__ gout, float scale, float* __restrict__ dx,
                                                             Strides ds, int64_t N, int64_t P, int W, int L, int kind) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int64_t n0 = (int64_t)blockIdx.x * kRows;
    const int count = (int)(N - n0 < kRows ? N - n0 : kRows);
    const int t = threadIdx.x;
    const int LP = L | 1;
    const float g = gout[0] * scale;
    const float tail = L > 2 ? 1.f / (float)(L - 2) : 0.f;
    if (STAGE) {
        stage_in(tile, x, n0, count, xs.w, L, LP);
        __syncthreads();
    }
    if (t < count) {
        const PixelAddr a = pixel_of(n0 + t, P, W);
        const int64_t gt = labels[a.n];
        const bool in_range = gt >= 0 && gt < L;
        float wgt = 1.f, m = 0.f, inv = 0.f;
        if (kind == kSoftmaxCE) {
            wgt = in_range ? (coef ? coef[gt] : 1.f) : 0.f;
            const float2 st = stats[a.n];
            m = st.x; inv = st.y;
        }
        if (STAGE) {
            float* row = tile + t * LP;
            for (int c = 0; c < L; ++c) row[c] = grad_of(row[c], c, gt, kind, g, wgt, m, inv, tail);
        } else {
            const float* row = x + a.b * xs.b + a.h * xs.h + a.w * xs.w;
            float* drow = dx + a.b * ds.b + a.h * ds.h + a.w * ds.w;
            for (int c = 0; c < L; ++c) drow[c * ds.c] = grad_of(row[c * xs.c], c, gt, kind, g, wgt, m, inv, tail);
        }
    }
    if (STAGE) {
        __syncthreads();
        const unsigned magic = 0xFFFFFFFFu / (unsigned)L + 1u;
        float* base = dx + n0 * L;
        for (unsigned e = t; e < (unsigned)(count * L); e += kRows) {
            const unsigned pix = div_small(e, magic), c = e - pix * L;
            base[e] = tile[pix * LP + c];
        }
    }
}

// class counts of one workgroup's 256 labels: lane c of every wave keeps the popcount of the ballot "label == c"
__global__ __launch_bounds__(kRows) void seg_histogram_kernel(const int64_t* __restrict__ labels, int32_t* __restrict__ partial, int64_t N,
                                                              int L) {
    __shared__ int32_t cnt[kRows / 64][kMaxL];
    const int64_t n = (int64_t)blockIdx.x * kRows + threadIdx.x;
    const int64_t lab = n < N ? labels[n] : -1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t mine = 0;
    for (int c = 0; c < L; ++c) {
        const int k = __popcll(__ballot(lab == c));
        if (lane == c) mine = k;
    }
    cnt[wave][lane] = mine;
    __syncthreads();
    if (threadIdx.x < L) {
        int32_t s = 0;
#pragma unroll
        for (int w = 0; w < kRows / 64; ++w) s += cnt[w][threadIdx.x];
        partial[(int64_t)blockIdx.x * L + threadIdx.x] = s;
    }
}

// occ[c] = sum of the rows in a fixed order (16 row groups, then the groups in order); the coefficient vector of
// "cross_entropy_balanced" (:229-242): class 0 and absent classes 0, present ones numel / (occ * n_present * L) x prior; when no
// label is above 0 the mode is plain cross entropy: every coefficient 1 (a select here, not a host decision)
__global__ __launch_bounds__(1024) void seg_histogram_finish_kernel(const int32_t* __restrict__ partial, int64_t* __restrict__ occ,
                                                                    const float* __restrict__ prior, float* __restrict__ coef,
                                                                    int64_t n_rows, int64_t N, int L) {
    __shared__ int64_t part[16][kMaxL];
    const int c = threadIdx.x & 63, grp = threadIdx.x >> 6;
    int64_t acc = 0;
    if (c < L)
        for (int64_t r = grp; r < n_rows; r += 16) acc += partial[r * L + c];
    part[grp][c] = acc;
    __syncthreads();
    if (grp != 0) return;
    int64_t total = 0;
#pragma unroll
    for (int g = 0; g < 16; ++g) total += part[g][c];
    const bool present = c >= 1 && c < L && total > 0;
    const int n_present = __popcll(__ballot(present));
    if (c >= L) return;
    if (occ) occ[c] = total;
    if (coef) {
        float v = 1.f;
        if (n_present > 0) {
            v = 0.f;
            if (present) {
                // N L / (occ n_present L) x prior in fp64, rounded once (the reference forms it by three fp32 operations)
                v = (float)((double)N / ((double)total * n_present) * (prior ? (double)prior[c] : 1.0));
            }
        }
        coef[c] = v;
    }
}

// one pixel pitch for the whole tensor: pixel n = (b, h, w) sits at n * s.w (the stride of a dimension of size 1 is arbitrary)
inline bool sliced_channels_last(const Strides& s, int B, int H, int W, int L) {
    return s.c == 1 && s.w >= L && (H == 1 || s.h == (int64_t)W * s.w) && (B == 1 || s.b == (int64_t)H * W * s.w);
}

inline size_t tile_bytes(bool stage, int L) {
    const size_t scratch = 12 * sizeof(double);
    const size_t tile = stage ? (size_t)kRows * (L | 1) * sizeof(float) : 0;
    return tile > scratch ? tile : scratch;
}

int check_common(const char* what, const void* x, const int64_t* xs, const void* labels, int B, int H, int W, int L, int kind) {
    H3D_REQUIRE(x && xs && labels, "%s: null pointer", what);
    H3D_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (int64_t)H * W <= INT32_MAX, "%s: bad shape B=%d H=%d W=%d", what, B, H, W);
    H3D_REQUIRE(L >= 2 && L <= kMaxL, "%s: label_dim %d outside [2, %d]", what, L, kMaxL);
    H3D_REQUIRE(kind >= kSoftmaxCE && kind <= kSoftplus, "%s: unknown kind %d", what, kind);
    H3D_REQUIRE(kind != kSoftplus || L >= 3, "%s: the softplus mode needs label_dim >= 3 (got %d)", what, L);
    H3D_REQUIRE(xs[0] >= 0 && xs[1] >= 0 && xs[2] >= 0 && xs[3] >= 0, "%s: negative stride", what);
    H3D_REQUIRE(((int64_t)B * H * W + kRows - 1) / kRows <= INT32_MAX, "%s: too many pixels", what);
    return H3D_OK;
}

}  // namespace

extern "C" int h3d_seg_loss_rows(void) { return kRows; }

extern "C" int h3d_seg_histogram(const int64_t* labels, int32_t* partial, int64_t* occ, const float* prior, float* coef, int64_t N, int L,
                                 h3d_stream_t stream) {
    H3D_REQUIRE(labels && partial && (occ || coef), "h3d_seg_histogram: null pointer");
    H3D_REQUIRE(N >= 1 && (N + kRows - 1) / kRows <= INT32_MAX, "h3d_seg_histogram: bad pixel count %lld", (long long)N);
    H3D_REQUIRE(L >= 2 && L <= kMaxL, "h3d_seg_histogram: label_dim %d outside [2, %d]", L, kMaxL);
    const int64_t rows = (N + kRows - 1) / kRows;
    hipStream_t st = static_cast<hipStream_t>(stream);
    h3d::pre_launch();
    hipLaunchKernelGGL(seg_histogram_kernel, dim3((unsigned)rows), dim3(kRows), 0, st, labels, partial, N, L);
    hipLaunchKernelGGL(seg_histogram_finish_kernel, dim3(1), dim3(1024), 0, st, partial, occ, prior, coef, rows, N, L);
    return h3d::launch_status("h3d_seg_histogram");
}

extern "C" int h3d_seg_loss_fwd(const float* x, const int64_t* x_strides, const int64_t* labels, const float* coef, float* partial,
                                float* stats, int B, int H, int W, int L, int kind, h3d_stream_t stream) {
    if (int rc = check_common("h3d_seg_loss_fwd", x, x_strides, labels, B, H, W, L, kind)) return rc;
    H3D_REQUIRE(partial, "h3d_seg_loss_fwd: null pointer");
    const int64_t P = (int64_t)H * W, N = P * B, rows = (N + kRows - 1) / kRows;
    const Strides xs{x_strides[0], x_strides[1], x_strides[2], x_strides[3]};
    const bool stage = sliced_channels_last(xs, B, H, W, L);
    hipStream_t st = static_cast<hipStream_t>(stream);
    float2* stats2 = reinterpret_cast<float2*>(stats);
    if (stage) {
        H3D_ALLOW_MAX_LDS(seg_loss_fwd_kernel<true>);
        h3d::pre_launch();
        hipLaunchKernelGGL(seg_loss_fwd_kernel<true>, dim3((unsigned)rows), dim3(kRows), tile_bytes(true, L), st, x, xs, labels, coef,
                           partial, stats2, N, P, W, L, kind);
    } else {
        h3d::pre_launch();
        hipLaunchKernelGGL(seg_loss_fwd_kernel<false>, dim3((unsigned)rows), dim3(kRows), tile_bytes(false, L), st, x, xs, labels, coef,
                           partial, stats2, N, P, W, L, kind);
    }
    return h3d::launch_status("h3d_seg_loss_fwd");
}

extern "C" int h3d_seg_loss_bwd(const float* x, const int64_t* x_strides, const int64_t* labels, const float* coef, const float* stats,
                                const float* grad_out, float scale, float* dx, const int64_t* dx_strides, int B, int H, int W, int L,
                                int kind, h3d_stream_t stream) {
    if (int rc = check_common("h3d_seg_loss_bwd", x, x_strides, labels, B, H, W, L, kind)) return rc;
    H3D_REQUIRE(grad_out && dx && dx_strides, "h3d_seg_loss_bwd: null pointer");
    H3D_REQUIRE(kind != kSoftmaxCE || stats, "h3d_seg_loss_bwd: the softmax modes need the forward's stats");
    H3D_REQUIRE(dx_strides[0] >= 0 && dx_strides[1] >= 0 && dx_strides[2] >= 0 && dx_strides[3] >= 0, "h3d_seg_loss_bwd: negative stride");
    const int64_t P = (int64_t)H * W, N = P * B, rows = (N + kRows - 1) / kRows;
    const Strides xs{x_strides[0], x_strides[1], x_strides[2], x_strides[3]};
    const Strides ds{dx_strides[0], dx_strides[1], dx_strides[2], dx_strides[3]};
    const bool stage = sliced_channels_last(xs, B, H, W, L) && sliced_channels_last(ds, B, H, W, L) && ds.w == L;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float2* stats2 = reinterpret_cast<const float2*>(stats);
    if (stage) {
        H3D_ALLOW_MAX_LDS(seg_loss_bwd_kernel<true>);
        h3d::pre_launch();
        hipLaunchKernelGGL(seg_loss_bwd_kernel<true>, dim3((unsigned)rows), dim3(kRows), tile_bytes(true, L), st, x, xs, labels, coef,
                           stats2, grad_out, scale, dx, ds, N, P, W, L, kind);
    } else {
        h3d::pre_launch();
        hipLaunchKernelGGL(seg_loss_bwd_kernel<false>, dim3((unsigned)rows), dim3(kRows), tile_bytes(false, L), st, x, xs, labels, coef,
                           stats2, grad_out, scale, dx, ds, N, P, W, L, kind);
    }
    return h3d::launch_status("h3d_seg_loss_bwd");
}
