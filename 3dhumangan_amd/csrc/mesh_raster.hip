// Mesh rasteriser for gfx950 (faces_per_pixel = 1, hard edges, no gradients): the SMPL mesh at the sampled camera, as the
// reference gets it from pytorch3d's MeshRasterizer in SHHQPreprocessor._forward_rasterize (lib/data/preprocessor.py:138-176),
// with the reference's post-processing (:156-174) in the raster launch's epilogue.
//
// Two launches on the caller's stream:
//   setup   one thread per (item, face): view transform + projection in fp64; the face's corners in anchored pixel units,
//           1/depth and a clamped pixel bounding box into the workspace; degenerate / behind-camera / off-image / out-of-range
//           faces get an empty box.
//   raster  one workgroup per (item, 16 x 16 pixel tile), one pixel per thread: the face boxes are streamed in chunks of 256,
//           the faces that meet the tile are compacted into LDS (per-wave ballot + mbcnt), then every pixel tests them.  The
//           best face is kept by the key (pz, face index) compared lexicographically, so the result does not depend on the
//           order in which faces are met: deterministic without a sort.
#include "common.hpp"

namespace {

constexpr int kTile = 16;             // pixels per tile side
constexpr int kThreads = kTile * kTile;
constexpr int kWaves = kThreads / h3d::kWave;
constexpr uint32_t kEmptyLo = 0xFFFFu;  // box (c0 = 0xFFFF, c1 = 0): meets no tile

// Per face: the corners in pixel units (u = (W - s x - 1) / 2, v = (H - s y - 1) / 2: pixel (r, c) sits at u = c, v = r) in fp64,
// and 1/z of each corner.  The edge functions in pixel units are those in NDC times (s/2)^2 (both axes flip, the sign stays) and
// the perspective-corrected barycentrics are ratios of them, so nothing else changes.  They are evaluated in fp64: a thin face
// seen edge-on has an area far below its edge lengths squared, and in fp32 the cancellation of the 2 x 2 determinant alone costs
// ~1e-4 in its barycentrics.
struct FaceRec {
    double2 p0, p1, p2;
    float4 iz;                      // 1/z0 1/z1 1/z2 0
};

__device__ __forceinline__ double edge_d(double px, double py, double ax, double ay, double bx, double by) {
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}

// Pixel range [lo, hi] whose centres  ctr(i) = n/s - (2i+1)/s  fall in [vmin, vmax], widened by one pixel for rounding and
// clamped to [0, n-1]; false when it misses the image.
__device__ __forceinline__ bool pixel_range(double vmin, double vmax, int n, double s, int& lo, int& hi) {
    const double flo = floor((n - s * vmax - 1.0) * 0.5) - 1.0;
    const double fhi = ceil((n - s * vmin - 1.0) * 0.5) + 1.0;
    if (!(flo <= (double)(n - 1)) || !(fhi >= 0.0)) return false;   // also false on NaN
    lo = (int)fmax(flo, 0.0);
    hi = (int)fmin(fhi, (double)(n - 1));
    return lo <= hi;
}

__global__ __launch_bounds__(256) void raster_setup_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                           const float* __restrict__ R, const float* __restrict__ T, float focal,
                                                           uint2* __restrict__ boxes, FaceRec* __restrict__ recs, int V, int F,
                                                           int H, int W) {
    const int b = blockIdx.y;
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int64_t o = (int64_t)b * F + f;
    uint2 box = make_uint2(kEmptyLo, kEmptyLo);
    FaceRec rec;
    rec.p0 = rec.p1 = rec.p2 = make_double2(0.0, 0.0);
    rec.iz = make_float4(0.f, 0.f, 0.f, 0.f);
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {
        const float* Rb = R + 9 * b;
        const float* Tb = T + 3 * b;
        const float* vb = verts + (int64_t)b * V * 3;
        double x[3], y[3], z[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int vi = k == 0 ? i0 : (k == 1 ? i1 : i2);
            const double v0 = vb[3 * vi], v1 = vb[3 * vi + 1], v2 = vb[3 * vi + 2];
            // row vectors: X = v @ R + T
            const double X = v0 * Rb[0] + v1 * Rb[3] + v2 * Rb[6] + Tb[0];
            const double Y = v0 * Rb[1] + v1 * Rb[4] + v2 * Rb[7] + Tb[1];
            const double Z = v0 * Rb[2] + v1 * Rb[5] + v2 * Rb[8] + Tb[2];
            z[k] = Z;
            x[k] = (double)focal * X / Z;
            y[k] = (double)focal * Y / Z;
        }
        const double area = edge_d(x[0], y[0], x[1], y[1], x[2], y[2]);
        const bool front = z[0] > 0.0 && z[1] > 0.0 && z[2] > 0.0;
        int c0, c1, r0, r1;
        const double s = (double)min(H, W);
        if (front && fabs(area) > 1e-8 &&
            pixel_range(fmin(x[0], fmin(x[1], x[2])), fmax(x[0], fmax(x[1], x[2])), W, s, c0, c1) &&
            pixel_range(fmin(y[0], fmin(y[1], y[2])), fmax(y[0], fmax(y[1], y[2])), H, s, r0, r1)) {
            box = make_uint2((uint32_t)c0 | ((uint32_t)c1 << 16), (uint32_t)r0 | ((uint32_t)r1 << 16));
            rec.p0 = make_double2(((double)W - s * x[0] - 1.0) * 0.5, ((double)H - s * y[0] - 1.0) * 0.5);
            rec.p1 = make_double2(((double)W - s * x[1] - 1.0) * 0.5, ((double)H - s * y[1] - 1.0) * 0.5);
            rec.p2 = make_double2(((double)W - s * x[2] - 1.0) * 0.5, ((double)H - s * y[2] - 1.0) * 0.5);
            rec.iz = make_float4((float)(1.0 / z[0]), (float)(1.0 / z[1]), (float)(1.0 / z[2]), 0.f);
        }
    }
    boxes[o] = box;
    recs[o] = rec;
}


__global__ __launch_bounds__(kThreads) void raster_tiles_kernel(const uint2* __restrict__ boxes, const FaceRec* __restrict__ recs,
                                                                const int32_t* __restrict__ faces,
                                                                const int32_t* __restrict__ face_labels,
                                                                const float* __restrict__ table, int32_t* __restrict__ pix_to_face,
                                                                float* __restrict__ zbuf, float* __restrict__ bary,
                                                                int64_t* __restrict__ segments, float* __restrict__ semantics,
                                                                int F, int H, int W, int tiles_x) {
    __shared__ double2 s_p0[kThreads], s_p1[kThreads], s_p2[kThreads];
    __shared__ float4 s_iz[kThreads];
    __shared__ int s_face[kThreads];
    __shared__ int s_cnt[kWaves];

    const int b = blockIdx.y;
    const int tid = threadIdx.x;
    const int lane = tid & (h3d::kWave - 1), wave = tid / h3d::kWave;
    const int tx0 = (blockIdx.x % tiles_x) * kTile, ty0 = (blockIdx.x / tiles_x) * kTile;
    const int tx1 = min(tx0 + kTile - 1, W - 1), ty1 = min(ty0 + kTile - 1, H - 1);
    const int col = tx0 + (tid % kTile), row = ty0 + (tid / kTile);
    const double pu = (double)col, pv = (double)row;       // pixel centre in pixel units

    const uint2* __restrict__ bb = boxes + (int64_t)b * F;
    const FaceRec* __restrict__ rb = recs + (int64_t)b * F;

    float best_z = __builtin_inff();
    int best_f = -1;
    float bw0 = -1.f, bw1 = -1.f, bw2 = -1.f;

    uint2 next = make_uint2(kEmptyLo, kEmptyLo);
    if (tid < F) next = bb[tid];
    for (int base = 0; base < F; base += kThreads) {
        const uint2 box = next;
        const int f = base + tid;
        if (base + kThreads + tid < F) next = bb[base + kThreads + tid];         // prefetch the next chunk's box
        const int c0 = (int)(box.x & 0xFFFFu), c1 = (int)(box.x >> 16);
        const int r0 = (int)(box.y & 0xFFFFu), r1 = (int)(box.y >> 16);
        const bool hit = f < F && c0 <= tx1 && c1 >= tx0 && r0 <= ty1 && r1 >= ty0;
        const uint64_t m = __ballot(hit);
        if (hit) {
            const int slot = wave * h3d::kWave +
                             (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            const FaceRec r = rb[f];
            s_p0[slot] = r.p0;
            s_p1[slot] = r.p1;
            s_p2[slot] = r.p2;
            s_iz[slot] = r.iz;
            s_face[slot] = f;
        }
        if (lane == 0) s_cnt[wave] = __popcll(m);
        __syncthreads();
        for (int w = 0; w < kWaves; ++w) {
            const int n = s_cnt[w];
            for (int k = w * h3d::kWave; k < w * h3d::kWave + n; ++k) {
                const double2 P0 = s_p0[k], P1 = s_p1[k], P2 = s_p2[k];
                const float4 iz = s_iz[k];
                const float e0 = (float)edge_d(pu, pv, P1.x, P1.y, P2.x, P2.y);   // w_i up to the common factor 1/A
                const float e1 = (float)edge_d(pu, pv, P2.x, P2.y, P0.x, P0.y);
                const float e2 = (float)edge_d(pu, pv, P0.x, P0.y, P1.x, P1.y);
                const float q0 = e0 * iz.x, q1 = e1 * iz.y, q2 = e2 * iz.z;       // w_i / z_i
                const float inv = 1.f / (q0 + q1 + q2);
                const float w0 = q0 * inv, w1 = q1 * inv, w2 = q2 * inv;
                if (w0 > 0.f && w1 > 0.f && w2 > 0.f) {
                    const float pz = (e0 + e1 + e2) * inv;                  // sum w'_i z_i = sum w_i / sum (w_i / z_i)
                    const int fk = s_face[k];
                    if (pz < best_z || (pz == best_z && fk < best_f)) {
                        best_z = pz;
                        best_f = fk;
                        bw0 = w0; bw1 = w1; bw2 = w2;
                    }
                }
            }
        }
        __syncthreads();
    }

    if (col >= W || row >= H) return;
    const int64_t plane = (int64_t)H * W;
    const int64_t p = (int64_t)b * plane + (int64_t)row * W + col;
    const bool hit = best_f >= 0;
    pix_to_face[p] = best_f;
    if (zbuf) zbuf[p] = hit ? best_z : -1.f;
    if (bary) {
        bary[3 * p] = bw0;
        bary[3 * p + 1] = bw1;
        bary[3 * p + 2] = bw2;
    }
    if (segments) segments[p] = hit ? (int64_t)face_labels[best_f] + 2 : 1;
    if (semantics) {
        float v0 = 0.f, v1 = 0.f, v2 = 0.f;
        if (hit) {
            const int k = (bw1 > bw0) ? ((bw2 > bw1) ? 2 : 1) : ((bw2 > bw0) ? 2 : 0);     // first maximum, as torch.argmax
            const int vi = faces[3 * best_f + k];
            v0 = table[3 * vi];
            v1 = table[3 * vi + 1];
            v2 = table[3 * vi + 2];
        }
        float* o = semantics + (int64_t)b * 3 * plane + (int64_t)row * W + col;
        o[0] = v0;
        o[plane] = v1;
        o[2 * plane] = v2;
    }
}

int64_t records_offset(int B, int F) { return (((int64_t)B * F * (int64_t)sizeof(uint2)) + 255) & ~(int64_t)255; }

}  // namespace

extern "C" int64_t h3d_mesh_raster_bytes(int B, int F) {
    if (B <= 0 || F <= 0) return 0;
    return records_offset(B, F) + (int64_t)B * F * (int64_t)sizeof(FaceRec);
}

extern "C" int h3d_mesh_rasterize(const float* vertices, const int32_t* faces, const float* R, const float* T, float focal,
                                  const int32_t* face_labels, const float* sem_table, int32_t* pix_to_face, float* zbuf,
                                  float* bary, int64_t* segments, float* semantics, void* workspace, int B, int V, int F,
                                  int H, int W, h3d_stream_t stream) {
    H3D_REQUIRE(vertices && faces && R && T && pix_to_face && workspace, "h3d_mesh_rasterize: null pointer");
    H3D_REQUIRE(!segments || face_labels, "h3d_mesh_rasterize: null pointer (segments need face_labels)");
    H3D_REQUIRE(!semantics || sem_table, "h3d_mesh_rasterize: null pointer (semantics need sem_table)");
    H3D_REQUIRE(B >= 1 && B <= 65535, "h3d_mesh_rasterize: B=%d out of range [1, 65535]", B);
    H3D_REQUIRE(V >= 1 && F >= 1, "h3d_mesh_rasterize: bad mesh V=%d F=%d", V, F);
    H3D_REQUIRE(H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "h3d_mesh_rasterize: bad image size %dx%d", H, W);
    H3D_REQUIRE(focal == focal && focal != 0.f, "h3d_mesh_rasterize: bad focal length");
    H3D_REQUIRE(h3d::aligned16(workspace), "h3d_mesh_rasterize: workspace must be 16-byte aligned");
    const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
    uint2* boxes = static_cast<uint2*>(workspace);
    FaceRec* recs = reinterpret_cast<FaceRec*>(static_cast<char*>(workspace) + records_offset(B, F));
    hipStream_t st = static_cast<hipStream_t>(stream);
    h3d::pre_launch();
    hipLaunchKernelGGL(raster_setup_kernel, dim3((F + 255) / 256, B), dim3(256), 0, st, vertices, faces, R, T, focal, boxes, recs,
                       V, F, H, W);
    int rc = h3d::launch_status("h3d_mesh_rasterize (setup)");
    if (rc != H3D_OK) return rc;
    hipLaunchKernelGGL(raster_tiles_kernel, dim3(tiles_x * tiles_y, B), dim3(kThreads), 0, st, boxes, recs, faces, face_labels,
                       sem_table, pix_to_face, zbuf, bary, segments, semantics, F, H, W, tiles_x);
    return h3d::launch_status("h3d_mesh_rasterize (raster)");
}
