// The rig of an extracted mesh: skin weights carried over from the SMPL body, the rest pose by inverse skinning (h3d_mesh_bind), and
// the mesh in any pose of the same skeleton (h3d_mesh_pose).  See include/h3d.h for both definitions.
//
// No atomics; every sum is taken in a fixed order, so two runs give the same bits.  Nothing lives in a runtime-indexed register
// array: the candidate list of the search has a compile-time length (K is a template argument, 1..8, every loop over it unrolled),
// and the per-vertex joint vector, whose length J is known at run time only, never exists per thread -- it is spread over the lanes
// of a wave (lane = joint).
//
// Bind, 256 threads = 4 waves, a wave owns 64 mesh vertices through three phases:
//   search  lane = vertex.  The SMPL vertices go through LDS in tiles of 1024 as three planes; every lane reads the same address (a
//           broadcast, four candidates per 16-byte read).  The scan runs in ascending index and inserts on strict <, so the K + 1
//           candidates come out ordered by (d^2, index) with no index comparison.  The distance is sqdist_exact: the same bits as the
//           nearest-vertex search of geo_features.hip.  Neighbour ids and their normalised weights go to LDS.
//   blend   lane = joint, a uniform loop over the wave's vertices: w_j = sum_k a^_k W[i_k, j] (ids and a^ broadcast from LDS, the row
//           of W one coalesced read), then five rounds of wave maximum + ballot (the lowest lane that holds the maximum) give the four
//           kept joints and the subtracted fifth value.  Lane 0 writes the four (joint, weight) to LDS.
//   finish  lane = vertex again: the four influences sorted by joint (a 5-comparator network), T from the bone table in LDS, the
//           determinant, the adjugate, the rest position and normal.
// Pose: one thread per (pose, vertex), the pose's J x 12 bone entries in LDS, four influences per vertex in slot order.
#include "device_helpers.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / h3d::kWave;
constexpr int kTile = 1024;             // SMPL vertices per LDS tile
constexpr int kMaxJ = 64;
constexpr int kMaxK = 8;
constexpr float kFar = 3.0e38f;         // pads a tile to a multiple of 4: its squared distance overflows to +inf, and inf < x is never true
constexpr float kInf = __builtin_huge_valf();

__device__ inline bool positive_finite_d(float v) { return v > 0.f && v <= 3.402823466e38f; }   // false for NaN, +-inf, <= 0

__device__ inline float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// rows 0..2 of a [J,4,4] table -> LDS, 12 floats per joint
__device__ inline void stage_bones(const float* __restrict__ A, int J, float* bone) {
    for (int e = threadIdx.x; e < J * 12; e += kThreads) bone[e] = A[(size_t)(e / 12) * 16 + e % 12];
}

// T = sum_i w_i bone[j_i] in the order given (12 entries: rows 0..2 of a 4 x 4)
__device__ inline void blend_bones(const float* bone, const int (&j)[4], const float (&w)[4], float (&T)[12]) {
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = w[0] * bone[j[0] * 12 + e];
#pragma unroll
    for (int i = 1; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 12; ++e) T[e] += w[i] * bone[j[i] * 12 + e];
}

// cofactors of R = T[:3,:3], C[r][c] at C[r * 3 + c]; the adjugate is its transpose; det by the first row
__device__ inline float cofactors(const float (&T)[12], float (&C)[9]) {
    const float a = T[0], b = T[1], c = T[2], d = T[4], e = T[5], f = T[6], g = T[8], h = T[9], i = T[10];
    C[0] = e * i - f * h, C[1] = f * g - d * i, C[2] = d * h - e * g;
    C[3] = c * h - b * i, C[4] = a * i - c * g, C[5] = b * g - a * h;
    C[6] = b * f - c * e, C[7] = c * d - a * f, C[8] = a * e - b * d;
    return a * C[0] + b * C[1] + c * C[2];
}

__device__ inline void store_unit(float* __restrict__ out, float x, float y, float z) {
    const float len = sqrtf(x * x + y * y + z * z);
    const bool ok = positive_finite_d(len);
    out[0] = ok ? x / len : 0.f;
    out[1] = ok ? y / len : 0.f;
    out[2] = ok ? z / len : 0.f;
}

template <int K>
__global__ __launch_bounds__(kThreads) void mesh_bind_kernel(const float* __restrict__ vertices, const float* __restrict__ normals,
                                                             int64_t M, const float* __restrict__ smpl_vertices,
                                                             const float* __restrict__ lbs_weights, const float* __restrict__ A, int V,
                                                             int J, float eps, float* __restrict__ rest_vertices,
                                                             float* __restrict__ rest_normals, int32_t* __restrict__ joints,
                                                             float* __restrict__ weights, float* __restrict__ det_out) {
    __shared__ __attribute__((aligned(16))) float tile[3][kTile];
    __shared__ float bone[kMaxJ * 12];
    __shared__ int nb_id[kWaves][K][h3d::kWave];
    __shared__ float nb_w[kWaves][K][h3d::kWave];
    __shared__ int sel_j[kWaves][4][h3d::kWave];
    __shared__ float sel_w[kWaves][4][h3d::kWave];

    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t wave_base = (int64_t)blockIdx.x * kThreads + wv * h3d::kWave;
    const int64_t left = M - wave_base;
    const int nv = left >= h3d::kWave ? h3d::kWave : (left > 0 ? (int)left : 0);      // this wave's vertices (wave-uniform)
    const int64_t vi = wave_base + lane < M ? wave_base + lane : M - 1;               // a lane past the end repeats the last vertex
    const float px = vertices[vi * 3 + 0], py = vertices[vi * 3 + 1], pz = vertices[vi * 3 + 2];

    stage_bones(A, J, bone);

    // ---- search: the K + 1 nearest, ordered by (d^2, index)
    float cd[K + 1];
    int ci[K + 1];
#pragma unroll
    for (int k = 0; k <= K; ++k) cd[k] = kInf, ci[k] = 0;
    for (int t0 = 0; t0 < V; t0 += kTile) {
        const int n = min(kTile, V - t0), n4 = (n + 3) & ~3;
        __syncthreads();                                   // the previous tile has been scanned
        for (int i = threadIdx.x; i < n4; i += kThreads) {
            const bool in = i < n;
            const float* __restrict__ p = smpl_vertices + (size_t)(t0 + (in ? i : 0)) * 3;
            tile[0][i] = in ? p[0] : kFar;
            tile[1][i] = in ? p[1] : kFar;
            tile[2][i] = in ? p[2] : kFar;
        }
        __syncthreads();
        if (nv > 0) {
            for (int i = 0; i < n4; i += 4) {
                const float4 xs = *reinterpret_cast<const float4*>(&tile[0][i]);
                const float4 ys = *reinterpret_cast<const float4*>(&tile[1][i]);
                const float4 zs = *reinterpret_cast<const float4*>(&tile[2][i]);
                const float x4[4] = {xs.x, xs.y, xs.z, xs.w}, y4[4] = {ys.x, ys.y, ys.z, ys.w}, z4[4] = {zs.x, zs.y, zs.z, zs.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float d = h3d::sqdist_exact(px, py, pz, x4[e], y4[e], z4[e]);
                    if (d < cd[K]) {
                        cd[K] = d, ci[K] = t0 + i + e;
#pragma unroll
                        for (int k = K; k > 0; --k) {
                            const bool up = cd[k] < cd[k - 1];          // strict: an equal distance stays behind the lower index
                            const float dk = cd[k], dm = cd[k - 1];
                            const int ik = ci[k], im = ci[k - 1];
                            cd[k - 1] = up ? dk : dm, cd[k] = up ? dm : dk;
                            ci[k - 1] = up ? ik : im, ci[k] = up ? im : ik;
                        }
                    }
                }
            }
        }
    }
    {
        const float last = 1.f / (cd[K] + eps);
        float a[K], s = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] = 1.f / (cd[k] + eps) - last, s += a[k];
        const bool usable = positive_finite_d(s);
        if (!usable) s = (float)K;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            nb_w[wv][k][lane] = (usable ? a[k] : 1.f) / s;
            nb_id[wv][k][lane] = ci[k];
        }
    }
    __syncthreads();

    // ---- blend: lane = joint
    const bool is_joint = lane < J;
    for (int v = 0; v < nv; ++v) {
        float w = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int id = nb_id[wv][k][v];
            const float a = nb_w[wv][k][v];
            if (is_joint) w += a * lbs_weights[(size_t)id * J + lane];
        }
        bool open = is_joint;
        float top[5];
        int topj[5];
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const float m = wave_max(open ? w : -kInf);
            const unsigned long long holders = __ballot(open && w == m);
            topj[r] = holders ? __ffsll((long long)holders) - 1 : -1;    // the lowest joint that holds the maximum; -1: nobody left
            top[r] = m;
            if (lane == topj[r]) open = false;
        }
        const float c = (J >= 5 && topj[4] >= 0) ? top[4] : 0.f;
        float u[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) u[i] = topj[i] >= 0 ? fmaxf(top[i] - c, 0.f) : 0.f;
        const float sum = ((u[0] + u[1]) + u[2]) + u[3];
        const bool usable = positive_finite_d(sum);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float wi = usable ? u[i] / sum : 0.f;
                sel_w[wv][i][v] = wi;
                sel_j[wv][i][v] = wi > 0.f ? topj[i] : 0;
            }
        }
    }
    __syncthreads();

    // ---- finish: lane = vertex
    if (lane >= nv) return;
    int j[4];
    float w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        j[i] = sel_j[wv][i][lane], w[i] = sel_w[wv][i][lane];
        joints[vi * 4 + i] = j[i];
        weights[vi * 4 + i] = w[i];
    }
    auto order = [&](int a, int b) {                       // ascending joint
        const bool swap = j[b] < j[a];
        const int ja = j[a], jb = j[b];
        const float wa = w[a], wb = w[b];
        j[a] = swap ? jb : ja, j[b] = swap ? ja : jb;
        w[a] = swap ? wb : wa, w[b] = swap ? wa : wb;
    };
    order(0, 1), order(2, 3), order(0, 2), order(1, 3), order(1, 2);
    float T[12], C[9];
    blend_bones(bone, j, w, T);
    const float det = cofactors(T, C);
    det_out[vi] = det;
    const float qx = px - T[3], qy = py - T[7], qz = pz - T[11];
    rest_vertices[vi * 3 + 0] = (C[0] * qx + C[3] * qy + C[6] * qz) / det;      // adjugate = cofactors transposed
    rest_vertices[vi * 3 + 1] = (C[1] * qx + C[4] * qy + C[7] * qz) / det;
    rest_vertices[vi * 3 + 2] = (C[2] * qx + C[5] * qy + C[8] * qz) / det;
    if (rest_normals) {
        const float nx = normals[vi * 3 + 0], ny = normals[vi * 3 + 1], nz = normals[vi * 3 + 2];
        store_unit(rest_normals + vi * 3, T[0] * nx + T[4] * ny + T[8] * nz, T[1] * nx + T[5] * ny + T[9] * nz,
                   T[2] * nx + T[6] * ny + T[10] * nz);
    }
}

__global__ __launch_bounds__(kThreads) void mesh_pose_kernel(const float* __restrict__ rest_vertices,
                                                             const float* __restrict__ rest_normals,
                                                             const int32_t* __restrict__ joints, const float* __restrict__ weights,
                                                             int64_t M, const float* __restrict__ A, int J,
                                                             float* __restrict__ vertices, float* __restrict__ normals) {
    __shared__ float bone[kMaxJ * 12];
    const int pose = blockIdx.y;
    stage_bones(A + (size_t)pose * J * 16, J, bone);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= M) return;
    int j[4];
    float w[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        j[s] = min(max(joints[i * 4 + s], 0), J - 1);      // a joint id outside the table reads inside it
        w[s] = weights[i * 4 + s];
    }
    float T[12];
    blend_bones(bone, j, w, T);
    const float x = rest_vertices[i * 3 + 0], y = rest_vertices[i * 3 + 1], z = rest_vertices[i * 3 + 2];
    float* __restrict__ out = vertices + ((size_t)pose * M + i) * 3;
    out[0] = T[0] * x + T[1] * y + T[2] * z + T[3];
    out[1] = T[4] * x + T[5] * y + T[6] * z + T[7];
    out[2] = T[8] * x + T[9] * y + T[10] * z + T[11];
    if (normals) {
        float C[9];
        const float det = cofactors(T, C);
        const float sign = det < 0.f ? -1.f : 1.f;
        const float nx = rest_normals[i * 3 + 0], ny = rest_normals[i * 3 + 1], nz = rest_normals[i * 3 + 2];
        store_unit(normals + ((size_t)pose * M + i) * 3, sign * (C[0] * nx + C[1] * ny + C[2] * nz),
                   sign * (C[3] * nx + C[4] * ny + C[5] * nz), sign * (C[6] * nx + C[7] * ny + C[8] * nz));
    }
}

template <int K>
void launch_bind(dim3 grid, hipStream_t st, const float* vertices, const float* normals, int64_t M, const float* smpl_vertices,
                 const float* lbs_weights, const float* A, int V, int J, float eps, float* rest_vertices, float* rest_normals,
                 int32_t* joints, float* weights, float* det) {
    hipLaunchKernelGGL(mesh_bind_kernel<K>, grid, dim3(kThreads), 0, st, vertices, normals, M, smpl_vertices, lbs_weights, A, V, J, eps,
                       rest_vertices, rest_normals, joints, weights, det);
}

}  // namespace

extern "C" int h3d_mesh_bind(const float* vertices, const float* normals, int64_t M, const float* smpl_vertices,
                             const float* lbs_weights, const float* A, int V, int J, int K, float eps, float* rest_vertices,
                             float* rest_normals, int32_t* joints, float* weights, float* det, h3d_stream_t stream) {
    H3D_REQUIRE(K >= 1 && K <= kMaxK, "h3d_mesh_bind: K=%d outside 1..%d", K, kMaxK);
    H3D_REQUIRE(V >= K + 1 && V <= (1 << 24), "h3d_mesh_bind: V=%d SMPL vertices, at least K + 1 = %d (at most 2^24)", V, K + 1);
    H3D_REQUIRE(J >= 1 && J <= kMaxJ, "h3d_mesh_bind: J=%d outside 1..%d", J, kMaxJ);
    H3D_REQUIRE(eps > 0.f && eps <= 3.402823466e38f, "h3d_mesh_bind: eps=%g must be positive", eps);
    H3D_REQUIRE((normals == nullptr) == (rest_normals == nullptr), "h3d_mesh_bind: normals and rest_normals go together");
    H3D_REQUIRE(M >= 0 && M < ((int64_t)1 << 31) * kThreads, "h3d_mesh_bind: M=%lld out of range", (long long)M);
    if (M == 0) return H3D_OK;
    H3D_REQUIRE(vertices && smpl_vertices && lbs_weights && A && rest_vertices && joints && weights && det,
                "h3d_mesh_bind: null pointer");
    h3d::pre_launch();
    const dim3 grid((unsigned)((M + kThreads - 1) / kThreads));
    const hipStream_t st = static_cast<hipStream_t>(stream);
#define H3D_BIND_CASE(k)                                                                                                       \
    case k:                                                                                                                    \
        launch_bind<k>(grid, st, vertices, normals, M, smpl_vertices, lbs_weights, A, V, J, eps, rest_vertices, rest_normals, \
                       joints, weights, det);                                                                                  \
        break;
    switch (K) {
        H3D_BIND_CASE(1) H3D_BIND_CASE(2) H3D_BIND_CASE(3) H3D_BIND_CASE(4) H3D_BIND_CASE(5) H3D_BIND_CASE(6) H3D_BIND_CASE(7)
        H3D_BIND_CASE(8)
    }
#undef H3D_BIND_CASE
    return h3d::launch_status("h3d_mesh_bind");
}

extern "C" int h3d_mesh_pose(const float* rest_vertices, const float* rest_normals, const int32_t* joints, const float* weights,
                             int64_t M, const float* A, int n, int J, float* vertices, float* normals, h3d_stream_t stream) {
    H3D_REQUIRE(J >= 1 && J <= kMaxJ, "h3d_mesh_pose: J=%d outside 1..%d", J, kMaxJ);
    H3D_REQUIRE(n >= 0 && n <= 65535, "h3d_mesh_pose: n=%d poses outside 0..65535", n);
    H3D_REQUIRE((normals == nullptr) == (rest_normals == nullptr), "h3d_mesh_pose: rest_normals and normals go together");
    H3D_REQUIRE(M >= 0 && M < ((int64_t)1 << 31) * kThreads, "h3d_mesh_pose: M=%lld out of range", (long long)M);
    if (M == 0 || n == 0) return H3D_OK;
    H3D_REQUIRE(rest_vertices && joints && weights && A && vertices, "h3d_mesh_pose: null pointer");
    h3d::pre_launch();
    hipLaunchKernelGGL(mesh_pose_kernel, dim3((unsigned)((M + kThreads - 1) / kThreads), (unsigned)n), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), rest_vertices, rest_normals, joints, weights, M, A, J, vertices, normals);
    return h3d::launch_status("h3d_mesh_pose");
}
