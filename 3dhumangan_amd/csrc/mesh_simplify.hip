// Simplification of an indexed triangle mesh by quadric vertex clustering on a uniform grid (Lindstrom's out-of-core scheme).  See
// include/h3d.h (h3d_mesh_cluster_cells / _faces / _solve) for the definition; the sorts and prefix sums between the three launches
// are the caller's (lib/components/mesh_simplify.py).
//
// No atomics and no LDS.  cells and faces: one thread per vertex / face, 256 threads.  solve: one wavefront per cluster, four to a
// workgroup; the lanes stride over the cluster's two segments (its vertices, its corner records), keep their thirteen partial sums in
// registers and combine them in a butterfly whose order depends on the lane number alone, so the result does not depend on how the
// grid was cut into workgroups and two runs give the same bits.  Every index that addresses memory is clamped into its tensor first:
// lists that do not belong to the mesh give a wrong vertex, never a load or store out of range; every store is guarded.
#include "common.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kWavesPerBlock = kThreads / h3d::kWave;

struct ClusterGrid {
    float ox, oy, oz, cell, inv_cell;
    int nx, ny, nz;
};

__device__ inline bool is_finite(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN and +-inf

// one subtraction, one multiplication, each rounded to fp32 on its own; fmaxf / fminf drop a NaN, an infinity goes to index 0 by name
__device__ inline int axis_cell(float x, float origin, float inv_cell, int n) {
    const float g = __fmul_rn(__fsub_rn(x, origin), inv_cell);
    if (!is_finite(x)) return 0;
    return min((int)fminf(fmaxf(floorf(g), 0.f), 2147483520.f), n - 1);     // the largest float below 2^31: the conversion is exact
}

__global__ __launch_bounds__(kThreads) void mesh_cluster_cells_kernel(const float* __restrict__ vertices, int64_t V, ClusterGrid g,
                                                                      int32_t* __restrict__ cells) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= V) return;
    const int ix = axis_cell(vertices[i * 3 + 0], g.ox, g.inv_cell, g.nx);
    const int iy = axis_cell(vertices[i * 3 + 1], g.oy, g.inv_cell, g.ny);
    const int iz = axis_cell(vertices[i * 3 + 2], g.oz, g.inv_cell, g.nz);
    cells[i] = (ix * g.ny + iy) * g.nz + iz;               // < nx ny nz < 2^31
}

__device__ inline int64_t clamp_index(int64_t i, int64_t top) { return min(max(i, (int64_t)0), top); }

__global__ __launch_bounds__(kThreads) void mesh_cluster_faces_kernel(const int32_t* __restrict__ faces, int64_t T,
                                                                      const int32_t* __restrict__ cluster, int64_t V,
                                                                      int32_t* __restrict__ out_faces, uint8_t* __restrict__ keep,
                                                                      int32_t* __restrict__ keys) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    const int32_t c0 = cluster[clamp_index(faces[t * 3 + 0], V - 1)];
    const int32_t c1 = cluster[clamp_index(faces[t * 3 + 1], V - 1)];
    const int32_t c2 = cluster[clamp_index(faces[t * 3 + 2], V - 1)];
    out_faces[t * 3 + 0] = keys[t * 3 + 0] = c0;
    out_faces[t * 3 + 1] = keys[t * 3 + 1] = c1;
    out_faces[t * 3 + 2] = keys[t * 3 + 2] = c2;
    keep[t] = (c0 != c1 && c1 != c2 && c0 != c2) ? 1 : 0;
}

struct Sums {
    float a00, a01, a02, a11, a12, a22, b0, b1, b2, m0, m1, m2, n;
};

// the same exchange in every lane: after the six steps all 64 lanes hold the same bits
__device__ inline float butterfly(float v) {
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) v += __shfl_xor(v, step, h3d::kWave);
    return v;
}

struct Segments {
    const int64_t* __restrict__ vertex_order;              // [V]  vertex ids by (cluster, vertex id)
    const int64_t* __restrict__ vertex_offsets;            // [C + 1]
    const int64_t* __restrict__ record_order;              // [3T] corner records 3 t + k by (cluster, record id)
    const int64_t* __restrict__ record_offsets;            // [C + 1]
    const int32_t* __restrict__ cluster_cells;             // [C]
};

__global__ __launch_bounds__(kThreads) void mesh_cluster_solve_kernel(const float* __restrict__ vertices, int64_t V,
                                                                      const int32_t* __restrict__ faces, int64_t T, Segments s,
                                                                      int64_t C, ClusterGrid g, float lambda, float reach,
                                                                      float* __restrict__ out) {
    const int lane = threadIdx.x & (h3d::kWave - 1);
    const int64_t c = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);   // wave-uniform
    if (c >= C) return;
    const int64_t cells = (int64_t)g.nx * g.ny * g.nz;
    const int id = (int)clamp_index(s.cluster_cells[c], cells - 1);
    const int iz = id % g.nz, iy = (id / g.nz) % g.ny, ix = id / (g.nz * g.ny);
    const float cx = __fadd_rn(g.ox, __fmul_rn((float)ix + 0.5f, g.cell));
    const float cy = __fadd_rn(g.oy, __fmul_rn((float)iy + 0.5f, g.cell));
    const float cz = __fadd_rn(g.oz, __fmul_rn((float)iz + 0.5f, g.cell));

    Sums q = {};
    const int64_t v0 = clamp_index(s.vertex_offsets[c], V), v1 = clamp_index(s.vertex_offsets[c + 1], V);
    for (int64_t i = v0 + lane; i < v1; i += h3d::kWave) {
        const int64_t v = clamp_index(s.vertex_order[i], V - 1) * 3;
        q.m0 += vertices[v + 0] - cx;
        q.m1 += vertices[v + 1] - cy;
        q.m2 += vertices[v + 2] - cz;
        q.n += 1.f;
    }
    const int64_t r0 = clamp_index(s.record_offsets[c], 3 * T), r1 = clamp_index(s.record_offsets[c + 1], 3 * T);
    for (int64_t i = r0 + lane; i < r1; i += h3d::kWave) {
        const int64_t t = clamp_index(s.record_order[i], 3 * T - 1) / 3 * 3;
        const int64_t i0 = clamp_index(faces[t + 0], V - 1) * 3;
        const int64_t i1 = clamp_index(faces[t + 1], V - 1) * 3;
        const int64_t i2 = clamp_index(faces[t + 2], V - 1) * 3;
        const float px = vertices[i0 + 0] - cx, py = vertices[i0 + 1] - cy, pz = vertices[i0 + 2] - cz;
        const float ux = (vertices[i1 + 0] - cx) - px, uy = (vertices[i1 + 1] - cy) - py, uz = (vertices[i1 + 2] - cz) - pz;
        const float wx = (vertices[i2 + 0] - cx) - px, wy = (vertices[i2 + 1] - cy) - py, wz = (vertices[i2 + 2] - cz) - pz;
        const float mx = uy * wz - uz * wy, my = uz * wx - ux * wz, mz = ux * wy - uy * wx;
        const float len = sqrtf(mx * mx + my * my + mz * mz);
        if (!(len > 0.f && is_finite(len))) continue;        // no area, or a corner that is nowhere: the record adds nothing
        const float w = 1.f / (2.f * len);
        const float d = -(mx * px + my * py + mz * pz);
        const float sx = w * mx, sy = w * my, sz = w * mz;
        q.a00 += sx * mx, q.a01 += sx * my, q.a02 += sx * mz;
        q.a11 += sy * my, q.a12 += sy * mz, q.a22 += sz * mz;
        q.b0 += sx * d, q.b1 += sy * d, q.b2 += sz * d;
    }
    q.a00 = butterfly(q.a00), q.a01 = butterfly(q.a01), q.a02 = butterfly(q.a02);
    q.a11 = butterfly(q.a11), q.a12 = butterfly(q.a12), q.a22 = butterfly(q.a22);
    q.b0 = butterfly(q.b0), q.b1 = butterfly(q.b1), q.b2 = butterfly(q.b2);
    q.m0 = butterfly(q.m0), q.m1 = butterfly(q.m1), q.m2 = butterfly(q.m2), q.n = butterfly(q.n);

    // every lane holds the same sums and solves the same system; lane 0 stores
    const float e0 = q.m0 / q.n, e1 = q.m1 / q.n, e2 = q.m2 / q.n;         // an empty segment (lists of another mesh): 0 / 0, caught below
    float x0 = e0, x1 = e1, x2 = e2;
    const float trace = q.a00 + q.a11 + q.a22;
    if (trace > 0.f) {
        const float shift = lambda * trace;
        const float m00 = q.a00 + shift, m11 = q.a11 + shift, m22 = q.a22 + shift;
        const float f0 = q.a00 * e0 + q.a01 * e1 + q.a02 * e2 + q.b0;
        const float f1 = q.a01 * e0 + q.a11 * e1 + q.a12 * e2 + q.b1;
        const float f2 = q.a02 * e0 + q.a12 * e1 + q.a22 * e2 + q.b2;
        // Cholesky M = L L^T, then L y = f, L^T z = y
        const float l00 = sqrtf(m00);
        const float l10 = q.a01 / l00, l20 = q.a02 / l00;
        const float l11 = sqrtf(m11 - l10 * l10);
        const float l21 = (q.a12 - l20 * l10) / l11;
        const float l22 = sqrtf(m22 - l20 * l20 - l21 * l21);
        const float y0 = f0 / l00;
        const float y1 = (f1 - l10 * y0) / l11;
        const float y2 = (f2 - l20 * y0 - l21 * y1) / l22;
        const float z2 = y2 / l22;
        const float z1 = (y1 - l21 * z2) / l11;
        const float z0 = (y0 - l10 * z1 - l20 * z2) / l00;
        x0 = e0 - z0, x1 = e1 - z1, x2 = e2 - z2;
    }
    const float r = reach * g.cell;
    if (x0 != x0 || x1 != x1 || x2 != x2) x0 = x1 = x2 = 0.f;             // NaN on any axis: the cell centre
    x0 = fminf(fmaxf(x0, -r), r), x1 = fminf(fmaxf(x1, -r), r), x2 = fminf(fmaxf(x2, -r), r);
    if (lane == 0) {
        out[c * 3 + 0] = cx + x0;
        out[c * 3 + 1] = cy + x1;
        out[c * 3 + 2] = cz + x2;
    }
}

bool positive_finite(float v) { return v > 0.f && v <= 3.402823466e38f; }

bool finite3(const float* v) {
    return fabsf(v[0]) <= 3.402823466e38f && fabsf(v[1]) <= 3.402823466e38f && fabsf(v[2]) <= 3.402823466e38f;
}

constexpr int64_t kInt32 = (int64_t)1 << 31;

}  // namespace

#define H3D_REQUIRE_CLUSTER_GRID(name)                                                                                                 \
    H3D_REQUIRE(origin, name ": null pointer");                                                                                        \
    H3D_REQUIRE(finite3(origin), name ": origin must be finite");                                                                      \
    H3D_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, name ": counts (%d, %d, %d) must be positive", nx, ny, nz);                             \
    H3D_REQUIRE((int64_t)nx * ny < kInt32 && (int64_t)nx * ny * nz < kInt32, name ": the cluster grid %d x %d x %d has 2^31 cells or " \
                "more", nx, ny, nz)

extern "C" int h3d_mesh_cluster_cells(const float* vertices, int64_t V, const float* origin, float inv_cell, int nx, int ny, int nz,
                                      int32_t* cells, h3d_stream_t stream) {
    H3D_REQUIRE_CLUSTER_GRID("h3d_mesh_cluster_cells");
    H3D_REQUIRE(positive_finite(inv_cell), "h3d_mesh_cluster_cells: inv_cell=%g must be positive and finite", inv_cell);
    H3D_REQUIRE(V >= 0 && V < kInt32, "h3d_mesh_cluster_cells: V=%lld out of range", (long long)V);
    if (V == 0) return H3D_OK;
    H3D_REQUIRE(vertices && cells, "h3d_mesh_cluster_cells: null pointer");
    h3d::pre_launch();
    hipLaunchKernelGGL(mesh_cluster_cells_kernel, dim3((unsigned)((V + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), vertices, V,
                       ClusterGrid{origin[0], origin[1], origin[2], 0.f, inv_cell, nx, ny, nz}, cells);
    return h3d::launch_status("h3d_mesh_cluster_cells");
}

extern "C" int h3d_mesh_cluster_faces(const int32_t* faces, int64_t T, const int32_t* cluster, int64_t V, int32_t* out_faces,
                                      uint8_t* keep, int32_t* keys, h3d_stream_t stream) {
    H3D_REQUIRE(T >= 0 && 3 * T < kInt32, "h3d_mesh_cluster_faces: T=%lld: 3 T must stay below 2^31", (long long)T);
    H3D_REQUIRE(V >= 0 && V < kInt32, "h3d_mesh_cluster_faces: V=%lld out of range", (long long)V);
    H3D_REQUIRE(T == 0 || V >= 1, "h3d_mesh_cluster_faces: %lld triangles without a vertex", (long long)T);
    if (T == 0) return H3D_OK;
    H3D_REQUIRE(faces && cluster && out_faces && keep && keys, "h3d_mesh_cluster_faces: null pointer");
    h3d::pre_launch();
    hipLaunchKernelGGL(mesh_cluster_faces_kernel, dim3((unsigned)((T + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), faces, T, cluster, V, out_faces, keep, keys);
    return h3d::launch_status("h3d_mesh_cluster_faces");
}

extern "C" int h3d_mesh_cluster_solve(const float* vertices, int64_t V, const int32_t* faces, int64_t T, const int64_t* vertex_order,
                                      const int64_t* vertex_offsets, const int64_t* record_order, const int64_t* record_offsets,
                                      const int32_t* cluster_cells, int64_t C, const float* origin, float cell, int nx, int ny, int nz,
                                      float regularization, float reach, float* out, h3d_stream_t stream) {
    H3D_REQUIRE_CLUSTER_GRID("h3d_mesh_cluster_solve");
    H3D_REQUIRE(positive_finite(cell), "h3d_mesh_cluster_solve: cell=%g must be positive and finite", cell);
    H3D_REQUIRE(positive_finite(regularization), "h3d_mesh_cluster_solve: regularization=%g must be positive", regularization);
    H3D_REQUIRE(reach >= 0.5f && reach <= 3.402823466e38f, "h3d_mesh_cluster_solve: reach=%g must be at least 0.5", reach);
    H3D_REQUIRE(T >= 0 && 3 * T < kInt32, "h3d_mesh_cluster_solve: T=%lld: 3 T must stay below 2^31", (long long)T);
    H3D_REQUIRE(V >= 0 && V < kInt32, "h3d_mesh_cluster_solve: V=%lld out of range", (long long)V);
    H3D_REQUIRE(C >= 0 && C <= V, "h3d_mesh_cluster_solve: C=%lld clusters of V=%lld vertices", (long long)C, (long long)V);
    if (C == 0) return H3D_OK;
    H3D_REQUIRE(vertices && vertex_order && vertex_offsets && record_offsets && cluster_cells && out,
                "h3d_mesh_cluster_solve: null pointer");
    H3D_REQUIRE(T == 0 || (faces && record_order), "h3d_mesh_cluster_solve: null pointer");
    h3d::pre_launch();
    hipLaunchKernelGGL(mesh_cluster_solve_kernel, dim3((unsigned)((C + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), vertices, V, faces, T,
                       Segments{vertex_order, vertex_offsets, record_order, record_offsets, cluster_cells}, C,
                       ClusterGrid{origin[0], origin[1], origin[2], cell, 0.f, nx, ny, nz}, regularization, reach, out);
    return h3d::launch_status("h3d_mesh_cluster_solve");
}
