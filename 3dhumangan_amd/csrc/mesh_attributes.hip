// Per-vertex attributes of an extracted mesh: normals from the density grid and colours carried over from rendered views.  See
// include/h3d.h (h3d_isosurface_normals / h3d_mesh_project_colors) for both definitions.
//
// Both kernels: one thread per vertex, 256 threads, no LDS, no atomics -- every sum is taken in registers in a fixed order, so two
// runs give the same bits.  Every index that addresses memory comes from a float clamped with fmaxf / fminf (which drop a NaN) before
// the conversion to int, so a non-finite position loads in range; every store is guarded by V.
//
// Normals: the eight nodes of the vertex's cell need the central (at the border: one-sided) difference along each axis; their
// stencils overlap in 32 distinct values of the 4 x 4 x 4 block around the cell (the 8 corners and, per axis, the 4 + 4 values one node
// below and above them), each loaded once.  The trilinear weights of the two other axes are applied to the DIFFERENCES first and the
// two divisions per axis follow: six divisions per vertex instead of 24, and the same function.  Vertices arrive in ascending edge id,
// so neighbouring threads read neighbouring cells and the block's lines are shared through L1 / L2.
//
// Colours: the views run in a loop; the per-view camera table (12 world-to-camera entries, the origin, the focal) is read at a
// wave-uniform index, i.e. through the scalar cache.  Each view costs a vertex 4 depth and 12 image texels.
//
// Texture (h3d_mesh_bake_texture): the same per-point colour at every texel of an atlas that gives each triangle half of a square
// cell; one thread per texel, a wave on an 8 x 8 texel block.  Face indices are clamped into the vertex range before they address
// memory; every store is guarded by the texture's edge.
#include "common.hpp"

namespace {

constexpr int kThreads = 256;

struct Grid {
    int Nx, Ny, Nz;
};

struct Frame {
    float ox, oy, oz, sx, sy, sz;
};

__device__ inline float lerp(float a, float b, float f) { return a + f * (b - a); }

__device__ inline bool is_finite(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN and +-inf

// grid coordinate -> cell c in [0, N - 2] and fraction g - c in [0, 1]
__device__ inline void locate(float g, int N, int& c, float& f) {
    g = fminf(fmaxf(g, 0.f), (float)(N - 1));             // NaN -> 0
    c = min((int)floorf(g), N - 2);
    f = g - (float)c;
}

__global__ __launch_bounds__(kThreads) void isosurface_normals_kernel(const float* __restrict__ volume, Grid g, Frame fr,
                                                                      const float* __restrict__ vertices, int64_t V,
                                                                      float* __restrict__ normals, float* __restrict__ gradient) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= V) return;
    const float px = vertices[i * 3 + 0], py = vertices[i * 3 + 1], pz = vertices[i * 3 + 2];
    int cx, cy, cz;
    float fx, fy, fz;
    locate((px - fr.ox) / fr.sx, g.Nx, cx, fx);
    locate((py - fr.oy) / fr.sy, g.Ny, cy, fy);
    locate((pz - fr.oz) / fr.sz, g.Nz, cz, fz);
    // along each axis: the node below the cell and the node above it, clamped to the grid (then the difference is one-sided)
    const int mx = max(cx - 1, 0), qx = min(cx + 2, g.Nx - 1);
    const int my = max(cy - 1, 0), qy = min(cy + 2, g.Ny - 1);
    const int mz = max(cz - 1, 0), qz = min(cz + 2, g.Nz - 1);
    const size_t sY = (size_t)g.Nz, sX = (size_t)g.Ny * g.Nz;
    auto at = [&](int x, int y, int z) { return volume[x * sX + y * sY + z]; };

    float c[2][2][2];                                      // the cell's corners
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int d = 0; d < 2; ++d) c[a][b][d] = at(cx + a, cy + b, cz + d);

    // axis x: differences at node cx (lo) and node cx + 1 (hi), bilinear over (y, z), then one division each
    float lo[2][2], hi[2][2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            lo[b][d] = c[1][b][d] - at(mx, cy + b, cz + d);
            hi[b][d] = at(qx, cy + b, cz + d) - c[0][b][d];
        }
    float g0 = lerp(lerp(lo[0][0], lo[0][1], fz), lerp(lo[1][0], lo[1][1], fz), fy) / ((float)(cx + 1 - mx) * fr.sx);
    float g1 = lerp(lerp(hi[0][0], hi[0][1], fz), lerp(hi[1][0], hi[1][1], fz), fy) / ((float)(qx - cx) * fr.sx);
    float Gx = lerp(g0, g1, fx);

#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            lo[a][d] = c[a][1][d] - at(cx + a, my, cz + d);
            hi[a][d] = at(cx + a, qy, cz + d) - c[a][0][d];
        }
    g0 = lerp(lerp(lo[0][0], lo[0][1], fz), lerp(lo[1][0], lo[1][1], fz), fx) / ((float)(cy + 1 - my) * fr.sy);
    g1 = lerp(lerp(hi[0][0], hi[0][1], fz), lerp(hi[1][0], hi[1][1], fz), fx) / ((float)(qy - cy) * fr.sy);
    float Gy = lerp(g0, g1, fy);

#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            lo[a][b] = c[a][b][1] - at(cx + a, cy + b, mz);
            hi[a][b] = at(cx + a, cy + b, qz) - c[a][b][0];
        }
    g0 = lerp(lerp(lo[0][0], lo[0][1], fy), lerp(lo[1][0], lo[1][1], fy), fx) / ((float)(cz + 1 - mz) * fr.sz);
    g1 = lerp(lerp(hi[0][0], hi[0][1], fy), lerp(hi[1][0], hi[1][1], fy), fx) / ((float)(qz - cz) * fr.sz);
    float Gz = lerp(g0, g1, fz);

    if (!(is_finite(px) && is_finite(py) && is_finite(pz))) Gx = Gy = Gz = 0.f;     // a vertex that is nowhere has no gradient
    if (gradient) {
        gradient[i * 3 + 0] = Gx;
        gradient[i * 3 + 1] = Gy;
        gradient[i * 3 + 2] = Gz;
    }
    const float len = sqrtf(Gx * Gx + Gy * Gy + Gz * Gz);
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (len > 0.f && is_finite(len)) nx = -Gx / len, ny = -Gy / len, nz = -Gz / len;
    normals[i * 3 + 0] = nx;
    normals[i * 3 + 1] = ny;
    normals[i * 3 + 2] = nz;
}

struct Views {
    int K, H, W, h, w;
};

// bilinear sample of a [rows, cols] plane at (x, y), both clamped to the plane
__device__ inline void bilinear_taps(float x, float y, int cols, int rows, int& x0, int& x1, int& y0, int& y1, float& ax, float& ay) {
    x = fminf(fmaxf(x, 0.f), (float)(cols - 1));          // NaN -> 0
    y = fminf(fmaxf(y, 0.f), (float)(rows - 1));
    x0 = min((int)floorf(x), cols - 1), y0 = min((int)floorf(y), rows - 1);
    x1 = min(x0 + 1, cols - 1), y1 = min(y0 + 1, rows - 1);
    ax = x - (float)x0, ay = y - (float)y0;
}

__device__ inline float bilinear_at(const float* __restrict__ plane, int cols, int x0, int x1, int y0, int y1, float ax, float ay) {
    const float* r0 = plane + (size_t)y0 * cols;
    const float* r1 = plane + (size_t)y1 * cols;
    return lerp(lerp(r0[x0], r0[x1], ax), lerp(r1[x0], r1[x1], ax), ay);
}

// The K views of one surface point (position p, normal n): sum = sum_k w_k and the w_k-weighted colour sums, the views in
// ascending k -- the definition of h3d_mesh_project_colors, shared by the per-vertex and the per-texel kernel.
__device__ inline void blend_views(float px, float py, float pz, float nx, float ny, float nz, const float* __restrict__ images,
                                   const float* __restrict__ depths, const float* __restrict__ table, const Views& s,
                                   float depth_tolerance, int normal_power, float& sum, float& r, float& g, float& b) {
    const float span = (float)s.w / (float)s.h;
    const float wm = (float)(s.w - 1), hm = (float)(s.h - 1);
    const float ratio_x = (float)s.W / (float)s.w, ratio_y = (float)s.H / (float)s.h;
    const size_t plane = (size_t)s.H * s.W;
    sum = 0.f, r = 0.f, g = 0.f, b = 0.f;
    for (int k = 0; k < s.K; ++k) {
        const float* __restrict__ M = table + (size_t)k * 16;           // wave-uniform
        const float cx = M[0] * px + M[1] * py + M[2] * pz + M[3];
        const float cy = M[4] * px + M[5] * py + M[6] * pz + M[7];
        const float cz = M[8] * px + M[9] * py + M[10] * pz + M[11];
        const float focal = M[15];
        const bool ok = cz > 1e-6f;
        const float u = (focal * cx / cz + span) / (2.f * span) * wm;
        const float v = (focal * cy / cz + 1.f) / 2.f * hm;
        const float dx = px - M[12], dy = py - M[13], dz = pz - M[14];
        const float t = sqrtf(dx * dx + dy * dy + dz * dz);
        const float base = fmaxf(0.f, -(nx * (dx / t) + ny * (dy / t) + nz * (dz / t)));
        float face = base;
        for (int e = 1; e < normal_power; ++e) face *= base;
        const float edge = fminf(fmaxf(fminf(fminf(u, wm - u), fminf(v, hm - v)), 0.f), 1.f);
        int x0, x1, y0, y1;
        float ax, ay;
        bilinear_taps(u, v, s.w, s.h, x0, x1, y0, y1, ax, ay);
        const float D = bilinear_at(depths + (size_t)k * s.h * s.w, s.w, x0, x1, y0, y1, ax, ay);
        const float vis = fminf(fmaxf(1.f - fabsf(t - D) / depth_tolerance, 0.f), 1.f);
        const float wk = edge * vis * face;
        if (!(ok && wk > 0.f && is_finite(wk))) continue;                  // a non-finite weight counts as 0
        bilinear_taps((u + 0.5f) * ratio_x - 0.5f, (v + 0.5f) * ratio_y - 0.5f, s.W, s.H, x0, x1, y0, y1, ax, ay);
        const float* im = images + (size_t)k * 3 * plane;
        sum += wk;
        r += wk * bilinear_at(im, s.W, x0, x1, y0, y1, ax, ay);
        g += wk * bilinear_at(im + plane, s.W, x0, x1, y0, y1, ax, ay);
        b += wk * bilinear_at(im + 2 * plane, s.W, x0, x1, y0, y1, ax, ay);
    }
}

__global__ __launch_bounds__(kThreads) void mesh_project_colors_kernel(const float* __restrict__ vertices,
                                                                       const float* __restrict__ normals, int64_t V,
                                                                       const float* __restrict__ images,
                                                                       const float* __restrict__ depths,
                                                                       const float* __restrict__ table, Views s,
                                                                       float depth_tolerance, int normal_power, float fill, float eps,
                                                                       float* __restrict__ colors, float* __restrict__ coverage) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= V) return;
    const float px = vertices[i * 3 + 0], py = vertices[i * 3 + 1], pz = vertices[i * 3 + 2];
    const float nx = normals[i * 3 + 0], ny = normals[i * 3 + 1], nz = normals[i * 3 + 2];
    float sum, r, g, b;
    blend_views(px, py, pz, nx, ny, nz, images, depths, table, s, depth_tolerance, normal_power, sum, r, g, b);
    const float den = sum + eps, back = eps * fill;
    colors[i * 3 + 0] = (r + back) / den;
    colors[i * 3 + 1] = (g + back) / den;
    colors[i * 3 + 2] = (b + back) / den;
    coverage[i] = sum;
}

struct Atlas {
    int S, R, c;                                           // texture edge, cells per row, cell edge in texels
};

// One thread per texel; a wave covers an 8 x 8 texel block (a workgroup 16 x 16), so it sees one to four triangles and their nine
// vertex / normal loads are shared through L1.  Every face index is clamped into [0, V - 1]; every store is guarded by S.
__global__ __launch_bounds__(kThreads) void mesh_bake_texture_kernel(const float* __restrict__ vertices,
                                                                     const float* __restrict__ normals, int64_t V,
                                                                     const int32_t* __restrict__ faces, int64_t T, Atlas a,
                                                                     const float* __restrict__ images,
                                                                     const float* __restrict__ depths,
                                                                     const float* __restrict__ table, Views s,
                                                                     float depth_tolerance, int normal_power, float fill, float eps,
                                                                     float* __restrict__ texture, float* __restrict__ coverage) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);                  // column
    const int row = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (q >= a.S || row >= a.S) return;
    const int cy = row / a.c, cx = q / a.c;
    const int j = row - cy * a.c, i = q - cx * a.c;
    const bool upper = i + j >= a.c - 1;
    const int64_t t = 2 * ((int64_t)cy * a.R + cx) + (upper ? 1 : 0);
    const size_t texel = (size_t)row * a.S + q;
    float sum = 0.f, r = 0.f, g = 0.f, b = 0.f;
    float den = 1.f, back = fill;                          // an unowned texel: the fill colour itself, coverage 0
    if (cy < a.R && cx < a.R && t < T) {
        const int ii = upper ? a.c - 1 - i : i, jj = upper ? a.c - 1 - j : j;
        const float m = (float)(a.c - 3);
        const float b1 = (float)ii / m, b2 = (float)jj / m;
        const float b0 = 1.f - b1 - b2;
        const int64_t top = V - 1;
        const int64_t i0 = min(max((int64_t)faces[t * 3 + 0], (int64_t)0), top) * 3;
        const int64_t i1 = min(max((int64_t)faces[t * 3 + 1], (int64_t)0), top) * 3;
        const int64_t i2 = min(max((int64_t)faces[t * 3 + 2], (int64_t)0), top) * 3;
        const float px = b0 * vertices[i0 + 0] + b1 * vertices[i1 + 0] + b2 * vertices[i2 + 0];
        const float py = b0 * vertices[i0 + 1] + b1 * vertices[i1 + 1] + b2 * vertices[i2 + 1];
        const float pz = b0 * vertices[i0 + 2] + b1 * vertices[i1 + 2] + b2 * vertices[i2 + 2];
        float nx = b0 * normals[i0 + 0] + b1 * normals[i1 + 0] + b2 * normals[i2 + 0];
        float ny = b0 * normals[i0 + 1] + b1 * normals[i1 + 1] + b2 * normals[i2 + 1];
        float nz = b0 * normals[i0 + 2] + b1 * normals[i1 + 2] + b2 * normals[i2 + 2];
        const float len = sqrtf(nx * nx + ny * ny + nz * nz);
        if (len > 0.f && is_finite(len)) nx /= len, ny /= len, nz /= len;
        else nx = ny = nz = 0.f;
        blend_views(px, py, pz, nx, ny, nz, images, depths, table, s, depth_tolerance, normal_power, sum, r, g, b);
        den = sum + eps, back = eps * fill;
    }
    texture[texel * 3 + 0] = (r + back) / den;
    texture[texel * 3 + 1] = (g + back) / den;
    texture[texel * 3 + 2] = (b + back) / den;
    coverage[texel] = sum;
}

bool positive_finite(float v) { return v > 0.f && v <= 3.402823466e38f; }

}  // namespace

// what h3d_mesh_project_colors and h3d_mesh_bake_texture both ask of the views
static int check_views(const char* who, int K, int H, int W, int h, int w, float depth_tolerance, float eps, int normal_power) {
    H3D_REQUIRE(K >= 1, "%s: K=%d views (at least 1)", who, K);
    H3D_REQUIRE(H >= 2 && W >= 2 && h >= 2 && w >= 2, "%s: images %dx%d and depths %dx%d need at least 2x2", who, H, W, h, w);
    H3D_REQUIRE((int64_t)K * 3 * H * W < ((int64_t)1 << 40) && (int64_t)K * h * w < ((int64_t)1 << 40), "%s: views too large", who);
    H3D_REQUIRE(positive_finite(depth_tolerance), "%s: depth_tolerance=%g must be positive", who, depth_tolerance);
    H3D_REQUIRE(positive_finite(eps), "%s: eps=%g must be positive", who, eps);
    H3D_REQUIRE(normal_power >= 1 && normal_power <= 8, "%s: normal_power=%d outside 1..8", who, normal_power);
    return H3D_OK;
}

extern "C" int h3d_isosurface_normals(const float* volume, int Nx, int Ny, int Nz, const float* origin, const float* spacing,
                                      const float* vertices, int64_t V, float* normals, float* gradient, h3d_stream_t stream) {
    H3D_REQUIRE(volume && origin && spacing, "h3d_isosurface_normals: null pointer");
    H3D_REQUIRE(Nx >= 2 && Ny >= 2 && Nz >= 2, "h3d_isosurface_normals: every axis needs at least 2 nodes (Nx=%d Ny=%d Nz=%d)", Nx, Ny,
                Nz);
    H3D_REQUIRE(positive_finite(spacing[0]) && positive_finite(spacing[1]) && positive_finite(spacing[2]),
                "h3d_isosurface_normals: spacing (%g, %g, %g) must be positive and finite", spacing[0], spacing[1], spacing[2]);
    H3D_REQUIRE(fabsf(origin[0]) <= 3.402823466e38f && fabsf(origin[1]) <= 3.402823466e38f && fabsf(origin[2]) <= 3.402823466e38f,
                "h3d_isosurface_normals: origin must be finite");
    H3D_REQUIRE(V >= 0 && V < ((int64_t)1 << 31) * kThreads, "h3d_isosurface_normals: V=%lld out of range", (long long)V);
    if (V == 0) return H3D_OK;
    H3D_REQUIRE(vertices && normals, "h3d_isosurface_normals: null pointer");
    h3d::pre_launch();
    hipLaunchKernelGGL(isosurface_normals_kernel, dim3((unsigned)((V + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), volume, Grid{Nx, Ny, Nz},
                       Frame{origin[0], origin[1], origin[2], spacing[0], spacing[1], spacing[2]}, vertices, V, normals, gradient);
    return h3d::launch_status("h3d_isosurface_normals");
}

extern "C" int h3d_mesh_project_colors(const float* vertices, const float* normals, int64_t V, const float* images, int K, int H,
                                       int W, const float* depths, int h, int w, const float* table, float depth_tolerance,
                                       int normal_power, float fill, float eps, float* colors, float* coverage,
                                       h3d_stream_t stream) {
    if (int rc = check_views("h3d_mesh_project_colors", K, H, W, h, w, depth_tolerance, eps, normal_power)) return rc;
    H3D_REQUIRE(V >= 0 && V < ((int64_t)1 << 31) * kThreads, "h3d_mesh_project_colors: V=%lld out of range", (long long)V);
    if (V == 0) return H3D_OK;
    H3D_REQUIRE(vertices && normals && images && depths && table && colors && coverage, "h3d_mesh_project_colors: null pointer");
    h3d::pre_launch();
    hipLaunchKernelGGL(mesh_project_colors_kernel, dim3((unsigned)((V + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), vertices, normals, V, images, depths, table, Views{K, H, W, h, w},
                       depth_tolerance, normal_power, fill, eps, colors, coverage);
    return h3d::launch_status("h3d_mesh_project_colors");
}

extern "C" int h3d_mesh_bake_texture(const float* vertices, const float* normals, int64_t V, const int32_t* faces, int64_t T, int S,
                                     const float* images, int K, int H, int W, const float* depths, int h, int w, const float* table,
                                     float depth_tolerance, int normal_power, float fill, float eps, float* texture, float* coverage,
                                     h3d_stream_t stream) {
    H3D_REQUIRE(S >= 2 && S <= 8192, "h3d_mesh_bake_texture: S=%d outside 2..8192", S);
    H3D_REQUIRE(T >= 0 && T <= 2 * (int64_t)2048 * 2048, "h3d_mesh_bake_texture: T=%lld out of range", (long long)T);
    const int64_t cells = (T + 1) / 2;
    int R = 1;                                             // ceil(sqrt(cells)) = isqrt(cells - 1) + 1 in integers
    if (cells > 1) {
        int64_t root = (int64_t)sqrt((double)(cells - 1));
        while (root * root > cells - 1) --root;
        while ((root + 1) * (root + 1) <= cells - 1) ++root;
        R = (int)root + 1;
    }
    const int c = S / R;
    H3D_REQUIRE(c >= 4, "h3d_mesh_bake_texture: T=%lld triangles need a texture of at least %d texels a side (cells of 4), got S=%d",
                (long long)T, 4 * R, S);
    if (int rc = check_views("h3d_mesh_bake_texture", K, H, W, h, w, depth_tolerance, eps, normal_power)) return rc;
    H3D_REQUIRE(V >= 0 && V < ((int64_t)1 << 31), "h3d_mesh_bake_texture: V=%lld out of range", (long long)V);
    H3D_REQUIRE(T == 0 || V >= 1, "h3d_mesh_bake_texture: %lld triangles without a vertex", (long long)T);
    H3D_REQUIRE(texture && coverage, "h3d_mesh_bake_texture: null pointer");
    H3D_REQUIRE(T == 0 || (vertices && normals && faces && images && depths && table), "h3d_mesh_bake_texture: null pointer");
    h3d::pre_launch();
    const unsigned blocks = (unsigned)((S + 15) / 16);
    hipLaunchKernelGGL(mesh_bake_texture_kernel, dim3(blocks, blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), vertices,
                       normals, V, faces, T, Atlas{S, R, c}, images, depths, table, Views{K, H, W, h, w}, depth_tolerance, normal_power,
                       fill, eps, texture, coverage);
    return h3d::launch_status("h3d_mesh_bake_texture");
}
