// Iso-surface of a density volume as an indexed triangle mesh: marching tetrahedra on the Kuhn (Freudenthal) split of every grid
// cell.  See include/h3d.h (h3d_isosurface_count / h3d_isosurface_emit) for the definition: ids, orientation and output order.
//
// Two launches with the caller's prefix sums between them.  Both walk the grid in tiles of kTX x kTY x kTZ nodes (z is the
// contiguous axis), one 256-thread workgroup per tile, and stage the tile's values with a halo on the upper side in LDS: a node's
// seven edges and the cell it is the lowest corner of read nodes p + {0,1}^3 only, so the halo is one node for the count.  The emit
// needs the crossing masks of the tile's upper neighbours as well (a face names a vertex by its rank among the edges of the
// vertex's lower node), hence two nodes of halo there, and it keeps mask and vertex base of every node of the tile + 1 in LDS.
// Each value is then read from memory (1 + h/8)(1 + h/8)(1 + h/16) times, h = 1 or 2, instead of 8 + 14 times.
//
// No atomics: every vertex and every face has its slot from the prefix sums, so two runs give the same bits.  Every store is guarded
// by the output sizes V and T, so prefix sums that do not belong to the volume (or a volume that changed between the launches)
// cannot send a store out of range.
#include "common.hpp"

namespace {

constexpr int kTX = 8, kTY = 8, kTZ = 16;
constexpr int kThreads = 256;
constexpr int kTileNodes = kTX * kTY * kTZ;

// corner c of a cell as bits: x = c & 1, y = (c >> 1) & 1, z = c >> 2
// tetrahedron k = the k-th permutation pi of the axes in lexicographic order: corners 0, e_pi1, e_pi1 + e_pi2, 7
struct Tables {
    unsigned char tet[6][4];      // corner codes of v0..v3
    unsigned char ntri[16];       // triangles of a case (bit i of the case: v_i inside)
    unsigned char tri[16][2][3];  // edges as (a << 2 | b), a < b tetrahedron vertices, oriented for an EVEN permutation
    unsigned char type[8];        // direction code -> edge type, for the emit's face loop (a load, measured faster than type_of there)
};

constexpr int perm_sign4(int a, int b, int c, int d) {
    const int p[4] = {a, b, c, d};
    int s = 1;
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (p[i] > p[j]) s = -s;
    return s;
}

// edge type 0..6 <-> direction code (bits x, y, z): (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1) = codes 1 2 4 3 5 6 7
constexpr int code_of(int type) { return type == 0 ? 1 : type == 1 ? 2 : type == 2 ? 4 : type == 3 ? 3 : type + 1; }
constexpr int type_of(int code) { return code == 1 ? 0 : code == 2 ? 1 : code == 4 ? 2 : code == 3 ? 3 : code - 1; }

constexpr unsigned char edge_code(int a, int b) { return (unsigned char)(a < b ? (a << 2 | b) : (b << 2 | a)); }

// The rule behind the 16 cases.  In a tetrahedron with det(v1 - v0, v2 - v0, v3 - v0) > 0 (an even permutation of the axes):
//   one vertex i on its own side, the others j < k < l: the triangle (ij, ik, il) points away from i iff (i, j, k, l) is an even
//     permutation of (0, 1, 2, 3); it must point away from i when i is inside and towards i when i is outside;
//   two inside i0 < i1, two outside o0 < o1: the quad (i0o0, i0o1, i1o1, i1o0) points from inside to outside iff (i0, i1, o0, o1)
//     is even; it is split along i0o0 - i1o1.
// A wrong orientation is mended by swapping the last two corners of each triangle.  The normal thus follows from the case and the
// tetrahedron alone, never from interpolated positions.
constexpr Tables make_tables() {
    Tables t{};
    const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (int k = 0; k < 6; ++k) {
        t.tet[k][0] = 0;
        t.tet[k][1] = (unsigned char)(1 << perms[k][0]);
        t.tet[k][2] = (unsigned char)(1 << perms[k][0] | 1 << perms[k][1]);
        t.tet[k][3] = 7;
    }
    for (int code = 1; code < 8; ++code) t.type[code] = (unsigned char)type_of(code);
    for (int c = 0; c < 16; ++c) {
        int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
        for (int v = 0; v < 4; ++v) {
            if (c >> v & 1) in[ni++] = v;
            else out[no++] = v;
        }
        if (ni == 0 || ni == 4) {
            t.ntri[c] = 0;
        } else if (ni == 2) {
            t.ntri[c] = 2;
            const bool keep = perm_sign4(in[0], in[1], out[0], out[1]) > 0;
            const unsigned char q0 = edge_code(in[0], out[0]), q1 = edge_code(in[0], out[1]), q2 = edge_code(in[1], out[1]),
                                q3 = edge_code(in[1], out[0]);
            t.tri[c][0][0] = q0, t.tri[c][0][1] = keep ? q1 : q2, t.tri[c][0][2] = keep ? q2 : q1;
            t.tri[c][1][0] = q0, t.tri[c][1][1] = keep ? q2 : q3, t.tri[c][1][2] = keep ? q3 : q2;
        } else {
            t.ntri[c] = 1;
            const int i = ni == 1 ? in[0] : out[0];
            const int* o = ni == 1 ? out : in;
            const bool away = perm_sign4(i, o[0], o[1], o[2]) > 0;
            const bool keep = ni == 1 ? away : !away;
            t.tri[c][0][0] = edge_code(i, o[0]);
            t.tri[c][0][1] = edge_code(i, keep ? o[1] : o[2]);
            t.tri[c][0][2] = edge_code(i, keep ? o[2] : o[1]);
        }
    }
    return t;
}

__constant__ Tables kTab = make_tables();


struct Grid {
    int Nx, Ny, Nz;
};

__device__ inline bool inside(float v, float level) { return v > level; }   // NaN and v == level are outside

// values of the tile's nodes and H halo nodes on the upper side of each axis -> LDS; nodes outside the grid read as 0 (never used:
// an edge or a cell that would read one does not exist)
template <int H>
__device__ inline void stage_values(const float* __restrict__ volume, Grid g, int x0, int y0, int z0, float* s_val) {
    constexpr int SY = kTY + H, SZ = kTZ + H, n = (kTX + H) * SY * SZ;
    for (int l = threadIdx.x; l < n; l += kThreads) {
        const int lz = l % SZ, ly = (l / SZ) % SY, lx = l / (SZ * SY);
        const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
        float v = 0.f;
        if (x < g.Nx && y < g.Ny && z < g.Nz) v = volume[((size_t)x * g.Ny + y) * g.Nz + z];
        s_val[l] = v;
    }
}

// bit t of the result: edge type t of node (x, y, z) exists and crosses the level.  s_val is a tile with halo H; (lx, ly, lz) and
// their upper neighbours lie inside it.
template <int H>
__device__ inline unsigned crossing_mask(const float* s_val, Grid g, int x, int y, int z, int lx, int ly, int lz, float level) {
    constexpr int SY = kTY + H, SZ = kTZ + H;
    if (x >= g.Nx || y >= g.Ny || z >= g.Nz) return 0u;
    const bool a = inside(s_val[(lx * SY + ly) * SZ + lz], level);
    const bool ex = x + 1 < g.Nx, ey = y + 1 < g.Ny, ez = z + 1 < g.Nz;
    unsigned m = 0;
#pragma unroll
    for (int code = 1; code < 8; ++code) {
        const int dx = code & 1, dy = code >> 1 & 1, dz = code >> 2;
        const bool exists = (!dx || ex) && (!dy || ey) && (!dz || ez);
        const bool b = inside(s_val[((lx + dx) * SY + ly + dy) * SZ + lz + dz], level);
        if (exists && a != b) m |= 1u << type_of(code);
    }
    return m;
}

// bit c of the result: corner c of the cell whose lowest corner is (lx, ly, lz) is inside
template <int H>
__device__ inline unsigned corner_bits(const float* s_val, int lx, int ly, int lz, float level) {
    constexpr int SY = kTY + H, SZ = kTZ + H;
    unsigned bits = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        if (inside(s_val[((lx + (c & 1)) * SY + ly + (c >> 1 & 1)) * SZ + lz + (c >> 2)], level)) bits |= 1u << c;
    return bits;
}

__device__ inline unsigned tet_case(unsigned bits, int k) {
    return (bits & 1u) | (bits >> kTab.tet[k][1] & 1u) << 1 | (bits >> kTab.tet[k][2] & 1u) << 2 | (bits >> 7 & 1u) << 3;
}

__global__ __launch_bounds__(kThreads) void isosurface_count_kernel(const float* __restrict__ volume, Grid g, float level,
                                                                    int32_t* __restrict__ vertex_counts,
                                                                    int32_t* __restrict__ triangle_counts) {
    __shared__ float s_val[(kTX + 1) * (kTY + 1) * (kTZ + 1)];
    const int x0 = blockIdx.z * kTX, y0 = blockIdx.y * kTY, z0 = blockIdx.x * kTZ;
    stage_values<1>(volume, g, x0, y0, z0, s_val);
    __syncthreads();
    for (int l = threadIdx.x; l < kTileNodes; l += kThreads) {
        const int lz = l % kTZ, ly = (l / kTZ) % kTY, lx = l / (kTZ * kTY);
        const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
        if (x >= g.Nx || y >= g.Ny || z >= g.Nz) continue;
        vertex_counts[(x * g.Ny + y) * g.Nz + z] = __popc(crossing_mask<1>(s_val, g, x, y, z, lx, ly, lz, level));
        if (x + 1 < g.Nx && y + 1 < g.Ny && z + 1 < g.Nz) {
            const unsigned bits = corner_bits<1>(s_val, lx, ly, lz, level);
            int n = 0;
            if (bits != 0u && bits != 255u) {
#pragma unroll
                for (int k = 0; k < 6; ++k) n += kTab.ntri[tet_case(bits, k)];
            }
            triangle_counts[(x * (g.Ny - 1) + y) * (g.Nz - 1) + z] = n;
        }
    }
}

struct Frame {
    float ox, oy, oz, sx, sy, sz;
};

__global__ __launch_bounds__(kThreads) void isosurface_emit_kernel(const float* __restrict__ volume, Grid g, float level, Frame f,
                                                                   const int32_t* __restrict__ vertex_offsets,
                                                                   const int64_t* __restrict__ triangle_offsets,
                                                                   float* __restrict__ vertices, int64_t V,
                                                                   int32_t* __restrict__ faces, int64_t T) {
    constexpr int SY = kTY + 2, SZ = kTZ + 2;           // value tile, halo 2
    constexpr int MY = kTY + 1, MZ = kTZ + 1;           // mask / vertex-base tile, halo 1
    __shared__ float s_val[(kTX + 2) * SY * SZ];
    __shared__ int32_t s_base[(kTX + 1) * MY * MZ];
    __shared__ unsigned char s_mask[(kTX + 1) * MY * MZ];
    const int x0 = blockIdx.z * kTX, y0 = blockIdx.y * kTY, z0 = blockIdx.x * kTZ;
    stage_values<2>(volume, g, x0, y0, z0, s_val);
    __syncthreads();

    // masks and vertex bases of the tile + 1; the tile's own nodes write their vertices
    for (int l = threadIdx.x; l < (kTX + 1) * MY * MZ; l += kThreads) {
        const int lz = l % MZ, ly = (l / MZ) % MY, lx = l / (MZ * MY);
        const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
        const unsigned m = crossing_mask<2>(s_val, g, x, y, z, lx, ly, lz, level);
        int32_t base = 0;
        if (m != 0u) base = max(vertex_offsets[(x * g.Ny + y) * g.Nz + z], 0);
        s_mask[l] = (unsigned char)m;
        s_base[l] = base;
        if (m == 0u || lx == kTX || ly == kTY || lz == kTZ) continue;
        const float a = s_val[(lx * SY + ly) * SZ + lz];
        int64_t at = base;
#pragma unroll
        for (int t = 0; t < 7; ++t) {                   // ascending edge id
            if (!(m >> t & 1u)) continue;
            const int c = code_of(t), dx = c & 1, dy = c >> 1 & 1, dz = c >> 2;
            const float b = s_val[((lx + dx) * SY + ly + dy) * SZ + lz + dz];
            const float s = (level - a) / (b - a);      // a and b lie on different sides: b - a != 0
            if (at < V) {
                vertices[at * 3 + 0] = f.ox + f.sx * ((float)x + s * (float)dx);
                vertices[at * 3 + 1] = f.oy + f.sy * ((float)y + s * (float)dy);
                vertices[at * 3 + 2] = f.oz + f.sz * ((float)z + s * (float)dz);
            }
            ++at;
        }
    }
    __syncthreads();

    for (int l = threadIdx.x; l < kTileNodes; l += kThreads) {
        const int lz = l % kTZ, ly = (l / kTZ) % kTY, lx = l / (kTZ * kTY);
        const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
        if (x + 1 >= g.Nx || y + 1 >= g.Ny || z + 1 >= g.Nz) continue;
        const unsigned bits = corner_bits<2>(s_val, lx, ly, lz, level);
        if (bits == 0u || bits == 255u) continue;
        int64_t at = max(triangle_offsets[(x * (g.Ny - 1) + y) * (g.Nz - 1) + z], (int64_t)0);
        for (int k = 0; k < 6; ++k) {
            const unsigned c = tet_case(bits, k);
            const int n = kTab.ntri[c];
            const bool even = k == 0 || k == 3 || k == 4;
            for (int t = 0; t < n; ++t) {
                int32_t id[3];
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const unsigned code = kTab.tri[c][t][e];
                    const unsigned lo = kTab.tet[k][code >> 2], hi = kTab.tet[k][code & 3u];
                    const int q = ((lx + (int)(lo & 1u)) * MY + ly + (int)(lo >> 1 & 1u)) * MZ + lz + (int)(lo >> 2);
                    const unsigned type = kTab.type[hi - lo];   // the corners of a Kuhn simplex form a chain: lo is a subset of hi
                    id[e] = s_base[q] + __popc((unsigned)s_mask[q] & ((1u << type) - 1u));
                }
                if (at < T) {
                    faces[at * 3 + 0] = id[0];
                    faces[at * 3 + 1] = even ? id[1] : id[2];
                    faces[at * 3 + 2] = even ? id[2] : id[1];
                }
                ++at;
            }
        }
    }
}

int check_grid(const char* who, int Nx, int Ny, int Nz) {
    H3D_REQUIRE(Nx >= 2 && Ny >= 2 && Nz >= 2, "%s: every axis needs at least 2 nodes (Nx=%d Ny=%d Nz=%d)", who, Nx, Ny, Nz);
    H3D_REQUIRE(7 * (int64_t)Nx * Ny * Nz < ((int64_t)1 << 31), "%s: edge id range 7*Nx*Ny*Nz = %lld does not fit int32", who,
                7 * (long long)Nx * Ny * Nz);
    return H3D_OK;
}

dim3 tiles(int Nx, int Ny, int Nz) { return dim3((Nz + kTZ - 1) / kTZ, (Ny + kTY - 1) / kTY, (Nx + kTX - 1) / kTX); }

}  // namespace

extern "C" int h3d_isosurface_count(const float* volume, int Nx, int Ny, int Nz, float level, int32_t* vertex_counts,
                                    int32_t* triangle_counts, h3d_stream_t stream) {
    H3D_REQUIRE(volume && vertex_counts && triangle_counts, "h3d_isosurface_count: null pointer");
    if (int rc = check_grid("h3d_isosurface_count", Nx, Ny, Nz)) return rc;
    const dim3 grid = tiles(Nx, Ny, Nz);
    H3D_REQUIRE(grid.y <= 65535u && grid.z <= 65535u, "h3d_isosurface_count: too many tiles along x or y (Nx=%d Ny=%d)", Nx, Ny);
    h3d::pre_launch();
    hipLaunchKernelGGL(isosurface_count_kernel, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), volume, Grid{Nx, Ny, Nz},
                       level, vertex_counts, triangle_counts);
    return h3d::launch_status("h3d_isosurface_count");
}

extern "C" int h3d_isosurface_emit(const float* volume, int Nx, int Ny, int Nz, float level, const float* origin,
                                   const float* spacing, const int32_t* vertex_offsets, const int64_t* triangle_offsets,
                                   float* vertices, int64_t V, int32_t* faces, int64_t T, h3d_stream_t stream) {
    H3D_REQUIRE(volume && origin && spacing && vertex_offsets && triangle_offsets && vertices && faces,
                "h3d_isosurface_emit: null pointer");
    if (int rc = check_grid("h3d_isosurface_emit", Nx, Ny, Nz)) return rc;
    H3D_REQUIRE(V >= 1 && V <= 7 * (int64_t)Nx * Ny * Nz, "h3d_isosurface_emit: V=%lld outside [1, 7*Nx*Ny*Nz]", (long long)V);
    H3D_REQUIRE(T >= 1 && T <= 12 * (int64_t)(Nx - 1) * (Ny - 1) * (Nz - 1), "h3d_isosurface_emit: T=%lld outside [1, 12*cells]",
                (long long)T);
    const dim3 grid = tiles(Nx, Ny, Nz);
    H3D_REQUIRE(grid.y <= 65535u && grid.z <= 65535u, "h3d_isosurface_emit: too many tiles along x or y (Nx=%d Ny=%d)", Nx, Ny);
    h3d::pre_launch();
    hipLaunchKernelGGL(isosurface_emit_kernel, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), volume, Grid{Nx, Ny, Nz},
                       level, Frame{origin[0], origin[1], origin[2], spacing[0], spacing[1], spacing[2]}, vertex_offsets,
                       triangle_offsets, vertices, V, faces, T);
    return h3d::launch_status("h3d_isosurface_emit");
}
