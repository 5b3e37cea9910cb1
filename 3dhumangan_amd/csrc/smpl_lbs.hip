// SMPL forward (linear blend skinning) for a batch of bodies == lbs() of the reference (lib/components/smpl.py:11-107) with the
// four smplx helpers it calls (blend_shapes, vertices2joints, batch_rodrigues, batch_rigid_transform), fp32 throughout.
//
// Three launches (smpl_shape and smpl_pose are independent of each other; smpl_skin reads both):
//   smpl_shape  v_shaped = v_template + shapedirs . betas; one thread per coordinate, a tile of kItems items per thread, so that
//               shapedirs is read once per tile.
//   smpl_pose   one wave per item: joints from the folded regressor (J_regressor . v_template and J_regressor . shapedirs, folded on
//               the host once per model -- the joints are linear in betas), Rodrigues with one joint per lane, the parents chain
//               sequentially over joints with the 12 free entries of each 4 x 4 product on 12 lanes, then A, the posed joints and
//               the pose feature (R[1:] - I, row-major over joints 1..J-1).
//   smpl_skin   64 vertices x kItems items per workgroup of 4 waves.  The tile's A and pose features sit in LDS.  Pose offsets: wave
//               s walks the s-th quarter of the (J-1)*9 rows of posedirs for all kItems items at once (posedirs, the only large operand,
//               is read once per tile of kItems items); the four partial sums meet in LDS and are added in slice order.  Skinning: wave s
//               blends and applies the transforms of items s and s + 4 of the tile.
// No atomics; every sum runs in a fixed order that depends on the model's shapes alone, so two runs agree bit for bit and an item's
// result does not depend on the batch around it.  Plain C++, vector stores only.
#include "common.hpp"

namespace {

constexpr int kItems = 8;        // items per tile (smpl_shape, smpl_skin)
constexpr int kSlices = 4;       // waves of a smpl_skin workgroup == slices of the pose-feature rows
constexpr int kMaxJ = 64;
static_assert(kItems == 2 * kSlices, "smpl_skin: each wave skins two items of the tile");

__global__ __launch_bounds__(256) void smpl_shape_kernel(const float* __restrict__ betas, const float* __restrict__ v_template,
                                                         const float* __restrict__ shapedirs, float* __restrict__ v_shaped,
                                                         int B, int64_t V3, int NB) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int b0 = blockIdx.y * kItems;
    if (e >= V3) return;
    float acc[kItems];
#pragma unroll
    for (int t = 0; t < kItems; ++t) acc[t] = 0.f;
    const float* sd = shapedirs + e * NB;
    for (int l = 0; l < NB; ++l) {
        const float s = sd[l];
#pragma unroll
        for (int t = 0; t < kItems; ++t) {
            const int b = min(b0 + t, B - 1);                        // wave-uniform address: a scalar load
            acc[t] = fmaf(betas[(int64_t)b * NB + l], s, acc[t]);
        }
    }
    const float vt = v_template[e];
#pragma unroll
    for (int t = 0; t < kItems; ++t)
        if (b0 + t < B) v_shaped[(int64_t)(b0 + t) * V3 + e] = vt + acc[t];
}

__global__ __launch_bounds__(64) void smpl_pose_kernel(const float* __restrict__ betas, const float* __restrict__ pose,
                                                       const float* __restrict__ joint_template, const float* __restrict__ joint_dirs,
                                                       const int32_t* __restrict__ parents, float* __restrict__ A,
                                                       float* __restrict__ joints, float* __restrict__ joints_posed,
                                                       float* __restrict__ pose_feature, int J, int NB, int pose2rot) {
    __shared__ float Js[kMaxJ][3];
    __shared__ float Rs[kMaxJ][9];
    __shared__ float Gs[kMaxJ][12];        // rows 0..2 of G_i (row 3 is 0 0 0 1)
    __shared__ int Ps[kMaxJ];
    const int64_t b = blockIdx.x;
    const int j = threadIdx.x;
    if (j < J) {
        float jx = 0.f, jy = 0.f, jz = 0.f;
        const float* jd = joint_dirs + (int64_t)j * 3 * NB;
        const float* be = betas + b * NB;
        for (int l = 0; l < NB; ++l) {
            const float w = be[l];
            jx = fmaf(w, jd[l], jx);
            jy = fmaf(w, jd[NB + l], jy);
            jz = fmaf(w, jd[2 * NB + l], jz);
        }
        jx += joint_template[j * 3 + 0];
        jy += joint_template[j * 3 + 1];
        jz += joint_template[j * 3 + 2];
        Js[j][0] = jx, Js[j][1] = jy, Js[j][2] = jz;
        float* jo = joints + (b * J + j) * 3;
        jo[0] = jx, jo[1] = jy, jo[2] = jz;

        float R[9];
        if (pose2rot) {
            // smplx batch_rodrigues: the epsilon goes onto every component before the norm; the direction divides the raw vector
            const float* aa = pose + (b * J + j) * 3;
            const float x = aa[0], y = aa[1], z = aa[2];
            const float ex = x + 1e-8f, ey = y + 1e-8f, ez = z + 1e-8f;
            const float angle = sqrtf(ex * ex + ey * ey + ez * ez);
            const float dx = x / angle, dy = y / angle, dz = z / angle;
            const float s = sinf(angle), c1 = 1.f - cosf(angle);
            // K = [[0,-dz,dy],[dz,0,-dx],[-dy,dx,0]];  R = I + s K + (1 - c) K K
            R[0] = 1.f + c1 * (-(dz * dz) - dy * dy);
            R[1] = s * -dz + c1 * (dy * dx);
            R[2] = s * dy + c1 * (dz * dx);
            R[3] = s * dz + c1 * (dx * dy);
            R[4] = 1.f + c1 * (-(dz * dz) - dx * dx);
            R[5] = s * -dx + c1 * (dz * dy);
            R[6] = s * -dy + c1 * (dx * dz);
            R[7] = s * dx + c1 * (dy * dz);
            R[8] = 1.f + c1 * (-(dy * dy) - dx * dx);
        } else {
            const float* rm = pose + (b * J + j) * 9;
#pragma unroll
            for (int i = 0; i < 9; ++i) R[i] = rm[i];
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) Rs[j][i] = R[i];
        if (j >= 1) {
            float* pf = pose_feature + b * (int64_t)(J - 1) * 9 + (j - 1) * 9;
#pragma unroll
            for (int i = 0; i < 9; ++i) pf[i] = R[i] - ((i & 3) == 0 ? 1.f : 0.f);       // the diagonal sits at 0, 4, 8
        }
        Ps[j] = parents[j];
    }
    __syncthreads();

    // G_0 = [R_0 | J_0];  G_i = G_parent(i) . [R_i | J_i - J_parent(i)]: lane 4 r + c owns entry (r, c)
    const int r = (j >> 2) % 3, c = j & 3;
    for (int i = 0; i < J; ++i) {
        if (j < 12) {
            float g;
            if (i == 0) {
                g = c < 3 ? Rs[0][r * 3 + c] : Js[0][r];
            } else {
                const int p = min(max(Ps[i], 0), i - 1);             // validated on the host; clamped so that no read leaves Gs
                float l0, l1, l2;
                if (c < 3) {
                    l0 = Rs[i][c], l1 = Rs[i][3 + c], l2 = Rs[i][6 + c];
                } else {
                    l0 = Js[i][0] - Js[p][0], l1 = Js[i][1] - Js[p][1], l2 = Js[i][2] - Js[p][2];
                }
                g = Gs[p][r * 4 + 0] * l0 + Gs[p][r * 4 + 1] * l1 + Gs[p][r * 4 + 2] * l2;
                if (c == 3) g += Gs[p][r * 4 + 3];
            }
            Gs[i][j] = g;
        }
        __syncthreads();
    }

    if (j < J) {
        float G[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) G[i] = Gs[j][i];
        const float jx = Js[j][0], jy = Js[j][1], jz = Js[j][2];
        float* jp = joints_posed + (b * J + j) * 3;
        jp[0] = G[3], jp[1] = G[7], jp[2] = G[11];
        float4* a = reinterpret_cast<float4*>(A + (b * J + j) * 16);
#pragma unroll
        for (int q = 0; q < 3; ++q)
            a[q] = make_float4(G[q * 4], G[q * 4 + 1], G[q * 4 + 2],
                               G[q * 4 + 3] - (G[q * 4] * jx + G[q * 4 + 1] * jy + G[q * 4 + 2] * jz));
        a[3] = make_float4(0.f, 0.f, 0.f, 1.f);
    }
}

// Dynamic LDS: As [kItems][J][12] | Fs [P][kItems] | Rd [kSlices][kItems][3][64] (the last two only with pose offsets, P > 0).
__global__ __launch_bounds__(256) void smpl_skin_kernel(const float* __restrict__ v_in, const float* __restrict__ pose_feature,
                                                        const float* __restrict__ posedirs, const float* __restrict__ A,
                                                        const float* __restrict__ rigid, const float* __restrict__ transl,
                                                        const float* __restrict__ weights, float* __restrict__ verts,
                                                        int B, int V, int J, int P) {
    extern __shared__ float4 smpl_lds[];
    float* As = reinterpret_cast<float*>(smpl_lds);
    float* Fs = As + kItems * J * 12;
    float* Rd = Fs + P * kItems;
    const int tid = threadIdx.x, vl = tid & 63, sl = tid >> 6;
    const int b0 = blockIdx.y * kItems;
    const int64_t v = (int64_t)blockIdx.x * 64 + vl;

    for (int e = tid; e < kItems * J * 12; e += 256) {
        const int t = e / (J * 12), rem = e - t * (J * 12), jj = rem / 12, rc = rem - jj * 12, r = rc >> 2, c = rc & 3;
        float val = 0.f;
        if (b0 + t < B) {
            const float* a = A + ((int64_t)(b0 + t) * J + jj) * 16;
            if (rigid) {                                             // rigid . A_j, rows 0..2
                const float* g = rigid + (int64_t)(b0 + t) * 16 + r * 4;
                val = g[0] * a[c] + g[1] * a[4 + c] + g[2] * a[8 + c];
                if (c == 3) val += g[3];
            } else {
                val = a[r * 4 + c];
            }
        }
        As[e] = val;
    }
    for (int e = tid; e < P * kItems; e += 256) {
        const int p = e / kItems, t = e - p * kItems;
        Fs[e] = b0 + t < B ? pose_feature[(int64_t)(b0 + t) * P + p] : 0.f;
    }
    __syncthreads();

    if (P > 0) {
        float off[kItems][3];
#pragma unroll
        for (int t = 0; t < kItems; ++t) off[t][0] = off[t][1] = off[t][2] = 0.f;
        const int pq = (P + kSlices - 1) / kSlices, p0 = sl * pq, p1 = min(P, p0 + pq);
        if (v < V) {
            const float* pd = posedirs + (int64_t)p0 * 3 * V + 3 * v;
#pragma unroll 4
            for (int p = p0; p < p1; ++p, pd += (int64_t)3 * V) {
                const float x = pd[0], y = pd[1], z = pd[2];
                const float4 f0 = *reinterpret_cast<const float4*>(Fs + p * kItems);
                const float4 f1 = *reinterpret_cast<const float4*>(Fs + p * kItems + 4);
                const float f[kItems] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
#pragma unroll
                for (int t = 0; t < kItems; ++t) {
                    off[t][0] = fmaf(f[t], x, off[t][0]);
                    off[t][1] = fmaf(f[t], y, off[t][1]);
                    off[t][2] = fmaf(f[t], z, off[t][2]);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < kItems; ++t)
#pragma unroll
            for (int k = 0; k < 3; ++k) Rd[((sl * kItems + t) * 3 + k) * 64 + vl] = off[t][k];
        __syncthreads();
    }
    if (v >= V) return;

    float T[2][12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[0][i] = T[1][i] = 0.f;
    const float* w = weights + v * J;
    for (int jj = 0; jj < J; ++jj) {
        const float wj = w[jj];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float4* a = reinterpret_cast<const float4*>(As + ((sl + h * kSlices) * J + jj) * 12);
            const float4 a0 = a[0], a1 = a[1], a2 = a[2];
            const float av[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
#pragma unroll
            for (int i = 0; i < 12; ++i) T[h][i] = fmaf(wj, av[i], T[h][i]);
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int t = sl + h * kSlices, b = b0 + t;
        if (b >= B) continue;
        const float* vi = v_in + ((int64_t)b * V + v) * 3;
        float x = vi[0], y = vi[1], z = vi[2];
        if (P > 0) {
            float o[3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
                o[k] = ((Rd[((0 * kItems + t) * 3 + k) * 64 + vl] + Rd[((1 * kItems + t) * 3 + k) * 64 + vl]) +
                        Rd[((2 * kItems + t) * 3 + k) * 64 + vl]) + Rd[((3 * kItems + t) * 3 + k) * 64 + vl];
            x += o[0], y += o[1], z += o[2];
        }
        float ox = T[h][0] * x + T[h][1] * y + T[h][2] * z + T[h][3];
        float oy = T[h][4] * x + T[h][5] * y + T[h][6] * z + T[h][7];
        float oz = T[h][8] * x + T[h][9] * y + T[h][10] * z + T[h][11];
        if (transl) ox += transl[b * 3 + 0], oy += transl[b * 3 + 1], oz += transl[b * 3 + 2];
        float* vo = verts + ((int64_t)b * V + v) * 3;
        vo[0] = ox, vo[1] = oy, vo[2] = oz;
    }
}

inline int64_t skin_lds_bytes(int J, int P) {
    return 4 * ((int64_t)kItems * J * 12 + (P > 0 ? (int64_t)P * kItems + kSlices * kItems * 3 * 64 : 0));
}

}  // namespace

extern "C" int h3d_smpl_shape(const float* betas, const float* v_template, const float* shapedirs, float* v_shaped, int B, int V,
                              int NB, h3d_stream_t stream) {
    H3D_REQUIRE(v_template && v_shaped && (NB == 0 || (betas && shapedirs)), "h3d_smpl_shape: null pointer");
    H3D_REQUIRE(B >= 1 && V >= 1 && NB >= 0, "h3d_smpl_shape: bad shape (B=%d V=%d NB=%d)", B, V, NB);
    H3D_REQUIRE((B + kItems - 1) / kItems <= 65535, "h3d_smpl_shape: B=%d exceeds %d items per call", B, 65535 * kItems);
    const int64_t V3 = (int64_t)V * 3;
    H3D_REQUIRE((V3 + 255) / 256 < (int64_t(1) << 31), "h3d_smpl_shape: V=%d too large", V);
    h3d::pre_launch();
    hipLaunchKernelGGL(smpl_shape_kernel, dim3((unsigned)((V3 + 255) / 256), (B + kItems - 1) / kItems), dim3(256), 0,
                       static_cast<hipStream_t>(stream), betas, v_template, shapedirs, v_shaped, B, V3, NB);
    return h3d::launch_status("h3d_smpl_shape");
}

extern "C" int h3d_smpl_pose(const float* betas, const float* pose, const float* joint_template, const float* joint_dirs,
                             const int32_t* parents, float* A, float* joints, float* joints_posed, float* pose_feature, int B,
                             int J, int NB, int pose2rot, h3d_stream_t stream) {
    H3D_REQUIRE(pose && joint_template && parents && A && joints && joints_posed && (NB == 0 || (betas && joint_dirs)) &&
                (J == 1 || pose_feature), "h3d_smpl_pose: null pointer");
    H3D_REQUIRE(B >= 1 && J >= 1 && J <= kMaxJ && NB >= 0, "h3d_smpl_pose: bad shape (B=%d, 1 <= J=%d <= %d, NB=%d)", B, J, kMaxJ, NB);
    H3D_REQUIRE(pose2rot == 0 || pose2rot == 1, "h3d_smpl_pose: pose2rot is 0 or 1");
    H3D_REQUIRE(h3d::aligned16(A), "h3d_smpl_pose: A must be 16-byte aligned");
    h3d::pre_launch();
    hipLaunchKernelGGL(smpl_pose_kernel, dim3(B), dim3(64), 0, static_cast<hipStream_t>(stream), betas, pose, joint_template,
                       joint_dirs, parents, A, joints, joints_posed, pose_feature, J, NB, pose2rot);
    return h3d::launch_status("h3d_smpl_pose");
}

extern "C" int h3d_smpl_skin(const float* v_in, const float* pose_feature, const float* posedirs, const float* A, const float* rigid,
                             const float* transl, const float* lbs_weights, float* verts, int B, int V, int J, h3d_stream_t stream) {
    H3D_REQUIRE(v_in && A && lbs_weights && verts, "h3d_smpl_skin: null pointer");
    H3D_REQUIRE((posedirs == nullptr) == (pose_feature == nullptr), "h3d_smpl_skin: posedirs and pose_feature go together");
    H3D_REQUIRE(B >= 1 && V >= 1 && J >= 1 && J <= kMaxJ, "h3d_smpl_skin: bad shape (B=%d V=%d, 1 <= J=%d <= %d)", B, V, J, kMaxJ);
    H3D_REQUIRE((B + kItems - 1) / kItems <= 65535, "h3d_smpl_skin: B=%d exceeds %d items per call", B, 65535 * kItems);
    const int P = posedirs && J > 1 ? (J - 1) * 9 : 0;
    const int64_t lds = skin_lds_bytes(J, P);
    H3D_REQUIRE(lds <= 160 * 1024, "h3d_smpl_skin: %lld bytes of LDS", (long long)lds);
    if (lds > 64 * 1024) H3D_ALLOW_MAX_LDS(smpl_skin_kernel);
    h3d::pre_launch();
    hipLaunchKernelGGL(smpl_skin_kernel, dim3((unsigned)(((int64_t)V + 63) / 64), (B + kItems - 1) / kItems), dim3(256), (size_t)lds,
                       static_cast<hipStream_t>(stream), v_in, P ? pose_feature : nullptr, P ? posedirs : nullptr, A, rigid, transl,
                       lbs_weights, verts, B, V, J, P);
    return h3d::launch_status("h3d_smpl_skin");
}
