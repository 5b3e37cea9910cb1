// Small device functions that several kernels of libh3d use with the same arithmetic (gfx950 only).
#pragma once
#include "common.hpp"

namespace h3d {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ float linspace_pm1(int n, int i) {   // torch.linspace(-1, 1, n)[i]
    if (n == 1) return -1.f;
    const float step = 2.f / (float)(n - 1);
    return (i < n / 2) ? -1.f + step * (float)i : 1.f - step * (float)(n - 1 - i);
}

// the oracle's squared distance, (dx*dx + dy*dy) + dz*dz without contraction: the nearest-vertex indices are bit-exact against it
__device__ __forceinline__ float sqdist_exact(float px, float py, float pz, float vx, float vy, float vz) {
    const float dx = __fsub_rn(px, vx), dy = __fsub_rn(py, vy), dz = __fsub_rn(pz, vz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// two fp32 (already scaled) -> packed f16 hi halves (returned) and packed f16 lo halves (residuals)
__device__ __forceinline__ unsigned split2_f16(float a, float b, unsigned& lo) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    const f16x2 h2 = __builtin_convertvector(f32x2{a, b}, f16x2);
    const float fa = (float)h2.x, fb = (float)h2.y;
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a - fa, b - fb}, f16x2));
    return __builtin_bit_cast(unsigned, h2);
}

}  // namespace h3d
