// Volume compositing (lib/generators/volume_rendering.py:12-56, ray_integration): the one device-side definition of the
// reference's rules -- the last sample's delta = 1e9, f = (1 - alpha) + 1e-12, softplus with threshold 20 against relu,
// last_back -- and of the wave-level transmittance scan around them.  The per-sample arithmetic (composite_sample) serves all
// six kernels: the stand-alone integration and its backward (ray_integrate.hip, train_ops.hip, with the full-wave scan) and the
// fused renders (field_x3.hip, field_x3t.hip, neural_field.hip).  The compositing step on top of it serves field_x3.hip at
// width 32; field_x3t.hip and neural_field.hip keep their own 64-wide copy of it, because with the call in place of the text
// the compiler allocates their registers differently (they run at the 512-register limit, spill counts moved).
// The 1e-3 refinement band of field_x3.hip is reasoned against this arithmetic.
// Nothing here knows which kernel calls it: parameters are compile-time, stores to global memory belong to the caller.
#pragma once
#include "common.hpp"

namespace h3d {

__device__ __forceinline__ float density(float x, int clamp_mode) {
    if (clamp_mode == 1) return x > 20.f ? x : log1pf(expf(x));   // F.softplus (beta = 1, threshold = 20)
    return fmaxf(x, 0.f);
}
__device__ __forceinline__ float density_deriv(float x, int clamp_mode) {
    if (clamp_mode == 1) return x > 20.f ? 1.f : 1.f / (1.f + expf(-x));
    return x > 0.f ? 1.f : 0.f;
}

// One sample of a ray.  The defaults are those of a lane without a sample: it leaves the products and sums alone.
// Every caller reads z, alpha and f; delta, sg and e are for the backward (composite_dalpha) and sg for field_x3's refinement test.
struct Sample {
    float z = 0.f, delta = 0.f, sg = 0.f;      // depth, distance to the next sample, density input (sigma + noise)
    float e = 1.f, alpha = 0.f, f = 1.f;       // e = 1 - alpha = exp(-delta * density), f = the transmittance factor
};

// Sample i of z_vals / noise (noise may be null); `last`: the ray's last sample.  ZP / NP are pointer types, so that a caller
// can pass address-space-1 pointers.  Loads in this order: z, the next z, the noise.
// LONG_RAY: alpha from expm1f instead of 1 - expf.  In a thin medium (delta * density ~ 1e-5) the difference keeps a few bits and
// the device expf rounds with a bias there: the weights' error grows linearly with the sample count, 3.6e-9 per sample
// (tests/test_gpu_composite_edges.py, thin_lastneg) -- 7e-6 at the 2048 samples the stand-alone kernels accept, under 5e-7 at the
// sample counts of the fused renders.  The stand-alone integration and its backward take it; the fused renders keep 1 - expf, their
// outputs are recorded bit for bit (tests/test_gpu_dynamic_tiles.py, test_gpu_ray_head.py).
template <bool LONG_RAY = false, typename ZP, typename NP, typename I>
__device__ __forceinline__ Sample composite_sample(float sigma, ZP z_vals, NP noise, I i, bool last, int clamp_mode) {
    Sample s;
    s.z = z_vals[i];
    s.delta = last ? 1e9f : z_vals[i + 1] - s.z;
    s.sg = sigma + (noise ? noise[i] : 0.f);
    if constexpr (LONG_RAY) {
        s.alpha = -expm1f(-s.delta * density(s.sg, clamp_mode));
        s.e = 1.f - s.alpha;                                       // the rounded 1 - alpha: f below is the same expression
    } else {
        s.e = expf(-s.delta * density(s.sg, clamp_mode));
        s.alpha = 1.f - s.e;
    }
    s.f = (1.f - s.alpha) + 1e-12f;
    return s;
}
// d alpha / d sigma of that sample
__device__ __forceinline__ float composite_dalpha(const Sample& s, int clamp_mode) {
    return s.delta * s.e * density_deriv(s.sg, clamp_mode);
}

// Transmittance scan over segments of `seglen` consecutive lanes (a power of two <= WIDTH, WIDTH = 64 or 32); sl = the lane's
// place in its segment.  scan_inclusive: product of f up to and including the lane.  scan_exclusive: the same without the
// lane's own factor, the transmittance in front of its sample within this tile.  tile_product: what a ray that continues in
// the next tile multiplies its carried transmittance by.
template <int WIDTH>
__device__ __forceinline__ float scan_inclusive(float f, int sl, int seglen) {
    float incl = f;
    for (int off = 1; off < seglen; off <<= 1) {
        const float u = __shfl_up(incl, off, WIDTH);
        if (sl >= off) incl *= u;
    }
    return incl;
}
template <int WIDTH>
__device__ __forceinline__ float scan_exclusive(float incl, int sl) {
    float excl = __shfl_up(incl, 1, WIDTH);
    if (sl == 0) excl = 1.f;
    return excl;
}
template <int WIDTH>
__device__ __forceinline__ float tile_product(float incl) { return __shfl(incl, WIDTH - 1, WIDTH); }

// What a ray carries from tile to tile: transmittance behind the samples so far, sum of w, sum of w * z.
struct RayCarry { float T = 1.f, W = 0.f, D = 0.f; };

// One tile of WIDTH samples, `seglen` per ray (rays longer than WIDTH: seglen = WIDTH and one ray over several tiles).
// Returns the lane's compositing weight, with the last_back fix-up on the ray's last sample (`ray_end`); bg = 1 - sum(w)
// of the lane's ray on the last tile, else 0.  depth(d) is called on the ray_end lanes of the last tile.
// Today's only caller is field_x3.hip (WIDTH = 32); neural_field.hip and field_x3t.hip hold the same step as text (see the top).
// (The scan is spelled out, not a call of scan_inclusive / scan_exclusive: with the call, field_x3_kernel's scan loop comes out
// with its branch inverted; like this its instructions are the ones of the text it replaces.)
template <int WIDTH, typename Depth>
__device__ __forceinline__ float composite_step(const Sample& s, RayCarry& c, int lane, int seglen, bool last_tile, bool ray_end,
                                                int last_back, float& bg, Depth&& depth) {
    const int sl = lane & (seglen - 1);
    float incl = s.f;
    for (int off = 1; off < seglen; off <<= 1) {
        const float u = __shfl_up(incl, off, WIDTH);
        if (sl >= off) incl *= u;
    }
    float excl = __shfl_up(incl, 1, WIDTH);
    if (sl == 0) excl = 1.f;
    float w = s.alpha * (c.T * excl);
    float wsum = w, dsum = w * s.z;
    for (int off = seglen >> 1; off > 0; off >>= 1) {
        wsum += __shfl_xor(wsum, off, WIDTH);
        dsum += __shfl_xor(dsum, off, WIDTH);
    }
    const float z_last = __shfl(s.z, lane | (seglen - 1), WIDTH);
    c.T *= tile_product<WIDTH>(incl);
    c.W += wsum;
    c.D += dsum;
    bg = 0.f;
    if (last_tile) {
        bg = 1.f - c.W;
        if (ray_end) {
            depth(c.D + bg * z_last);               // both last_back variants agree on depth
            if (last_back) w += bg;
        }
    }
    return w;
}

}  // namespace h3d
