// Weight packing of the split-operand field engines: the arithmetic every packer shares, defined once.
//
// field_x3.hip (register engines, host packer and field_pack_kernel) and field_x3t.hip (LDS-resident engines, host packer)
// turn the same fp32 parameters into f16 hi / lo fragments and fp6 records; what differs between them is only WHERE the
// bytes go, and that part stays with each engine.  Everything here is plain C++ and __host__ __device__: every operation is
// exact or an IEEE-rounded division, so a host packer and a device packer built on it produce the same blob bit for bit
// (tests/test_gpu_field_pack_device.py).
#pragma once
#include "x3_common.hpp"      // kX2Rho
#include <math.h>
#include <string.h>

namespace h3d {

__host__ __device__ inline uint16_t f32_to_f16_rn(float f) {            // round-to-nearest-even, handles subnormals; inputs are finite
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x47800000u) return (uint16_t)(sign | 0x7bffu);          // clamp to max finite (never hit: scaled)
    if (x < 0x38800000u) {                                             // subnormal / zero in f16
        if (x < 0x33000000u) return (uint16_t)sign;
        const uint32_t mant = (x & 0x7fffffu) | 0x800000u;
        const int shift = 126 - (int)(x >> 23);                       // 14..24
        uint32_t r = mant >> shift;
        const uint32_t rem = mant & ((1u << shift) - 1), half = 1u << (shift - 1);
        if (rem > half || (rem == half && (r & 1))) ++r;
        return (uint16_t)(sign | r);
    }
    uint32_t r = ((x - 0x38000000u) >> 13);
    const uint32_t rem = x & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (r & 1))) ++r;
    return (uint16_t)(sign | r);
}

__host__ __device__ inline float f16_to_f32(uint16_t v) {
    const uint32_t sign = (uint32_t)(v & 0x8000u) << 16;
    uint32_t e = (v >> 10) & 0x1f, m = v & 0x3ffu, x;
    if (e == 0) {
        if (m == 0) x = sign;
        else {
            int s = 0;
            while (!(m & 0x400u)) { m <<= 1; ++s; }
            x = sign | ((uint32_t)(113 - s) << 23) | ((m & 0x3ffu) << 13);
        }
    } else x = sign | ((e + 112) << 23) | (m << 13);
    float f;
    memcpy(&f, &x, 4);
    return f;
}

// the split of a (scaled) weight: v = hi + lo + O(2^-22 |v|) with both halves f16 bit patterns
__host__ __device__ inline void split_f16(float v, uint16_t& hi, uint16_t& lo) {
    hi = f32_to_f16_rn(v);
    lo = f32_to_f16_rn(v - f16_to_f32(hi));
}

// floor(log2(q)) of a positive finite q, from the exponent field (exact; log2f may round up to the next integer just below a
// power of two, and host and device must agree bit for bit: h3d_field_pack_*_device)
__host__ __device__ inline int floor_log2(float q) {
    uint32_t x;
    memcpy(&x, &q, 4);
    const int e = (int)((x >> 23) & 0xffu);
    if (e) return e - 127;
    int s = 0;                                   // subnormal
    for (uint32_t m = x & 0x7fffffu; m && !(m & 0x400000u); m <<= 1) ++s;
    return -127 - s;
}
// the largest power of two 2^e with mx * 2^e <= target (1 for an all-zero matrix)
__host__ __device__ inline float pow2_scale_of(float mx, float target) { return mx > 0.f ? ldexpf(1.f, floor_log2(target / mx)) : 1.f; }

// input feature of k-slot (half hh, element e) of k-step ks when the consumer's B fragments are accumulator registers
// (field_x3.hip: FilmProducer, x3t_common.hpp: "K order"): tile ks/2, accumulator register r = 8*(ks & 1) + e
//  ->  row (r & 3) + 8*(r >> 2) + 4*hh
__host__ __device__ inline int acc_k(int ks, int hh, int e) { return 32 * (ks / 2) + (e & 3) + 8 * (2 * (ks & 1) + (e >> 2)) + 4 * hh; }

// The slice of a row-major matrix that one packed matrix is made of: rows [0, n_out), columns [in_begin, in_begin + in_count)
// of W (rows `ld` floats apart); zero outside (the padding of the 32-row tiles and 16-column k-steps).
struct WeightSlice {
    const float* w;
    int ld, in_begin, in_count, n_out;
    __host__ __device__ float at(int nn, int k, float scale) const {
        return k < in_count && nn < n_out ? w[(int64_t)nn * ld + in_begin + k] * scale : 0.f;
    }
};
// column of k-slot (hh, e) of k-step ks: accumulator order (the input is a previous layer's accumulators) or the natural
// order (inputs assembled from memory: coordinates, geometry features, view direction)
__host__ __device__ inline int slot_k(bool acc_order, int ks, int hh, int e) { return acc_order ? acc_k(ks, hh, e) : 16 * ks + 8 * hh + e; }

// ---- x2 packing: fp6 (e2m3) codes and block scales
__host__ __device__ inline unsigned e2m3_code(float v) {            // round-to-nearest-even on the code grid, saturating at 7.5
    const unsigned sign = v < 0.f ? 32u : 0u;
    const float a = fminf(fabsf(v), 7.5f);
    const float step = a < 2.f ? 0.125f : a < 4.f ? 0.25f : 0.5f;
    const float q = nearbyintf(a / step) * step;         // default rounding mode: ties to even; spacing doubles exactly at 2 and 4
    unsigned c;
    if (q < 2.f) c = (unsigned)(q * 8.f);                // 0 .. 15: subnormals 0..7 and [1, 2)
    else if (q < 4.f) c = 16u + (unsigned)((q - 2.f) * 4.f);
    else c = 24u + (unsigned)((q - 4.f) * 2.f);
    return sign | c;
}

// 32 B fp6 record of one lane and K-tile from its 16 (already scaled) weights' f16 hi values and fp32 residuals: the 32 six-bit
// codes of hi * alpha (slots 0-15, dwords 0-2) and lo * 2^12 * alpha (slots 16-31, dwords 3-5), the block-scale byte in every
// byte of dwords 6 and 7
__host__ __device__ inline void x2_make_record(const float (&hi)[16], const float (&lo)[16], unsigned (&rec)[8]) {
    float mx = 0.f;
    for (int i = 0; i < 16; ++i) mx = fmaxf(mx, fabsf(hi[i]));
    // block scale alpha = 2^ea: the largest with |hi| * alpha <= 7.5 unless a lo code would saturate (then half of
    // it); the instruction multiplies the codes by 2^(byte - 127) = 1 / alpha
    int ea = mx > 0.f ? floor_log2(7.5f / mx) : 0;
    if (ea > 100) ea = 100;
    if (ea < -100) ea = -100;
    // (f16-subnormal hi values leave lo up to 2^-1 of hi instead of 2^-11: several steps then)
    for (bool sat = true; sat && ea > -100;) {
        sat = false;
        for (int i = 0; i < 16; ++i) sat = sat || fabsf(lo[i]) * kX2Rho * ldexpf(1.f, ea) > 7.5f;
        if (sat) --ea;
    }
    const float alpha = ldexpf(1.f, ea);
    for (int d = 0; d < 8; ++d) rec[d] = 0;
    for (int sl = 0; sl < 32; ++sl) {
        const float v = sl < 16 ? hi[sl] * alpha : lo[sl - 16] * alpha * kX2Rho;
        const uint64_t code = e2m3_code(v);
        const int bit = 6 * sl;
        rec[bit / 32] |= (unsigned)(code << (bit & 31));
        if ((bit & 31) > 26) rec[bit / 32 + 1] |= (unsigned)(code >> (32 - (bit & 31)));
    }
    rec[6] = rec[7] = (unsigned)(127 - ea) * 0x01010101u;
}

// One lane, one K-tile of an accumulator-order matrix in the x2 arithmetic: the 16 weights of (row nn, lane half hh, k-steps
// 2T and 2T + 1) -> their f16 hi bit patterns (h16[8 j + e]: element e of k-step 2T + j) and the fp6 record of the tile
__host__ __device__ inline void x2_lane_tile(const WeightSlice& m, float scale, int nn, int hh, int T, uint16_t (&h16)[16], unsigned (&rec)[8]) {
    float hi[16], lo[16];
    for (int j = 0; j < 2; ++j)
        for (int e = 0; e < 8; ++e) {
            const float v = m.at(nn, acc_k(2 * T + j, hh, e), scale);
            h16[8 * j + e] = f32_to_f16_rn(v);
            hi[8 * j + e] = f16_to_f32(h16[8 * j + e]);
            lo[8 * j + e] = v - hi[8 * j + e];
        }
    x2_make_record(hi, lo, rec);
}

}  // namespace h3d
