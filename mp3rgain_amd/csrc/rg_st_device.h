// rg_st_device.h -- internal, HIP only: the device helpers the stereo image scan (rg_stereo.hip) and the null test
// (rg_compare.hip) both use, one copy: a sample out of a 16-byte vector, the funnel shift that brings the second plane's pair of
// vectors into place, q of a sample of a plane whose format is not known at compile time, and sixteen 16-bit values from LDS as
// doubles.
#pragma once

#include "rg_stereo.h"

// sample j of a vector as the stored pattern, S16 sign-extended (j is a compile-time constant after unrolling)
template <int FMT>
__device__ __forceinline__ uint32_t st_sample(const uint4 &w, uint32_t j) {
    if (FMT == RG_FMT_S16_PLANAR) {
        const uint32_t d = (j >> 1) == 0 ? w.x : (j >> 1) == 1 ? w.y : (j >> 1) == 2 ? w.z : w.w;
        return (uint32_t)(int32_t)(int16_t)(d >> (16u * (j & 1u)));
    }
    return j == 0 ? w.x : j == 1 ? w.y : j == 2 ? w.z : w.w;
}
// the 16 bytes that begin `ws` dwords and `bits` bits (0 or 16) into the 32 bytes of a | b; ws and bits are workgroup-uniform
__device__ __forceinline__ uint4 st_shift(const uint4 &a, const uint4 &b, uint32_t ws, uint32_t bits) {
    const uint32_t x0 = ws == 0 ? a.x : ws == 1 ? a.y : ws == 2 ? a.z : a.w;
    const uint32_t x1 = ws == 0 ? a.y : ws == 1 ? a.z : ws == 2 ? a.w : b.x;
    const uint32_t x2 = ws == 0 ? a.z : ws == 1 ? a.w : ws == 2 ? b.x : b.y;
    const uint32_t x3 = ws == 0 ? a.w : ws == 1 ? b.x : ws == 2 ? b.y : b.z;
    if (!bits) return uint4{x0, x1, x2, x3};
    const uint32_t x4 = ws == 0 ? b.x : ws == 1 ? b.y : ws == 2 ? b.z : b.w;
    return uint4{(x0 >> 16) | (x1 << 16), (x1 >> 16) | (x2 << 16), (x2 >> 16) | (x3 << 16), (x3 >> 16) | (x4 << 16)};
}

// q of sample k of a plane
__device__ __forceinline__ int16_t st_q_at(const unsigned char *plane, uint32_t format, uint64_t k) {
    bool finite;
    if (format == RG_FMT_S16_PLANAR) return reinterpret_cast<const int16_t *>(plane)[k];
    const uint32_t raw = reinterpret_cast<const uint32_t *>(plane)[k];
    return (int16_t)(format == RG_FMT_F32_PLANAR ? rg_st_q<RG_FMT_F32_PLANAR>(raw, &finite) : rg_st_q<RG_FMT_S32_PLANAR>(raw, &finite));
}
// 16 consecutive 16-bit values from LDS (32-byte aligned) as doubles
__device__ __forceinline__ void st_load16(const int16_t *src, double *dst) {
    const uint4 a = reinterpret_cast<const uint4 *>(src)[0], b = reinterpret_cast<const uint4 *>(src)[1];
    const uint32_t d[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
        dst[2 * i] = (double)(int32_t)(int16_t)d[i];
        dst[2 * i + 1] = (double)((int32_t)d[i] >> 16);
    }
}
