// gs_fixed128.hpp -- the 128-bit fixed-point arithmetic of the order-independent sums: three device functions, no kernels, so
// that every translation unit that folds a scattered sum (gs_detfold.hpp in icp.hip, voxel.hip) states it once.
//
// With M = the largest finite |x| of a fold (float bits mbits, biased exponent eb) and at most 2^lg terms per sum,
// E = det_scale(mbits, lg) = 252 - eb - lg keeps every sum of x 2^E below 2^126.  det_to_fixed is exact for every bit of
// weight >= 2^-E (bits below are truncated toward zero: at least 102 - lg binary places below M); det_to_float rounds the
// 128-bit sum once to fp32 (nearest, ties to even) and scales it by 2^-E.
#pragma once
#include "gs_common.hpp"

namespace gs {

__device__ __forceinline__ int det_scale(uint32_t mbits, int lg) {
    const int eb = max((int)(mbits >> 23), 1);
    return 252 - eb - lg;
}

__device__ __forceinline__ __int128 det_to_fixed(uint32_t bits, int E) {
    const uint32_t e = (bits >> 23) & 0xffu, m = bits & 0x7fffffu;
    const uint32_t mant = e ? (m | 0x800000u) : m;
    const int s = (e ? (int)e : 1) - 150 + E;  // x = mant 2^(s - E)
    unsigned __int128 u = 0;
    if (s >= 0) u = (unsigned __int128)mant << s;  // s <= 102 - lg
    else if (s > -24) u = mant >> (-s);
    return (bits >> 31) ? -(__int128)u : (__int128)u;
}

__device__ __forceinline__ float det_to_float(unsigned long long lo, unsigned long long hi, int E) {
    const __int128 v = (__int128)(((unsigned __int128)hi << 64) | lo);
    const bool neg = v < 0;
    const unsigned __int128 m = neg ? (unsigned __int128)(-v) : (unsigned __int128)v;
    if (m == 0) return 0.0f;
    const unsigned long long mh = (unsigned long long)(m >> 64), ml = (unsigned long long)m;
    const int p = mh ? 127 - __clzll((long long)mh) : 63 - __clzll((long long)ml);  // leading bit
    uint32_t mant;
    int sh = 0;
    if (p <= 23) {
        mant = (uint32_t)ml;
    } else {
        sh = p - 23;
        mant = (uint32_t)(m >> sh);
        const unsigned __int128 one = 1, rem = m & ((one << sh) - 1), half = one << (sh - 1);
        if (rem > half || (rem == half && (mant & 1u))) ++mant;  // 2^24 after the carry: still exact in fp32
    }
    const float r = ldexpf((float)mant, sh - E);
    return neg ? -r : r;
}

}  // namespace gs
