// gs_fixed128.hpp -- the 128-bit fixed-point arithmetic of the order-independent sums: device functions, no kernels, so
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

// ------------------------------------------------------------------ one term of a fold (the max pass, then the accumulate pass)
// the largest finite |x| so far, as float bits
__device__ __forceinline__ uint32_t fold_max(uint32_t mx, float x) {
    const uint32_t u = __float_as_uint(x) & 0x7fffffffu;
    return (u < 0x7f800000u && u > mx) ? u : mx;
}
// x joins the sum held in the two 64-bit words at a; a non-finite x sets one of 3 bits (NaN, +inf, -inf) at `shift` of *flags
__device__ __forceinline__ void fold_add_at(uint32_t *flags, int shift, unsigned long long *a, float x, int E) {
    const uint32_t bits = __float_as_uint(x);
    if ((bits & 0x7fffffffu) >= 0x7f800000u) {
        const uint32_t code = (bits & 0x7fffffu) ? 1u : ((bits >> 31) ? 4u : 2u);
        atomicOr(flags, code << shift);
        return;
    }
    const __int128 v = det_to_fixed(bits, E);
    if (v == 0) return;
    const unsigned long long lo = (unsigned long long)v;
    unsigned long long hi = (unsigned long long)(v >> 64);
    const unsigned long long old = atomicAdd(a, lo);
    hi += (old + lo < old) ? 1ull : 0ull;  // the carry out of the low word, counted once by the adder that caused it
    if (hi) atomicAdd(a + 1, hi);
}
// what the flags of a sum make of it: true -> r is the NaN or infinity a float sum would give
__device__ __forceinline__ bool fold_flagged(uint32_t f, float &r) {
    if (!f) return false;
    r = ((f & 1u) || (f & 6u) == 6u) ? __int_as_float(0x7fc00000) : __int_as_float((f & 2u) ? 0x7f800000 : (int)0xff800000);
    return true;
}

}  // namespace gs
