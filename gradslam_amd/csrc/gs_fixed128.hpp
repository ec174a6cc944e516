// gs_fixed128.hpp -- the exact fold: scattered sums whose fp32 results do not depend on the order of arrival.  Device and host
// functions, no kernels: every translation unit that folds (gs_detfold.hpp in icp.hip, voxel.hip, neighbors.hip, tsdf.hip) brings
// its own loops over its own terms and takes every step of the rule from here.
//
// A fold of rows x nch sums runs over its terms twice and over its sums once:
//   max pass    M = the largest finite |x| of all terms: fold_max per term, fold_max_commit per wave (integer atomicMax on the
//               float bits: exact, commutative)
//   accumulate  x -> x 2^E as a signed 128-bit fixed-point integer, added into the (lo, hi) pair of 64-bit words of its sum with
//               integer atomics; the low word's wrap is carried into the high word by the adder that caused it (fold_add).  A
//               non-finite x sets one of 3 flag bits of its sum instead: NaN, +inf, -inf
//   finish      per sum: the float sum's NaN (a NaN, or both infinities) or infinity where a flag is set, else the 128-bit
//               sum rounded once to fp32 (nearest, ties to even) and scaled by 2^-E (fold_result)
// Integer addition is associative, so the sums -- and the fp32 results -- are the same bits whatever the order of arrival.
//
// Scale: with M's float bits mbits (biased exponent eb, so |x| < 2^(eb - 126)) and at most 2^lg terms per sum (fold_lg),
// E = det_scale(mbits, lg) = 252 - eb - lg keeps every sum of x 2^E below 2^126.  det_to_fixed is exact for every bit of
// weight >= 2^-E (bits below are truncated toward zero: at least 102 - lg binary places below M); det_to_float rounds the
// 128-bit sum once to fp32 and scales it by 2^-E.  The accumulators, the flags and the maximum start from zero.
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

// ------------------------------------------------------------------ the workspace of a fold of rows x nch sums
constexpr int FOLD_FLAGS_PER_WORD = 10;  // 3 bits (NaN, +inf, -inf) per channel, ten channels per flag word

struct Fold {  // (see fold_carve for the order of the pieces)
    uint32_t *maxbits;        // 1: float bits of the largest finite |x|
    uint32_t *flags;          // rows x ceil(nch / 10) words
    unsigned long long *acc;  // rows x nch x (lo, hi)
    int nch;
};
__host__ __device__ __forceinline__ int fold_flag_words(int nch) { return (nch + FOLD_FLAGS_PER_WORD - 1) / FOLD_FLAGS_PER_WORD; }

// Pieces in the order maximum | flags | sums, or sums | flags | maximum for a caller whose accumulators have always started its
// workspace (voxel.hip, neighbors.hip).  The total is the same; where the sums sit is not free: moved behind the other two
// pieces, the most contended voxel reduction measured 2 % slower (profiles/fold_ab.txt).
static inline Fold fold_carve(Carve &c, size_t rows, int nch, bool sums_first = false) {
    Fold f;
    const size_t flag_bytes = rows * fold_flag_words(nch) * 4, sum_bytes = rows * nch * 16;
    if (sums_first) {
        f.acc = c.take<unsigned long long>(sum_bytes);
        f.flags = c.take<uint32_t>(flag_bytes);
        f.maxbits = c.take<uint32_t>(4);
    } else {
        f.maxbits = c.take<uint32_t>(4);
        f.flags = c.take<uint32_t>(flag_bytes);
        f.acc = c.take<unsigned long long>(sum_bytes);
    }
    f.nch = nch;
    return f;
}
static inline int fold_lg(int64_t n) {  // ceil(log2 n) for n terms per sum at most
    int lg = 0;
    while (((int64_t)1 << lg) < n) ++lg;
    return lg;
}

// ------------------------------------------------------------------ max pass
// the largest finite |x| so far, as float bits
__device__ __forceinline__ uint32_t fold_max(uint32_t mx, float x) {
    const uint32_t u = __float_as_uint(x) & 0x7fffffffu;
    return (u < 0x7f800000u && u > mx) ? u : mx;
}
// the wave's maximum joins the fold's: one atomic per wave, none for a wave of zeros.  Every lane of the wave calls it.
__device__ __forceinline__ void fold_max_commit(uint32_t *maxbits, uint32_t mx) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off, kWave));
    if ((threadIdx.x & 63) == 0 && mx > 0) atomicMax(maxbits, mx);
}

// the flag word of (row, ch), whose 3 bits sit at fold_flag_shift(ch)
__device__ __forceinline__ uint32_t *fold_flag_word(const Fold &f, int64_t row, int ch) {
    return f.flags + row * fold_flag_words(f.nch) + ch / FOLD_FLAGS_PER_WORD;
}
__device__ __forceinline__ int fold_flag_shift(int ch) { return 3 * (ch % FOLD_FLAGS_PER_WORD); }

// ------------------------------------------------------------------ accumulate
// false for a non-finite term, whose flag bit is set at (row, ch); true: the term is to be added
__device__ __forceinline__ bool fold_finite(const Fold &f, int64_t row, int ch, uint32_t bits) {
    if ((bits & 0x7fffffffu) < 0x7f800000u) return true;
    const uint32_t code = (bits & 0x7fffffu) ? 1u : ((bits >> 31) ? 4u : 2u);
    atomicOr(fold_flag_word(f, row, ch), code << fold_flag_shift(ch));
    return false;
}
// the 128-bit term (lo, hi) joins the sum at a; an all-zero term costs no atomic
__device__ __forceinline__ void fold_add_words(unsigned long long *a, unsigned long long lo, unsigned long long hi) {
    if ((lo | hi) == 0ull) return;
    const unsigned long long old = atomicAdd(a, lo);
    hi += (old + lo < old) ? 1ull : 0ull;  // the carry out of the low word, counted once by the adder that caused it
    if (hi) atomicAdd(a + 1, hi);
}
__device__ __forceinline__ unsigned long long *fold_sum(const Fold &f, int64_t row, int ch) { return f.acc + (row * f.nch + ch) * 2; }
__device__ __forceinline__ void fold_add(const Fold &f, int64_t row, int ch, float x, int E) {
    const uint32_t bits = __float_as_uint(x);
    if (!fold_finite(f, row, ch, bits)) return;
    const __int128 v = det_to_fixed(bits, E);
    fold_add_words(fold_sum(f, row, ch), (unsigned long long)v, (unsigned long long)(v >> 64));
}

// ------------------------------------------------------------------ finish
// The sum's words are read whether or not a flag is set.  Read only behind the flag test they are a second dependent memory
// trip per sum (a caller's finish loop cannot keep the flag word of a row in a register across its own stores, which may
// alias it), and the ray cast's reverse pass, 2 M voxels x 4 sums, measured 4 % slower; issued together the two loads cost one.
__device__ __forceinline__ float fold_result(const Fold &f, int64_t row, int ch, int E) {
    const unsigned long long *a = fold_sum(f, row, ch);
    const uint32_t fl = (*fold_flag_word(f, row, ch) >> fold_flag_shift(ch)) & 7u;
    const float r = det_to_float(a[0], a[1], E);
    if (!fl) return r;
    return ((fl & 1u) || (fl & 6u) == 6u) ? __int_as_float(0x7fc00000) : __int_as_float((fl & 2u) ? 0x7f800000 : (int)0xff800000);
}

}  // namespace gs
