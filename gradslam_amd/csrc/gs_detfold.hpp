// gs_detfold.hpp -- the deterministic fold of the scattered target / normal adjoints (torch.use_deterministic_algorithms).
//
// The default reverse passes add d_bar / n_bar of every source i into row j = NN(i) of g_tgt / g_nrm with float atomics, in
// arrival order.  The DET variants store each contribution instead -- one row of DET_ROW words per (launch q, source i):
// d_bar (3) | n_bar (3) | j (int bits, -1 = no contribution) | pad -- and fold the rows into the targets afterwards in four
// launches, however many reverse launches wrote rows:
//   det_clear_k   zero the accumulators, the flags and the maximum
//   det_max_k     M = max |x| over every finite contribution (integer atomicMax on the float bits: exact, commutative)
//   det_acc_k     x -> x 2^E as a signed 128-bit fixed-point integer, added into a (lo, hi) pair of 64-bit words per
//                 (target, component) with integer atomics (the low word's wrap is carried into the high word by the adder
//                 that caused it); non-finite contributions set flag bits of their target instead
//   det_finish_k  per (target, component): the 128-bit sum rounded once to fp32 (nearest, ties to even), scaled by 2^-E
// Integer addition is associative, so the sums -- and the fp32 results -- do not depend on the order of arrival.
// Scale: with |x| < 2^(eb - 126) (eb = biased exponent of M) and at most 2^lg contributions per target, E = 252 - eb - lg
// keeps every sum below 2^126.  Conversion is exact for every bit of weight >= 2^-E (bits below are truncated: at least
// 2^(102 - lg) below M).  A flag word per target holds 3 bits per component: NaN, +inf, -inf; the result is what the
// float sum gives: NaN for a NaN or for both infinities, else the infinity.
#pragma once
#include "gs_common.hpp"
#include "gs_fixed128.hpp"

namespace gs {

constexpr int DET_ROW = 8;  // words per stored contribution

__device__ __forceinline__ void det_store_row(float *__restrict__ rows, int64_t i, const f3 dt, const f3 dn, int j) {
    int4 *p = reinterpret_cast<int4 *>(rows + DET_ROW * i);
    p[0] = make_int4(__float_as_int(dt.x), __float_as_int(dt.y), __float_as_int(dt.z), __float_as_int(dn.x));
    p[1] = make_int4(__float_as_int(dn.y), __float_as_int(dn.z), j, 0);
}
__device__ __forceinline__ void det_store_none(float *__restrict__ rows, int64_t i) {
    reinterpret_cast<int *>(rows)[DET_ROW * i + 6] = -1;
}

struct DetWs {
    float *rows;                // Q x cap_s x DET_ROW
    uint32_t *maxbits, *flags;  // 1 ; cap_t
    unsigned long long *acc;    // cap_t x 6 x (lo, hi)
};
static inline size_t det_ws_layout(int Q, int cap_s, int cap_t, void *ws, DetWs *out) {
    const size_t rows_b = align_up((size_t)Q * cap_s * DET_ROW * 4, 256), max_b = 256, flags_b = align_up((size_t)cap_t * 4, 256);
    const size_t acc_b = align_up((size_t)cap_t * 6 * 16, 256);
    if (ws && out) {
        char *p = (char *)ws;
        out->rows = (float *)p;
        out->maxbits = (uint32_t *)(p + rows_b);
        out->flags = (uint32_t *)(p + rows_b + max_b);
        out->acc = (unsigned long long *)(p + rows_b + max_b + flags_b);
    }
    return rows_b + max_b + flags_b + acc_b;
}
static inline int det_lg(int Q, int cap_s) {  // ceil(log2(most contributions one target can receive))
    const int64_t n = (int64_t)Q * cap_s;
    int lg = 0;
    while (((int64_t)1 << lg) < n) ++lg;
    return lg;
}

__global__ void det_clear_k(uint32_t *__restrict__ maxbits, uint32_t *__restrict__ flags, unsigned long long *__restrict__ acc,
                            const int32_t *__restrict__ d_nt, int cap_t) {
    const int nt = min(*d_nt, cap_t);
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (int i = tid; i < 12 * nt; i += stride) acc[i] = 0ull;
    for (int i = tid; i < nt; i += stride) flags[i] = 0u;
    if (tid == 0) *maxbits = 0u;
}

// grid (x: sources, y: launch q)
__global__ __launch_bounds__(256) void det_max_k(const float *__restrict__ rows, int cap_s, const int32_t *__restrict__ d_ns,
                                                 uint32_t *__restrict__ maxbits) {
    const int ns = min(*d_ns, cap_s);
    const int4 *R = reinterpret_cast<const int4 *>(rows + (size_t)blockIdx.y * cap_s * DET_ROW);
    int m = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += gridDim.x * blockDim.x) {
        const int4 a = R[2 * i], b = R[2 * i + 1];
        if (b.z < 0) continue;
        const int w[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const int u = w[c] & 0x7fffffff;
            if (u < 0x7f800000) m = max(m, u);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off, kWave));
    if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(maxbits, (uint32_t)m);
}

__global__ __launch_bounds__(256) void det_acc_k(const float *__restrict__ rows, int cap_s, const int32_t *__restrict__ d_ns,
                                                 const int32_t *__restrict__ d_nt, int cap_t, const uint32_t *__restrict__ maxbits,
                                                 int lg, uint32_t *__restrict__ flags, unsigned long long *__restrict__ acc) {
    const int ns = min(*d_ns, cap_s), nt = min(*d_nt, cap_t);
    const int E = det_scale(*maxbits, lg);
    const int4 *R = reinterpret_cast<const int4 *>(rows + (size_t)blockIdx.y * cap_s * DET_ROW);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += gridDim.x * blockDim.x) {
        const int4 a = R[2 * i], b = R[2 * i + 1];
        const int j = b.z;
        if (j < 0 || j >= nt) continue;
        const int w[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const uint32_t bits = (uint32_t)w[c];
            if ((bits & 0x7fffffffu) >= 0x7f800000u) {
                const uint32_t code = (bits & 0x7fffffu) ? 1u : ((bits >> 31) ? 4u : 2u);
                atomicOr(flags + j, code << (3 * c));
                continue;
            }
            const __int128 v = det_to_fixed(bits, E);
            if (v == 0) continue;
            unsigned long long *p = acc + ((int64_t)j * 6 + c) * 2;
            const unsigned long long lo = (unsigned long long)v;
            unsigned long long hi = (unsigned long long)(v >> 64);
            const unsigned long long old = atomicAdd(p, lo);
            hi += (old + lo < old) ? 1ull : 0ull;  // the carry out of the low word, counted once by the adder that caused it
            if (hi) atomicAdd(p + 1, hi);
        }
    }
}

// rows < min(nt, cap_t) of g_tgt / g_nrm (either may be NULL) are written, nothing else
__global__ void det_finish_k(const unsigned long long *__restrict__ acc, const uint32_t *__restrict__ flags,
                             const uint32_t *__restrict__ maxbits, int lg, const int32_t *__restrict__ d_nt, int cap_t,
                             float *__restrict__ g_tgt, float *__restrict__ g_nrm) {
    const int nt = min(*d_nt, cap_t);
    const int E = det_scale(*maxbits, lg);
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < 6 * nt; t += gridDim.x * blockDim.x) {
        const int row = t / 6, c = t - 6 * row;
        float *out = c < 3 ? g_tgt : g_nrm;
        if (!out) continue;
        const uint32_t fl = (flags[row] >> (3 * c)) & 7u;
        float r;
        if (fl) r = ((fl & 1u) || (fl & 6u) == 6u) ? __int_as_float(0x7fc00000) : __int_as_float((fl & 2u) ? 0x7f800000 : (int)0xff800000);
        else r = det_to_float(acc[2 * (int64_t)t], acc[2 * (int64_t)t + 1], E);
        out[3 * (int64_t)row + (c % 3)] = r;
    }
}

// the four fold launches over Q launches' rows (cap_s rows each, the first *d_ns of them written)
static inline int det_fold_run(const DetWs &w, int Q, int cap_s, const int32_t *d_ns, const int32_t *d_nt, int cap_t, float *g_tgt,
                               float *g_nrm, hipStream_t st, const char *name) {
    const int lg = det_lg(Q, cap_s);
    hipLaunchKernelGGL(det_clear_k, dim3(min(cdiv((int64_t)12 * cap_t, 256), 1024)), dim3(256), 0, st, w.maxbits, w.flags, w.acc, d_nt, cap_t);
    const dim3 grid(min(cdiv(cap_s, 256), 256), Q);
    hipLaunchKernelGGL(det_max_k, grid, dim3(256), 0, st, (const float *)w.rows, cap_s, d_ns, w.maxbits);
    hipLaunchKernelGGL(det_acc_k, grid, dim3(256), 0, st, (const float *)w.rows, cap_s, d_ns, d_nt, cap_t, (const uint32_t *)w.maxbits, lg,
                       w.flags, w.acc);
    hipLaunchKernelGGL(det_finish_k, dim3(min(cdiv((int64_t)6 * cap_t, 256), 1024)), dim3(256), 0, st, (const unsigned long long *)w.acc,
                       (const uint32_t *)w.flags, (const uint32_t *)w.maxbits, lg, d_nt, cap_t, g_tgt, g_nrm);
    GS_LAUNCH_CHECK(name);
    return GS_OK;
}

}  // namespace gs
