// gs_icp_reduce.hpp -- the fixed-order reduction (J) of the 29 linearisation sums over the blocks' partial rows (a block's
// row itself: gs_rowsum.hpp's block_row).  Included by icp.hip ahead of its stand-alone kernels, and by gs_icp_step.hpp.
//
// J  gather + 29-term reduction, HBM/L2-bound at 40 algorithmic bytes per source point; wave
//    butterflies + a fixed-order two-level tree (deterministic, no float atomics).  Fused into the association
//    kernel's epilogue inside the loops; linearize_k / finalize44_k serve the stand-alone entry points.
#pragma once

#include "gs_icp_assoc.hpp"

namespace gs {

// Fixed-order reduction of the per-block partials by a 1024-thread block into acc_sm[NACC]:
// thread (g, k) = (t / 32, t % 32) sums rows g, g+32, g+64, ... of accumulator k (coalesced over k),
// then 29 threads add the 32 group sums in order.  Two short LDS stages, no shuffle chains.
constexpr int RP_LOADS = 16;  // reduce_partials: loads in flight per thread
constexpr int RP_FEW = 10;    // knn1_loop_k for launches of at most 32 * RP_FEW blocks (a 160 x 120 frame: 300): every instruction of its
                              // prologue is executed by sixteen waves on four SIMDs
// The two halves of one round, for a caller that has other loads to put in flight between them (knn1_loop_k: a launch of at
// most 32 * RP_LOADS = 512 rows is ONE round): rp_issue requests thread (g, k)'s rows, rp_finish sums them in the order below.
template <int NL = RP_LOADS>
__device__ __forceinline__ void rp_issue(const float *__restrict__ partials, int nblocks, int b0, float (&a)[RP_LOADS]) {
    // Clamped addresses, unconditional loads; rp_sum masks what lies outside.  (A select -- or a branch -- at the load makes
    // the compiler wait for each value where it is requested: sixteen trips in a row instead of one.)
    // NL < RP_LOADS: the caller knows that nblocks <= 32 NL (the rows beyond are zeros in either form: same sums).
    const int kc = min((int)(threadIdx.x & 31), NACC - 1), last = max(nblocks - 1, 0);
#pragma unroll
    for (int u = 0; u < RP_LOADS; ++u) a[u] = u < NL ? partials[min(b0 + 32 * u, last) * NACC + kc] : 0.0f;
}
template <int NL = RP_LOADS>
__device__ __forceinline__ float rp_sum(const float (&a)[RP_LOADS], int nblocks, int b0, float v) {
    const int k = threadIdx.x & 31;
#pragma unroll
    for (int u = 0; u < NL; ++u) v += (k < NACC && b0 + 32 * u < nblocks) ? a[u] : 0.0f;
    return v;
}
// knn1_loop_k's form: rows b0, b0 + 32, ... b0 + 32 (NL - 1) exist and hold zeros where no block wrote (partial_rows_alloc,
// icp_prepare_k), so nothing is clamped or masked -- three instructions per row instead of seven, and each of them is
// executed by up to sixteen waves on four SIMDs.  Lanes k >= NACC sum words of the neighbouring row: never read.
template <int NL>
__device__ __forceinline__ void rp_issue_padded(const float *__restrict__ partials, int b0, float (&a)[RP_LOADS]) {
    const float *p = partials + b0 * NACC + (threadIdx.x & 31);
#pragma unroll
    for (int u = 0; u < RP_LOADS; ++u) a[u] = u < NL ? p[32 * NACC * u] : 0.0f;
}
template <int NL>
__device__ __forceinline__ float rp_sum_padded(const float (&a)[RP_LOADS]) {
    float v = 0.0f;
#pragma unroll
    for (int u = 0; u < NL; ++u) v += a[u];
    return v;
}
__device__ __forceinline__ void rp_finish(float v, float *acc_sm) {
    __shared__ float stage[32][33];
    const int k = threadIdx.x & 31, g = threadIdx.x >> 5;  // blockDim.x == 1024 -> g in [0, 32)
    stage[k][g] = v;
    __syncthreads();
    if (threadIdx.x < NACC) {
        float t = 0.0f;
#pragma unroll
        for (int q = 0; q < 32; ++q) t += stage[threadIdx.x][q];
        acc_sm[threadIdx.x] = t;
    }
    __syncthreads();
}
// rp_finish for a 512-thread block: thread (g, k) brings the sums of row groups g and g + 16
__device__ __forceinline__ void rp_finish2(float v, float v2, float *acc_sm) {
    __shared__ float stage[32][33];
    const int k = threadIdx.x & 31, g = threadIdx.x >> 5;  // blockDim.x == 512 -> g in [0, 16)
    stage[k][g] = v;
    stage[k][g + 16] = v2;
    __syncthreads();
    if (threadIdx.x < NACC) {
        float t = 0.0f;
#pragma unroll
        for (int q = 0; q < 32; ++q) t += stage[threadIdx.x][q];
        acc_sm[threadIdx.x] = t;
    }
    __syncthreads();
}
// rp_finish for a block in which only wave 0 needs the sums (knn1_loop_k<true>: the other fifteen waves stage the search's
// windows meanwhile, and the two block barriers above kept them from starting for 1.2 us -- phase stamps, r04a).  Every
// wave leaves its 128 sums in LDS, waits for its OWN LDS writes (the caller's state words among them) and counts itself in;
// wave 0 waits for the count, then adds the 32 group sums in the same order as rp_finish.  `cnt` must be zero and visible
// to all waves before the first of them gets here (the caller's raw barrier at kernel start).  NW: the block's waves; an
// eight-wave block brings up to three groups per thread (g3).
template <int NW>
__device__ __forceinline__ void rp_finish_wave0(float v, int g, float v2, int g2, float v3, int g3, float *acc_sm, unsigned int *cnt) {
    __shared__ float stage[32][33];
    const int k = threadIdx.x & 31;
    if (g >= 0) stage[k][g] = v;     // (g, g2: the row groups this thread summed, -1 = none -- knn1_loop_k hands the planning
    if (g2 >= 0) stage[k][g2] = v2;  // waves' groups to two of the waves that only wait)
    if (NW != 16 && g3 >= 0) stage[k][g3] = v3;
    if (threadIdx.x >= 64) {
        if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {
        while (__hip_atomic_load(cnt, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < (unsigned int)(NW - 1)) __builtin_amdgcn_s_sleep(1);
        if (threadIdx.x < NACC) {
            float t = 0.0f;
#pragma unroll
            for (int q = 0; q < 32; ++q) t += stage[threadIdx.x][q];
            acc_sm[threadIdx.x] = t;
        }
    }
}
__device__ __forceinline__ void reduce_partials(const float *__restrict__ partials, int nblocks, float *acc_sm) {
    const int g = threadIdx.x >> 5;
    float v = 0.0f;
    // The rows were written by the previous launch on other CUs: every read is a trip to memory-side
    // cache (~1.5 us), so what matters is how many of them are in flight -- sixteen per thread and round: the 512
    // rows of a full chip (two tiles per CU) in ONE round.
    for (int b0 = g; b0 < nblocks; b0 += 32 * RP_LOADS) {
        float a[RP_LOADS];
        rp_issue(partials, nblocks, b0, a);
        v = rp_sum(a, nblocks, b0, v);
    }
    rp_finish(v, acc_sm);
}

// H (6x6 symmetric) | g | e | cnt from the 29 accumulators
__device__ __forceinline__ void expand44(const float *acc, float *out44) {
    int q = 0;
    for (int u = 0; u < 6; ++u)
        for (int v = u; v < 6; ++v) { out44[6 * u + v] = acc[q]; out44[6 * v + u] = acc[q]; ++q; }
    for (int u = 0; u < 6; ++u) out44[36 + u] = acc[21 + u];
    out44[42] = acc[27];
    out44[43] = acc[28];
}

}  // namespace gs
