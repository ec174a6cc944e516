// gs_rowsum.hpp -- the fixed-order fp32 sum behind every reverse pass that is not a scatter: device functions only.
//
// THE ORDER.  Each thread of many blocks holds N terms; the N sums over all of them are formed in plain fp32, without atomics,
// in ONE order, so they have the same bits from run to run:
//   1. per wave, wave_sum's 64-lane butterfly (offsets 32, 16, .. 1); lane 0 leaves the wave's N sums in LDS;
//   2. behind a barrier, thread n < N adds the block's waves left to right, starting from wave 0's sum (block_row_sum), and
//      stores the block's row of N;
//   3. a finishing launch folds the rows (fold_rows): thread (g, k) = (tid / COLS, tid % COLS) adds rows g, g + GROUPS,
//      g + 2 GROUPS, .. of column k in ascending order onto +0; then thread k adds the GROUPS partial sums g = 0, 1, .. in
//      ascending order onto +0.
// A stored row may hold -0 where another form of step 2 would hold +0; every reader adds rows onto +0, so no sum can tell.
// tests/helpers.py restates the order in numpy (block_rows_f32, fold_rows_f32).
#pragma once

#include "gs_common.hpp"

namespace gs {

// step 2 for thread n, on its own: sm is [WAVES][N] wave sums, complete and visible (the caller's barrier)
template <int N, int WAVES>
__device__ __forceinline__ float block_row_sum(const float *sm, int n) {
    float s = sm[n];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s = s + sm[w * N + n];
    return s;
}

// steps 1 and 2 for a block of WAVES waves, all of them arriving: sum n of the row goes to *at(n), a functor so that the
// address is formed behind the barrier and holds no register across the butterflies
template <int N, int WAVES, class At>
__device__ __forceinline__ void block_row(const float (&acc)[N], At at) {
    __shared__ float sm[WAVES * N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const float v = wave_sum(acc[k]);
        if (lane == 0) sm[wave * N + k] = v;
    }
    __syncthreads();
    if (threadIdx.x < N) *at(threadIdx.x) = block_row_sum<N, WAVES>(sm, threadIdx.x);
}

// step 3 by a block of GROUPS * COLS threads: rows [nrow][N] -> out[0 .. N) in LDS; ends with a barrier.  Only the leading
// `live` columns are read (the others sum to +0).  Four loads in flight per thread: the rows come from other CUs' launches,
// and a 480 x 640 image leaves over a thousand of them.
template <int N, int GROUPS, int COLS>
__device__ __forceinline__ void fold_rows(const float *__restrict__ rows, int nrow, int live, float *out) {
    static_assert(N <= COLS, "one thread per column in every group");
    __shared__ float stage[N][GROUPS + 1];
    const int k = threadIdx.x % COLS, g = threadIdx.x / COLS;
    float v = 0.0f;
    if (k < live) {
#pragma unroll 4
        for (int r = g; r < nrow; r += GROUPS) v += rows[(int64_t)r * N + k];
    }
    if (k < N) stage[k][g] = v;
    __syncthreads();
    if (threadIdx.x < N) {
        float t = 0.0f;
#pragma unroll
        for (int q = 0; q < GROUPS; ++q) t += stage[threadIdx.x][q];
        out[threadIdx.x] = t;
    }
    __syncthreads();
}

}  // namespace gs
