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

// ------------------------------------------------------------------ the transposing butterfly (rgbd.hip, sdf.hip)
// A block's N <= 32 sums when every LANE brings N terms of its own (one pixel per lane): the geometry of steps 1 and 2 and
// their order of magnitude (six pairwise steps in the wave, then the waves in order), but as a TRANSPOSING butterfly: at step s a lane keeps one half of its values and hands
// the other half to its partner (the lane 2^s away), so the 32 (N + zeros) values per lane halve at every step -- 31
// exchanges per lane instead of N x 6 -- and steps 0 .. 3 are DPP moves in the vector pipeline (quad permutes, rotations of
// the 16-lane row), not LDS permutes: at one source pixel per lane the permutes of 29 plain butterflies were the kernel's whole
// time (16 us at 480 x 640).  Partners: lane ^ 1, lane ^ 2, the lane 4 further round its row (same low bits, bit 2 flipped),
// lane ^ 8, lane ^ 16, lane ^ 32.  Value k ends in the lanes whose low five bits are k's bits reversed.  Every addition is
// keep + received, in a fixed order: the same bits from run to run.
template <int CTRL>
__device__ __forceinline__ float rowsum_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int N, int CTRL>
__device__ __forceinline__ void rowsum_fold_dpp(float (&a)[32], bool up) {  // N values -> N / 2; `up` lanes keep the upper half
#pragma unroll
    for (int j = 0; j < N / 2; ++j) {
        const float send = up ? a[j] : a[j + N / 2], keep = up ? a[j + N / 2] : a[j];
        a[j] = keep + rowsum_dpp<CTRL>(send);
    }
}
// a[0 .. N) the lane's terms, a[N .. 32) zeros -> partials[blockIdx.x * N + n], the block's row; all WAVES waves arrive
template <int N, int WAVES>
__device__ __forceinline__ void block_row_transposed(float (&a)[32], float *__restrict__ partials) {
    static_assert(N <= 32, "one value per lane of half a wave");
    __shared__ float sm[WAVES][32];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    rowsum_fold_dpp<32, 0xB1>(a, lane & 1);    // quad_perm [1, 0, 3, 2]
    rowsum_fold_dpp<16, 0x4E>(a, lane & 2);    // quad_perm [2, 3, 0, 1]
    rowsum_fold_dpp<8, 0x124>(a, lane & 4);    // row_ror 4
    rowsum_fold_dpp<4, 0x128>(a, lane & 8);    // row_ror 8
    {
        const bool up = lane & 16;
        const float send = up ? a[0] : a[1], keep = up ? a[1] : a[0];
        a[0] = keep + __shfl_xor(send, 16, kWave);
    }
    a[0] = a[0] + __shfl_xor(a[0], 32, kWave);
    const int k = ((lane & 1) << 4) | ((lane & 2) << 2) | (lane & 4) | ((lane & 8) >> 2) | ((lane & 16) >> 4);
    if (lane < 32) sm[wid][k] = a[0];
    __syncthreads();
    if (threadIdx.x < N) {
        float v = 0.0f;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) v += sm[w][threadIdx.x];
        partials[blockIdx.x * N + threadIdx.x] = v;
    }
}

}  // namespace gs
