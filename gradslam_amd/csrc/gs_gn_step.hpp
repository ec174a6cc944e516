// gs_gn_step.hpp -- what the Gauss-Newton loops of the two image-aligned odometries (rgbd.hip, sdf.hip) share, stated once:
// the level and status constants, the layout of the tape row and of an iteration's adjoint row, the loop's kernels that do not
// look at a pixel -- the start-up, X the step, Xb its reverse, the fold of the 12-wide rows, the seam's adjoint row -- and, on
// the host, their launches, the iteration schedule and the checks on the image and the loop's parameters.
// The kernels are WHOLE kernels, each `static`, so that either unit compiles its own copy of the same function: as bodies
// inlined into per-unit kernels they compiled to other instructions than in place ("SDF odometry";
// profiles/gn_kernels_isa.txt).  What stays in the units is what looks at a pixel: L the linearise kernels with the lane's 29
// terms, Lb the pixel-reverse kernels with their M | g | e2 prologue, the pyramids and the finishes.
#pragma once

#include <algorithm>

#include "gs_se3_bwd.hpp"  // fold_rows (gs_rowsum.hpp), BWD_T, BWD_GROUPS, top3_times_Tt, pull_gT, se3_exp_bwd; it brings
                           // gs_icp_step.hpp (solve6, se3_exp_dev) and gs_icp_reduce.hpp (reduce_partials, expand44, NACC)

namespace gs {

constexpr int GN_MAX_LEVELS = 8, GN_MIN_SIDE = 4;       // the coarsest level (grid) is at least 4 x 4
constexpr int GN_STATUS_FEW = 1, GN_STATUS_SOLVE = 2;  // fewer than 6 valid pixels | the solve (or the composed transform) was not finite
// An iteration's tape row of batch element b (GN_TAPE_WORDS floats at tape + GN_TAPE_WORDS b): T before the step (16), the 29
// sums as reduced (g not yet negated), xi (6), 1 if the step was applied else 0 -- what the reverse pass replays.
constexpr int GN_TAPE_WORDS = 64, GN_TAPE_SUMS = 16, GN_TAPE_XI = 45, GN_TAPE_APPLIED = 51;
// An iteration's adjoint row of batch element b, which Xb (or the seam's gn_sums_adj_k) writes and the pixel-reverse kernels read:
constexpr int GN_ADJ_WORDS = 32;  // adjoints of the 28 sums AS REDUCED (the six of g: of the sum, not of minus it; cnt has none)
constexpr int GN_ADJ_LIVE = 28;   // 1: the pixel pass applies them; 0: a step that was not applied -- nothing, not even 0 x inf

// ------------------------------------------------------------------ the start-up
// T[b] = out_T[b] = init[b] or the identity; info = 0.  One thread of a 256-thread block per word.
static __global__ __launch_bounds__(256) void gn_init_k(const float *__restrict__ init, int B, int n_info, float *__restrict__ Tall,
                                                       float *__restrict__ out_T, float *__restrict__ info) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 16 * B) {
        const float v = init ? init[i] : (((i & 15) % 5 == 0) ? 1.0f : 0.0f);
        Tall[i] = v;
        out_T[i] = v;
    }
    if (i < n_info) info[i] = 0.0f;
}

// ------------------------------------------------------------------ X: step
// grid B, 1024 threads.  Reduces batch element b's `nblocks` partial rows; `sums` (B, 29: H upper | g = -sum | err | cnt)
// is written when given; with `apply`, lane 0 solves and composes T[b] <- exp(xi) T[b], and writes out_T[b] and the level's
// info row (cnt, err, status bits of the level so far, iterations run at the level).
// TAPE: also the iteration's tape row of batch element b (GN_TAPE_*).
template <bool TAPE>
static __global__ __launch_bounds__(1024) void gn_step_k(float *__restrict__ Tall, const float *__restrict__ partials, int nblocks, int prow,
                                                        float damp, int level, int levels, int it, int apply, float *__restrict__ out_T,
                                                        float *__restrict__ info, float *__restrict__ sums, float *__restrict__ tape) {
    __shared__ float acc[NACC];
    __shared__ double lu_sm[42];
    const int b = blockIdx.x;
    reduce_partials(partials + (int64_t)b * prow * NACC, nblocks, acc);
    if (threadIdx.x != 0) return;
    if (sums) {
        for (int k = 0; k < NACC; ++k) sums[NACC * b + k] = (k >= 21 && k < 27) ? -acc[k] : acc[k];
    }
    if (!apply) return;
    float *T = Tall + 16 * b;
    float *row = info + ((int64_t)b * levels + level) * 4;
    int status = it == 0 ? 0 : (int)row[2];
    const float cnt = acc[28];
    float *rec = TAPE ? tape + GN_TAPE_WORDS * b : nullptr;
    if constexpr (TAPE) {
        for (int k = 0; k < 16; ++k) rec[k] = T[k];
        for (int k = 0; k < NACC; ++k) rec[GN_TAPE_SUMS + k] = acc[k];
        for (int k = 0; k < 6; ++k) rec[GN_TAPE_XI + k] = 0.0f;
        rec[GN_TAPE_APPLIED] = 0.0f;
    }
    if (cnt < 6.0f) {
        status |= GN_STATUS_FEW;
    } else {
        float hg[44], xi[6], dT[16], Tn[16];
        expand44(acc, hg);
        for (int k = 0; k < 6; ++k) hg[36 + k] = -hg[36 + k];
        solve6(hg, hg + 36, damp, xi, lu_sm);
        bool fin = true;
        for (int k = 0; k < 6; ++k) fin = fin && fabsf(xi[k]) < INFINITY;
        if (fin) {
            se3_exp_dev(xi, dT);
            compose44(dT, T, Tn);
            for (int k = 0; k < 12; ++k) fin = fin && fabsf(Tn[k]) < INFINITY;
        }
        if (fin) {
            if constexpr (TAPE) {
                for (int k = 0; k < 6; ++k) rec[GN_TAPE_XI + k] = xi[k];
                rec[GN_TAPE_APPLIED] = 1.0f;
            }
            for (int k = 0; k < 16; ++k) T[k] = Tn[k];
        } else {
            status |= GN_STATUS_SOLVE;
        }
    }
    row[0] = cnt;
    row[1] = acc[27];
    row[2] = (float)status;
    row[3] = (float)(it + 1);
    for (int k = 0; k < 16; ++k) out_T[16 * b + k] = T[k];
}

// ------------------------------------------------------------------ Xb: step reverse, and what goes with it
// out[b] (stride floats, 12 or 16: the bottom row is zero) = g_in[b] rows 0..2 (NULL: zero) + the sum of b's 12-wide rows
static __global__ __launch_bounds__(BWD_T) void gn_fold12_k(const float *__restrict__ gT_in, const float *__restrict__ partials12, int nblocks,
                                                           int prow, float *__restrict__ out, int stride) {
    __shared__ float sums[12];
    const int b = blockIdx.x;
    fold_rows<12, BWD_GROUPS, 16>(partials12 + (int64_t)b * prow * 12, nblocks, 12, sums);
    if ((int)threadIdx.x < stride)
        out[stride * b + threadIdx.x] = threadIdx.x < 12 ? (gT_in ? gT_in[16 * b + threadIdx.x] : 0.0f) + sums[threadIdx.x] : 0.0f;
}

// The seam (gs_rgbd_rows_bwd, gs_sdf_rows_bwd): the adjoints of the sums as the rows call returns them (g = MINUS the sum) -> of
// the sums as reduced; the adjoint of cnt is ignored
static __global__ __launch_bounds__(256) void gn_sums_adj_k(const float *__restrict__ g_sums, int B, float *__restrict__ adj) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * GN_ADJ_WORDS) return;
    const int b = i / GN_ADJ_WORDS, k = i - b * GN_ADJ_WORDS;
    const float g = k < 28 ? g_sums[NACC * b + k] : 0.0f;
    adj[i] = k == GN_ADJ_LIVE ? 1.0f : ((k >= 21 && k < 27) ? -g : g);
}

// grid B, one 256-thread block per batch element.  gT (B,16): the carried adjoint of T (rows 0..2), updated in place; rec: this
// iteration's tape rows; adj: its (B, GN_ADJ_WORDS).  The pixel pass before left 12-sum rows -- the adjoint of T_{k+1} through ITS
// linearisation -- which are folded (fold_rows) into the carried adjoint; then, one lane, fp64 where the forward's fp32 value
// would lose the gradient: dT-bar = T-bar_{k+1} T_k^T, T-bar_k = dT^T T-bar_{k+1}, the exponential's and the solve's adjoints ->
// the adjoints of the iteration's 28 sums.  A step that was not applied is the identity.
// POSES (the SDF loop, whose pixel has a second transform): gP (B,16), the running adjoint of the poses, takes the same fold of
// the rows of partP (NULL: the poses' adjoint is not wanted).  Without POSES the two arguments are not read.
template <bool POSES>
static __global__ __launch_bounds__(BWD_T) void gn_step_bwd_k(float *__restrict__ gTall, const float *__restrict__ partials12, int nblocks,
                                                             int prow, const float *__restrict__ rec_all, float damp,
                                                             float *__restrict__ adj_all, float *__restrict__ gPall,
                                                             const float *__restrict__ partP) {
    __shared__ float sums[12];
    __shared__ double lu_sm[42];
    __shared__ float g[16], xi[6], dT[16], hg[44], gx[6], y[6];
    __shared__ double gdT[12], gxi[6];
    const int b = blockIdx.x;
    fold_rows<12, BWD_GROUPS, 16>(partials12 + (int64_t)b * prow * 12, nblocks, 12, sums);
    if constexpr (POSES) {
        __shared__ float psums[12];
        if (partP) {
            fold_rows<12, BWD_GROUPS, 16>(partP + (int64_t)b * prow * 12, nblocks, 12, psums);
            if (threadIdx.x < 12) gPall[16 * b + threadIdx.x] = gPall[16 * b + threadIdx.x] + psums[threadIdx.x];
        }
    }
    if (threadIdx.x != 0) return;
    const float *rec = rec_all + GN_TAPE_WORDS * b;
    float *gT = gTall + 16 * b, *A = adj_all + GN_ADJ_WORDS * b;
    for (int k = 0; k < 16; ++k) g[k] = k < 12 ? gT[k] + sums[k] : 0.0f;
    for (int k = 0; k < GN_ADJ_WORDS; ++k) A[k] = 0.0f;
    if (rec[GN_TAPE_APPLIED] != 0.0f) {
        for (int k = 0; k < 6; ++k) xi[k] = rec[GN_TAPE_XI + k];
        se3_exp_dev(xi, dT);  // the forward's dT, bit for bit
        top3_times_Tt(g, rec, gdT);
        pull_gT(g, dT);
        se3_exp_bwd(xi, gdT, gxi);
        // xi = M^-1 g', M = H + damp I symmetric, g' = MINUS the six sums:  y = M^-1 xi-bar;  H-bar = -y xi^T, g'-bar = y
        expand44(rec + GN_TAPE_SUMS, hg);
        for (int k = 0; k < 6; ++k) gx[k] = (float)gxi[k];
        solve6(hg, gx, damp, y, lu_sm);
        int q = 0;
        for (int u = 0; u < 6; ++u)
            for (int v = u; v < 6; ++v) A[q++] = u == v ? -(y[u] * xi[u]) : -(y[u] * xi[v] + y[v] * xi[u]);
        for (int u = 0; u < 6; ++u) A[21 + u] = -y[u];
        A[GN_ADJ_LIVE] = 1.0f;
    }
    for (int k = 0; k < 12; ++k) gT[k] = g[k];
}

// ------------------------------------------------------------------ host
// The two launches every entry point of either loop makes the same way (the caller checks them: GS_LAUNCH_CHECK with its name)
static inline void gn_launch_init(const float *init, int B, int levels, float *T, float *out_T, float *info, hipStream_t st) {
    const int n_info = B * levels * 4;
    hipLaunchKernelGGL(gn_init_k, dim3(cdiv(std::max(16 * B, n_info), 256)), dim3(256), 0, st, init, B, n_info, T, out_T, info);
}
// (tape: this iteration's rows, or NULL for the loop without a tape and for the rows calls)
static inline void gn_launch_step(int B, float *T, const float *partials, int nblocks, int prow, float damp, int level, int levels, int it,
                                  int apply, float *out_T, float *info, float *sums, float *tape, hipStream_t st) {
    const auto step = tape ? gn_step_k<true> : gn_step_k<false>;
    hipLaunchKernelGGL(step, dim3(B), dim3(1024), 0, st, T, partials, nblocks, prow, damp, level, levels, it, apply, out_T, info, sums, tape);
}

// The iteration schedule: the levels run coarsest (levels - 1) first.  base[l]: iterations that ran before level l's.
struct GnSchedule { int total, base[GN_MAX_LEVELS]; };
static inline GnSchedule gn_schedule(int levels, const int *numiters) {
    GnSchedule s;
    s.total = 0;
    for (int l = levels - 1; l >= 0; --l) { s.base[l] = s.total; s.total += numiters[l]; }
    return s;
}
// the bound on a SUMMED iteration count, as the size queries take it (GN_REQUIRE_LOOP bounds each level's)
static inline bool gn_total_ok(int levels, int64_t total) { return total >= 0 && total <= (int64_t)levels * (1 << 20); }

// The bounds on (B, H, W) both units share: 0 or the number (1..3) of the first one broken; a unit numbers its own from 4.
static inline int gn_image_fault(int B, int H, int W) {
    if (!(B >= 1 && B <= 65535)) return 1;
    if (!(H >= 1 && W >= 1 && (int64_t)H * W <= (1 << 24))) return 2;
    if (!((int64_t)B * H * W <= (1 << 30))) return 3;
    return 0;
}
#define GN_REQUIRE_IMAGE(name, fault)                                                                                    \
    do {                                                                                                                 \
        GS_REQUIRE((fault) != 1, name ": B must be in [1, 65535], got %d", B);                                           \
        GS_REQUIRE((fault) != 2, name ": H x W must be positive and at most 2^24 pixels, got %d x %d", H, W);            \
        GS_REQUIRE((fault) != 3, name ": B H W must be at most 2^30, got %d x %d x %d", B, H, W);                        \
    } while (0)
#define GN_REQUIRE_LOOP(name)                                                                                                     \
    do {                                                                                                                          \
        GS_REQUIRE(damp >= 0.0f && damp < INFINITY, name ": damp must be finite and not negative, got %g", (double)damp);         \
        for (int l = 0; l < levels; ++l)                                                                                          \
            GS_REQUIRE(numiters[l] >= 0 && numiters[l] <= (1 << 20), name ": numiters[%d] must be in [0, 2^20], got %d", l, numiters[l]); \
    } while (0)

}  // namespace gs
