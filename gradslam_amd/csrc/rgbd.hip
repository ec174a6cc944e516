// rgbd.hip -- dense RGB-D odometry: joint photometric + depth alignment of two frames over an image pyramid, coarse to fine
// (gs_rgbd_odometry, gs_rgbd_rows, gs_rgbd_pyramid) and its reverse pass (gs_rgbd_odometry_taped, gs_rgbd_odometry_bwd,
// gs_rgbd_rows_bwd: Xb, Lb, Pb further down).  The rule -- every fp32 operation in order -- is stated in
// include/gradslam_hip.h above the entry points; this file follows it line by line (the library is built without contraction).
//
// P  pyramid: level 0 is (intensity, depth or 0) per pixel as ONE float2, so that a bilinear corner is one 8-byte load; every
//    further level is a 2 x 2 reduction of the level before.  One launch per frame and level.
// L  linearise: one source pixel per lane: warp, four corner loads, the two Jacobian rows and residuals, the lane's 29 terms;
//    a transposing wave butterfly, then the waves in order, leave one partial row per block (gs_icp_reduce.hpp's geometry).
// X  step: a launch of its own, one 1024-thread block per batch element: reduce_partials (fixed order), then one lane solves
//    (gs::solve6, fp64) and composes T <- exp(xi) T.  Two launches per iteration, no float atomics, nothing synchronises the
//    host; the loop state (T per batch element) lives in the workspace.
#include <math.h>
#include <stddef.h>
#include <algorithm>
#include <type_traits>

// gs_icp_step.hpp (solve6, se3_exp_dev; it brings gs_icp_reduce.hpp) also DEFINES icp.hip's stand-alone step kernel, a plain
// __global__ with external linkage: a second translation unit that includes the header as it is would define the symbol a
// second time.  This unit's copy gets a name of its own; nothing launches it.
#define icp_step_k icp_step_k_in_rgbd_unit
#include "gs_icp_step.hpp"
#undef icp_step_k
#include "gs_fixed128.hpp"
#include "gs_se3_bwd.hpp"

namespace gs {

constexpr int RGBD_T = LIN_T;        // lanes (= source pixels) per linearise block: block_reduce_store's geometry
constexpr int RGBD_MAX_LEVELS = 8;
constexpr int RGBD_MIN_SIDE = 4;     // the coarsest level is at least 4 x 4
constexpr int RGBD_STATUS_FEW = 1;   // fewer than 6 valid pixels
constexpr int RGBD_STATUS_SOLVE = 2; // the solve (or the composed transform) was not finite

struct RgbdCam {
    float fx, fy, cx, cy;
};
// intrinsics (4 x 4 row-major) at pyramid level `level`: fx, fy halve; cx' = (cx + 0.5) / 2 - 0.5 (pixel centres at integers)
__device__ __forceinline__ RgbdCam rgbd_cam(const float *__restrict__ K, int level) {
    RgbdCam c{K[0], K[5], K[2], K[6]};
    for (int l = 0; l < level; ++l) {
        c.fx = c.fx * 0.5f;
        c.fy = c.fy * 0.5f;
        c.cx = (c.cx + 0.5f) * 0.5f - 0.5f;
        c.cy = (c.cy + 0.5f) * 0.5f - 0.5f;
    }
    return c;
}

// ------------------------------------------------------------------ P: pyramid
__global__ __launch_bounds__(256) void rgbd_level0_k(const float *__restrict__ depth, const float *__restrict__ rgb, int64_t n,
                                                    float rgb_scale, float2 *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
    const float I = rgb_scale * ((0.299f * r + 0.587f * g) + 0.114f * b);
    const float d = depth[i];
    out[i] = make_float2(I, (d > 0.0f && d < INFINITY) ? d : 0.0f);
}

// in: (B, Hp, Wp) of the level before; out: (B, Hl, Wl) with Hl = Hp / 2, Wl = Wp / 2.  grid (blocks of 256 pixels, B)
__global__ __launch_bounds__(256) void rgbd_down_k(const float2 *__restrict__ in, int Hp, int Wp, int Hl, int Wl, float ddm,
                                                  float2 *__restrict__ out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= Hl * Wl) return;
    const int v = p / Wl, u = p - v * Wl;
    const float2 *src = in + (int64_t)blockIdx.y * Hp * Wp + (int64_t)(2 * v) * Wp + 2 * u;
    const float2 c[4] = {src[0], src[1], src[Wp], src[Wp + 1]};
    const float I = (((c[0].x + c[1].x) + c[2].x) + c[3].x) * 0.25f;
    float dmin = INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k) dmin = (c[k].y > 0.0f && c[k].y < dmin) ? c[k].y : dmin;
    float s = 0.0f;
    int n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (c[k].y > 0.0f && c[k].y - dmin <= ddm) { s = s + c[k].y; ++n; }
    out[(int64_t)blockIdx.y * Hl * Wl + p] = make_float2(I, n > 0 ? s / (float)n : 0.0f);
}

// ------------------------------------------------------------------ L: linearise
// The block's 29 sums -> partials[blockIdx.x], in block_reduce_store's geometry and order of magnitude (six pairwise steps in
// the wave, then the waves in order), but as a TRANSPOSING butterfly: at step s a lane keeps one half of its values and hands
// the other half to its partner (the lane 2^s away), so the 32 (29 + 3 zeros) values per lane halve at every step -- 31
// exchanges per lane instead of 29 x 6 -- and steps 0 .. 3 are DPP moves in the vector pipeline (quad permutes, rotations of
// the 16-lane row), not LDS permutes: at one source pixel per lane the permutes of 29 plain butterflies were the kernel's whole
// time (16 us at 480 x 640).  Partners: lane ^ 1, lane ^ 2, the lane 4 further round its row (same low bits, bit 2 flipped),
// lane ^ 8, lane ^ 16, lane ^ 32.  Value k ends in the lanes whose low five bits are k's bits reversed.  Every addition is
// keep + received, in a fixed order: the same bits from run to run.
template <int CTRL>
__device__ __forceinline__ float rgbd_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int N, int CTRL>
__device__ __forceinline__ void rgbd_fold_dpp(float (&a)[32], bool up) {  // N values -> N / 2; `up` lanes keep the upper half
#pragma unroll
    for (int j = 0; j < N / 2; ++j) {
        const float send = up ? a[j] : a[j + N / 2], keep = up ? a[j + N / 2] : a[j];
        a[j] = keep + rgbd_dpp<CTRL>(send);
    }
}
__device__ __forceinline__ void rgbd_block_reduce_store(float (&a)[32], float *__restrict__ partials) {
    __shared__ float sm[RGBD_T / 64][32];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    rgbd_fold_dpp<32, 0xB1>(a, lane & 1);    // quad_perm [1, 0, 3, 2]
    rgbd_fold_dpp<16, 0x4E>(a, lane & 2);    // quad_perm [2, 3, 0, 1]
    rgbd_fold_dpp<8, 0x124>(a, lane & 4);    // row_ror 4
    rgbd_fold_dpp<4, 0x128>(a, lane & 8);    // row_ror 8
    {
        const bool up = lane & 16;
        const float send = up ? a[0] : a[1], keep = up ? a[1] : a[0];
        a[0] = keep + __shfl_xor(send, 16, kWave);
    }
    a[0] = a[0] + __shfl_xor(a[0], 32, kWave);
    const int k = ((lane & 1) << 4) | ((lane & 2) << 2) | (lane & 4) | ((lane & 8) >> 2) | ((lane & 16) >> 4);
    if (lane < 32) sm[wid][k] = a[0];
    __syncthreads();
    if (threadIdx.x < NACC) {
        float v = 0.0f;
#pragma unroll
        for (int w = 0; w < RGBD_T / 64; ++w) v += sm[w][threadIdx.x];
        partials[blockIdx.x * NACC + threadIdx.x] = v;
    }
}

// grid (blocks of RGBD_T source pixels, B).  tgt / src: this level's (B, Hl, Wl) float2 images; K (B, 4, 4) of level 0;
// T (B, 16).  partials: row blockIdx.x of batch element b at partials + (b * prow + blockIdx.x) * NACC.
// ROWS: also write the per-pixel valid flag and the 14 floats J_I | r_I | J_D | r_D (zeros where not valid).
template <bool ROWS>
__global__ __launch_bounds__(RGBD_T) void rgbd_linearize_k(const float2 *__restrict__ tgt, const float2 *__restrict__ src, int Hl,
                                                          int Wl, int level, const float *__restrict__ K,
                                                          const float *__restrict__ Tall, float wI, float wD, float ddm,
                                                          float *__restrict__ partials, int prow, int32_t *__restrict__ valid,
                                                          float *__restrict__ rows) {
    const int b = blockIdx.y, npix = Hl * Wl;
    const int p = blockIdx.x * RGBD_T + threadIdx.x;
    const RgbdCam cam = rgbd_cam(K + 16 * b, level);
    const float *__restrict__ T = Tall + 16 * b;
    const float2 *__restrict__ timg = tgt + (int64_t)b * npix;

    float JI[6], JD[6], rI = 0.0f, rD = 0.0f;
#pragma unroll
    for (int k = 0; k < 6; ++k) { JI[k] = 0.0f; JD[k] = 0.0f; }
    bool ok = p < npix;
    float2 s = make_float2(0.0f, 0.0f);
    int v = 0, u = 0;
    if (ok) {
        v = p / Wl;
        u = p - v * Wl;
        s = src[(int64_t)b * npix + p];
        ok = s.y > 0.0f;
    }
    if (ok) {
        const float d = s.y;
        const float px = d * (((float)u - cam.cx) / cam.fx), py = d * (((float)v - cam.cy) / cam.fy);
        const float qx = ((T[0] * px + T[1] * py) + T[2] * d) + T[3];
        const float qy = ((T[4] * px + T[5] * py) + T[6] * d) + T[7];
        const float qz = ((T[8] * px + T[9] * py) + T[10] * d) + T[11];
        ok = qz > 0.0f;
        const float iz = 1.0f / qz;
        const float x = (cam.fx * qx) * iz + cam.cx, y = (cam.fy * qy) * iz + cam.cy;
        const float xf = floorf(x), yf = floorf(y);
        // 0 <= i <= W - 2 and 0 <= j <= H - 2 (a NaN fails every comparison)
        ok = ok && xf >= 0.0f && xf <= (float)(Wl - 2) && yf >= 0.0f && yf <= (float)(Hl - 2);
        if (ok) {
            const int i = (int)xf, j = (int)yf;
            const float a = x - xf, bb = y - yf;
            const float2 *c = timg + (int64_t)j * Wl + i;
            const float2 c00 = c[0], c10 = c[1], c01 = c[Wl], c11 = c[Wl + 1];  // c_xy: x offset first
            ok = c00.y > 0.0f && c10.y > 0.0f && c01.y > 0.0f && c11.y > 0.0f;
            // bilinear interpolants and their exact derivatives
            const float iX0 = c10.x - c00.x, iX1 = c11.x - c01.x, dX0 = c10.y - c00.y, dX1 = c11.y - c01.y;
            const float iTop = c00.x + a * iX0, iBot = c01.x + a * iX1, dTop = c00.y + a * dX0, dBot = c01.y + a * dX1;
            const float Ih = iTop + bb * (iBot - iTop), Dh = dTop + bb * (dBot - dTop);
            const float Ix = iX0 + bb * (iX1 - iX0), Iy = iBot - iTop, Dx = dX0 + bb * (dX1 - dX0), Dy = dBot - dTop;
            const float ri = Ih - s.x, rd = Dh - qz;
            ok = ok && fabsf(rd) <= ddm;
            if (ok) {
                const float gx = cam.fx * iz, gy = cam.fy * iz;
                // d(value) / dq as a row (c0, c1, c2); d q / d xi = [I | -q^]  ->  J = w (c | q x c)
                const float i0 = Ix * gx, i1 = Iy * gy, i2 = -((i0 * qx + i1 * qy) * iz);
                const float d0 = Dx * gx, d1 = Dy * gy, d2 = -((d0 * qx + d1 * qy) * iz) - 1.0f;
                JI[0] = wI * i0; JI[1] = wI * i1; JI[2] = wI * i2;
                JI[3] = wI * (qy * i2 - qz * i1); JI[4] = wI * (qz * i0 - qx * i2); JI[5] = wI * (qx * i1 - qy * i0);
                JD[0] = wD * d0; JD[1] = wD * d1; JD[2] = wD * d2;
                JD[3] = wD * (qy * d2 - qz * d1); JD[4] = wD * (qz * d0 - qx * d2); JD[5] = wD * (qx * d1 - qy * d0);
                rI = wI * ri;
                rD = wD * rd;
            }
        }
    }
    if (ROWS && p < npix) {
        const int64_t o = (int64_t)b * npix + p;
        valid[o] = ok ? 1 : 0;
        float *r = rows + 14 * o;
#pragma unroll
        for (int k = 0; k < 6; ++k) { r[k] = JI[k]; r[7 + k] = JD[k]; }
        r[6] = rI;
        r[13] = rD;
    }
    // the lane's 29 terms: upper triangle of J_I^T J_I + J_D^T J_D | J_I^T r_I + J_D^T r_D | r_I^2 + r_D^2 | 1
    float acc[32];
    int q = 0;
#pragma unroll
    for (int m = 0; m < 6; ++m)
#pragma unroll
        for (int n = m; n < 6; ++n) acc[q++] = JI[m] * JI[n] + JD[m] * JD[n];
#pragma unroll
    for (int m = 0; m < 6; ++m) acc[21 + m] = JI[m] * rI + JD[m] * rD;
    acc[27] = rI * rI + rD * rD;
    acc[28] = ok ? 1.0f : 0.0f;
    acc[29] = 0.0f; acc[30] = 0.0f; acc[31] = 0.0f;
    rgbd_block_reduce_store(acc, partials + (int64_t)b * prow * NACC);
}

// ------------------------------------------------------------------ X: step
// grid B, 1024 threads.  Reduces batch element b's `nblocks` partial rows; `sums` (B, 29: H upper | g = -sum | err | cnt)
// is written when given; with `apply`, lane 0 solves and composes T[b] <- exp(xi) T[b], and writes out_T[b] and the level's
// info row (cnt, err, status bits of the level so far, iterations run at the level).
// TAPE: the iteration's tape row of batch element b (RGBD_TAPE_WORDS floats at tape + RGBD_TAPE_WORDS b): T before the step (16),
// the 29 sums as reduced (g not yet negated), xi (6), 1 if the step was applied else 0 -- what the reverse pass replays.
constexpr int RGBD_TAPE_WORDS = 64, RGBD_TAPE_SUMS = 16, RGBD_TAPE_XI = 45, RGBD_TAPE_APPLIED = 51;
template <bool TAPE>
__global__ __launch_bounds__(1024) void rgbd_step_k(float *__restrict__ Tall, const float *__restrict__ partials, int nblocks, int prow,
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
    float *rec = TAPE ? tape + RGBD_TAPE_WORDS * b : nullptr;
    if constexpr (TAPE) {
        for (int k = 0; k < 16; ++k) rec[k] = T[k];
        for (int k = 0; k < NACC; ++k) rec[RGBD_TAPE_SUMS + k] = acc[k];
        for (int k = 0; k < 6; ++k) rec[RGBD_TAPE_XI + k] = 0.0f;
        rec[RGBD_TAPE_APPLIED] = 0.0f;
    }
    if (cnt < 6.0f) {
        status |= RGBD_STATUS_FEW;
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
                for (int k = 0; k < 6; ++k) rec[RGBD_TAPE_XI + k] = xi[k];
                rec[RGBD_TAPE_APPLIED] = 1.0f;
            }
            for (int k = 0; k < 16; ++k) T[k] = Tn[k];
        } else {
            status |= RGBD_STATUS_SOLVE;
        }
    }
    row[0] = cnt;
    row[1] = acc[27];
    row[2] = (float)status;
    row[3] = (float)(it + 1);
    for (int k = 0; k < 16; ++k) out_T[16 * b + k] = T[k];
}

// T[b] = out_T[b] = init[b] or the identity; info = 0.  One thread per word.
__global__ __launch_bounds__(256) void rgbd_init_k(const float *__restrict__ init, int B, int n_info, float *__restrict__ Tall,
                                                  float *__restrict__ out_T, float *__restrict__ info) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 16 * B) {
        const float v = init ? init[i] : (((i & 15) % 5 == 0) ? 1.0f : 0.0f);
        Tall[i] = v;
        out_T[i] = v;
    }
    if (i < n_info) info[i] = 0.0f;
}

// ------------------------------------------------------------------ the reverse pass (the rule: include/gradslam_hip.h)
// Per iteration, last to first:
// Xb step reverse, one 256-thread block per batch element: the pixel pass before left 12-sum rows -- the adjoint of T_{k+1}
//    through ITS linearisation -- which are folded (reduce12) into the carried adjoint; then, one lane, fp64 where the forward's
//    fp32 value would lose the gradient: dT-bar = T-bar_{k+1} T_k^T, T-bar_k = dT^T T-bar_{k+1}, the exponential's and the
//    solve's adjoints -> the adjoints of the iteration's 29 sums.  A step that was not applied is the identity.
// Lb pixel reverse, the forward's geometry: the pixel's forward values again from the taped T_k (the same operations: the
//    same decisions), the adjoints of its two rows and residuals from those of the sums, pulled back to q, the eight corner
//    values, the source pixel and T.  <MAX> does all of it but the corner sums, of which it takes the largest magnitude;
//    <ACC> only adds the corner terms into the level's exact fold (gs_fixed128.hpp).  One fold and one finish per level.
// Pb the pyramids' adjoints, coarsest to finest, after all levels: a gather per fine pixel, then level 0 into the images.
constexpr int RGBD_ADJ_WORDS = 32;  // adjoints of the 28 sums AS REDUCED (the six of g: of the sum, not of minus it; cnt has none)
constexpr int RGBD_ADJ_LIVE = 28;   // 1: the pixel pass applies them; 0: a step that was not applied -- nothing, not even 0 x inf
enum { RGBD_BWD_MAX = 0, RGBD_BWD_ACC = 1 };

// out[b] (stride floats, 12 or 16: the bottom row is zero) = gT_in[b] rows 0..2 (NULL: zero) + the sum of b's 12-wide rows
__global__ __launch_bounds__(BWD_T) void rgbd_gT_k(const float *__restrict__ gT_in, const float *__restrict__ partials12, int nblocks,
                                                  int prow, float *__restrict__ out, int stride) {
    __shared__ float sums[12];
    const int b = blockIdx.x;
    reduce12(partials12 + (int64_t)b * prow * 12, nblocks, sums);
    if ((int)threadIdx.x < stride)
        out[stride * b + threadIdx.x] = threadIdx.x < 12 ? (gT_in ? gT_in[16 * b + threadIdx.x] : 0.0f) + sums[threadIdx.x] : 0.0f;
}

// gs_rgbd_rows_bwd: the adjoints of the sums as gs_rgbd_rows returns them (g = MINUS the sum) -> of the sums as reduced; the
// adjoint of cnt is ignored
__global__ __launch_bounds__(256) void rgbd_sums_adj_k(const float *__restrict__ g_sums, int B, float *__restrict__ adj) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * RGBD_ADJ_WORDS) return;
    const int b = i / RGBD_ADJ_WORDS, k = i - b * RGBD_ADJ_WORDS;
    const float g = k < 28 ? g_sums[NACC * b + k] : 0.0f;
    adj[i] = k == RGBD_ADJ_LIVE ? 1.0f : ((k >= 21 && k < 27) ? -g : g);
}

// grid B.  gT (B,16): the carried adjoint of T (rows 0..2), updated in place; rec: this iteration's tape rows; adj: its (B, 32)
__global__ __launch_bounds__(BWD_T) void rgbd_step_bwd_k(float *__restrict__ gTall, const float *__restrict__ partials12, int nblocks,
                                                        int prow, const float *__restrict__ rec_all, float damp,
                                                        float *__restrict__ adj_all) {
    __shared__ float sums[12];
    __shared__ double lu_sm[42];
    __shared__ float g[16], xi[6], dT[16], hg[44], gx[6], y[6];
    __shared__ double gdT[12], gxi[6];
    const int b = blockIdx.x;
    reduce12(partials12 + (int64_t)b * prow * 12, nblocks, sums);
    if (threadIdx.x != 0) return;
    const float *rec = rec_all + RGBD_TAPE_WORDS * b;
    float *gT = gTall + 16 * b, *A = adj_all + RGBD_ADJ_WORDS * b;
    for (int k = 0; k < 16; ++k) g[k] = k < 12 ? gT[k] + sums[k] : 0.0f;
    for (int k = 0; k < RGBD_ADJ_WORDS; ++k) A[k] = 0.0f;
    if (rec[RGBD_TAPE_APPLIED] != 0.0f) {
        for (int k = 0; k < 6; ++k) xi[k] = rec[RGBD_TAPE_XI + k];
        se3_exp_dev(xi, dT);  // the forward's dT, bit for bit
        top3_times_Tt(g, rec, gdT);
        pull_gT(g, dT);
        se3_exp_bwd(xi, gdT, gxi);
        // xi = M^-1 g', M = H + damp I symmetric, g' = MINUS the six sums:  y = M^-1 xi-bar;  H-bar = -y xi^T, g'-bar = y
        expand44(rec + RGBD_TAPE_SUMS, hg);
        for (int k = 0; k < 6; ++k) gx[k] = (float)gxi[k];
        solve6(hg, gx, damp, y, lu_sm);
        int q = 0;
        for (int u = 0; u < 6; ++u)
            for (int v = u; v < 6; ++v) A[q++] = u == v ? -(y[u] * xi[u]) : -(y[u] * xi[v] + y[v] * xi[u]);
        for (int u = 0; u < 6; ++u) A[21 + u] = -y[u];
        A[RGBD_ADJ_LIVE] = 1.0f;
    }
    for (int k = 0; k < 12; ++k) gT[k] = g[k];
}

// One source pixel's forward values, by rgbd_linearize_k's operations in its order (the same bits, so the same decisions).
struct RgbdPix {
    float px, py, d, ux, vy;  // the back-projection: px = d ux, py = d vy
    float qx, qy, qz, iz, a, bb;
    int corner;               // c00's index in the level's image
    float2 c00, c10, c01, c11;
    float Is;
};
__device__ __forceinline__ bool rgbd_pixel_fwd(const float2 *__restrict__ timg, const float2 s, int u, int v, int Hl, int Wl,
                                               const RgbdCam cam, const float *__restrict__ T, float ddm, RgbdPix &P) {
    if (!(s.y > 0.0f)) return false;
    const float d = s.y;
    P.ux = ((float)u - cam.cx) / cam.fx;
    P.vy = ((float)v - cam.cy) / cam.fy;
    const float px = d * P.ux, py = d * P.vy;
    const float qx = ((T[0] * px + T[1] * py) + T[2] * d) + T[3];
    const float qy = ((T[4] * px + T[5] * py) + T[6] * d) + T[7];
    const float qz = ((T[8] * px + T[9] * py) + T[10] * d) + T[11];
    bool ok = qz > 0.0f;
    const float iz = 1.0f / qz;
    const float x = (cam.fx * qx) * iz + cam.cx, y = (cam.fy * qy) * iz + cam.cy;
    const float xf = floorf(x), yf = floorf(y);
    ok = ok && xf >= 0.0f && xf <= (float)(Wl - 2) && yf >= 0.0f && yf <= (float)(Hl - 2);
    if (!ok) return false;
    const int i = (int)xf, j = (int)yf;
    P.corner = j * Wl + i;
    const float2 *c = timg + P.corner;
    P.c00 = c[0]; P.c10 = c[1]; P.c01 = c[Wl]; P.c11 = c[Wl + 1];
    if (!(P.c00.y > 0.0f && P.c10.y > 0.0f && P.c01.y > 0.0f && P.c11.y > 0.0f)) return false;
    P.a = x - xf; P.bb = y - yf;
    const float dX0 = P.c10.y - P.c00.y, dX1 = P.c11.y - P.c01.y;
    const float dTop = P.c00.y + P.a * dX0, dBot = P.c01.y + P.a * dX1;
    const float Dh = dTop + P.bb * (dBot - dTop);
    if (!(fabsf(Dh - qz) <= ddm)) return false;
    P.px = px; P.py = py; P.d = d; P.qx = qx; P.qy = qy; P.qz = qz; P.iz = iz; P.Is = s.x;
    return true;
}

// One channel F (I or D) of a valid pixel: its row J (6) and residual r again, their adjoints from those of the sums (M: the
// symmetric 6 x 6 that J-bar = M J + g r needs, g: the adjoints of the six sums J r, e2 = twice err's), pulled back to the
// four corners cb (00, 10, 01, 11), to q, iz, gx, gy and to the cell coordinates a, b.  `minus`: the other term of the residual
// (I_s or q_z); returns its adjoint.
__device__ __forceinline__ float rgbd_chan_bwd(float F00, float F10, float F01, float F11, float minus, float cz, float w, const RgbdPix &P,
                                               float gx, float gy, const float *__restrict__ M, const float *__restrict__ g, float e2,
                                               float (&cb)[4], float &qxb, float &qyb, float &qzb, float &izb, float &gxb, float &gyb,
                                               float &ab, float &bbb) {
    const float qx = P.qx, qy = P.qy, qz = P.qz, iz = P.iz, a = P.a, bb = P.bb;
    const float X0 = F10 - F00, X1 = F11 - F01;
    const float top = F00 + a * X0, bot = F01 + a * X1;
    const float Fh = top + bb * (bot - top), Fx = X0 + bb * (X1 - X0), Fy = bot - top;
    const float c0 = Fx * gx, c1 = Fy * gy, t = c0 * qx + c1 * qy, c2 = -(t * iz) - cz;
    float J[6] = {w * c0, w * c1, w * c2, w * (qy * c2 - qz * c1), w * (qz * c0 - qx * c2), w * (qx * c1 - qy * c0)};
    const float r = w * (Fh - minus);
    float Jb[6], rb = e2 * r;
#pragma unroll
    for (int u = 0; u < 6; ++u) {
        float v = g[u] * r;
#pragma unroll
        for (int k = 0; k < 6; ++k) v += M[6 * u + k] * J[k];
        Jb[u] = v;
        rb += g[u] * J[u];
    }
    float c0b = w * ((Jb[0] + qz * Jb[4]) - qy * Jb[5]);
    float c1b = w * ((Jb[1] - qz * Jb[3]) + qx * Jb[5]);
    const float c2b = w * ((Jb[2] + qy * Jb[3]) - qx * Jb[4]);
    qxb += w * (c1 * Jb[5] - c2 * Jb[4]);
    qyb += w * (c2 * Jb[3] - c0 * Jb[5]);
    qzb += w * (c0 * Jb[4] - c1 * Jb[3]);
    const float tb = -(c2b * iz);
    izb -= c2b * t;
    c0b += tb * qx; c1b += tb * qy;
    qxb += tb * c0; qyb += tb * c1;
    const float Fxb = c0b * gx, Fyb = c1b * gy, Fhb = w * rb;
    gxb += c0b * Fx; gyb += c1b * Fy;
    const float topb = Fhb * (1.0f - bb) - Fyb, botb = Fhb * bb + Fyb;
    bbb += Fhb * (bot - top) + Fxb * (X1 - X0);  // F_x's b-derivative = F_y's a-derivative: the one second derivative of the cell
    const float X0b = Fxb * (1.0f - bb) + topb * a, X1b = Fxb * bb + botb * a;
    ab += topb * X0 + botb * X1;
    cb[0] = topb - X0b; cb[1] = X0b; cb[2] = botb - X1b; cb[3] = X1b;
    return -Fhb;
}

// grid (blocks of RGBD_T source pixels, B), rgbd_linearize_k's.  T: batch element b's transform at T + tstride b; adj (B, 32).
// MAX: gsrc[pixel] += the source pixel's (I, D) adjoint (its owner lane, in launch order); the block's 12 sums of T's adjoint
// -> partials12 row blockIdx.x; the largest corner term -> the fold.  ACC: the eight corner terms -> the fold's sums (row =
// the target pixel, channel I or D), scaled for at most 2^lg terms per sum.
template <int MODE>
__global__ __launch_bounds__(RGBD_T) void rgbd_pixel_bwd_k(const float2 *__restrict__ tgt, const float2 *__restrict__ src, int Hl, int Wl,
                                                          int level, const float *__restrict__ K, const float *__restrict__ Tall,
                                                          int tstride, const float *__restrict__ adj, float wI, float wD, float ddm,
                                                          Fold fold, int lg, float2 *__restrict__ gsrc, float *__restrict__ partials12,
                                                          int prow) {
    __shared__ float M[36], g[6], e2s;
    const int b = blockIdx.y, npix = Hl * Wl;
    const int p = blockIdx.x * RGBD_T + threadIdx.x;
    const float *__restrict__ A = adj + RGBD_ADJ_WORDS * b;
    if (threadIdx.x < 36) {
        int u = threadIdx.x / 6, v = threadIdx.x % 6;
        const bool diag = u == v;
        if (u > v) { const int t = u; u = v; v = t; }
        const float s = A[u * 6 - (u * (u - 1)) / 2 + (v - u)];
        M[threadIdx.x] = diag ? 2.0f * s : s;
    } else if (threadIdx.x < 42) {
        g[threadIdx.x - 36] = A[21 + (threadIdx.x - 36)];
    } else if (threadIdx.x == 42) {
        e2s = 2.0f * A[27];
    }
    __syncthreads();
    const RgbdCam cam = rgbd_cam(K + 16 * b, level);
    const float *__restrict__ T = Tall + (int64_t)tstride * b;
    const float2 *__restrict__ timg = tgt + (int64_t)b * npix;
    RgbdPix P;
    bool ok = false;
    if (p < npix && A[RGBD_ADJ_LIVE] != 0.0f) {
        const int v = p / Wl, u = p - v * Wl;
        ok = rgbd_pixel_fwd(timg, src[(int64_t)b * npix + p], u, v, Hl, Wl, cam, T, ddm, P);
    }
    float acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.0f;
    uint32_t mx = 0;
    const int E = MODE == RGBD_BWD_ACC ? det_scale(*fold.maxbits, lg) : 0;
    if (ok) {
        const float gx = cam.fx * P.iz, gy = cam.fy * P.iz;
        float cI[4], cD[4], qxb = 0.0f, qyb = 0.0f, qzb = 0.0f, izb = 0.0f, gxb = 0.0f, gyb = 0.0f, ab = 0.0f, bbb = 0.0f;
        const float Isb = rgbd_chan_bwd(P.c00.x, P.c10.x, P.c01.x, P.c11.x, P.Is, 0.0f, wI, P, gx, gy, M, g, e2s, cI, qxb, qyb, qzb, izb, gxb,
                                        gyb, ab, bbb);
        const float qzr = rgbd_chan_bwd(P.c00.y, P.c10.y, P.c01.y, P.c11.y, P.qz, 1.0f, wD, P, gx, gy, M, g, e2s, cD, qxb, qyb, qzb, izb, gxb,
                                        gyb, ab, bbb);
        qzb += qzr;  // r_D = w_D (D^ - q_z)
        if (MODE == RGBD_BWD_ACC) {
            const int64_t row = (int64_t)b * npix + P.corner;
            const int64_t rows[4] = {row, row + 1, row + Wl, row + Wl + 1};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                fold_add(fold, rows[k], 0, cI[k], E);
                fold_add(fold, rows[k], 1, cD[k], E);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) mx = fold_max(fold_max(mx, cI[k]), cD[k]);
            // x = (fx q_x) iz + cx, y likewise; gx = fx iz, gy = fy iz; iz = 1 / q_z
            izb += cam.fx * gxb + cam.fy * gyb;
            qxb += ab * gx; izb += ab * (cam.fx * P.qx);
            qyb += bbb * gy; izb += bbb * (cam.fy * P.qy);
            qzb -= (izb * P.iz) * P.iz;
            // q = T (px, py, d, 1)
            acc[0] = qxb * P.px; acc[1] = qxb * P.py; acc[2] = qxb * P.d; acc[3] = qxb;
            acc[4] = qyb * P.px; acc[5] = qyb * P.py; acc[6] = qyb * P.d; acc[7] = qyb;
            acc[8] = qzb * P.px; acc[9] = qzb * P.py; acc[10] = qzb * P.d; acc[11] = qzb;
            const float pxb = (T[0] * qxb + T[4] * qyb) + T[8] * qzb, pyb = (T[1] * qxb + T[5] * qyb) + T[9] * qzb;
            const float db = (((T[2] * qxb + T[6] * qyb) + T[10] * qzb) + pxb * P.ux) + pyb * P.vy;
            float2 *o = gsrc + (int64_t)b * npix + p;
            const float2 old = *o;
            *o = make_float2(old.x + Isb, old.y + db);
        }
    }
    if (MODE == RGBD_BWD_MAX) {
        // The fold's maximum only grows, so a term no larger than a value it has held needs no atomic: after the first blocks
        // almost none is issued (thousands of waves, one address).  The maximum is the same whichever are skipped.
        if (mx <= __hip_atomic_load(fold.maxbits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) mx = 0;
        fold_max_commit(fold.maxbits, mx);
        block_store12(acc, partials12 + (int64_t)b * prow * 12);
    }
}

// the level's target adjoint from its fold: n = B npix rows, two channels
__global__ __launch_bounds__(256) void rgbd_fold_finish_k(Fold fold, int lg, int64_t n, float2 *__restrict__ gtgt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int E = det_scale(*fold.maxbits, lg);
    gtgt[i] = make_float2(fold_result(fold, i, 0, E), fold_result(fold, i, 1, E));
}

// rgbd_down_k's adjoint as a gather: fine pixel p of (B, Hp, Wp) belongs to one coarse pixel (none in an odd last row or column);
// gin[p] += (0.25 I-bar, D-bar / n where the fine depth was taken).  grid (blocks of 256 fine pixels, B)
__global__ __launch_bounds__(256) void rgbd_down_bwd_k(const float2 *__restrict__ in, int Hp, int Wp, int Hl, int Wl, float ddm,
                                                      const float2 *__restrict__ gout, float2 *__restrict__ gin) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= Hp * Wp) return;
    const int v = p / Wp, u = p - v * Wp, cv = v >> 1, cu = u >> 1;
    if (cv >= Hl || cu >= Wl) return;
    const float2 *src = in + (int64_t)blockIdx.y * Hp * Wp + (int64_t)(2 * cv) * Wp + 2 * cu;
    const float2 c[4] = {src[0], src[1], src[Wp], src[Wp + 1]};
    float dmin = INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k) dmin = (c[k].y > 0.0f && c[k].y < dmin) ? c[k].y : dmin;
    int n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (c[k].y > 0.0f && c[k].y - dmin <= ddm) ++n;
    const float mine = (v & 1) ? ((u & 1) ? c[3].y : c[2].y) : ((u & 1) ? c[1].y : c[0].y);
    const float2 go = gout[(int64_t)blockIdx.y * Hl * Wl + (int64_t)cv * Wl + cu];
    const bool taken = mine > 0.0f && mine - dmin <= ddm;
    float2 *o = gin + (int64_t)blockIdx.y * Hp * Wp + p;
    const float2 old = *o;
    *o = make_float2(old.x + 0.25f * go.x, old.y + (taken ? go.y / (float)n : 0.0f));
}

// rgbd_level0_k's adjoint: the luma weights times rgb_scale into rgb, the depth's where the depth was kept; either may be NULL
__global__ __launch_bounds__(256) void rgbd_level0_bwd_k(const float *__restrict__ depth, const float2 *__restrict__ g, int64_t n,
                                                        float rgb_scale, float *__restrict__ g_depth, float *__restrict__ g_rgb) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float2 gi = g[i];
    if (g_rgb) {
        const float s = rgb_scale * gi.x;
        g_rgb[3 * i] = 0.299f * s;
        g_rgb[3 * i + 1] = 0.587f * s;
        g_rgb[3 * i + 2] = 0.114f * s;
    }
    if (g_depth) {
        const float d = depth[i];
        g_depth[i] = (d > 0.0f && d < INFINITY) ? gi.y : 0.0f;
    }
}

// ------------------------------------------------------------------ host
struct RgbdWs {
    float *T;         // B x 16
    float *partials;  // B x prow x NACC
    float2 *tgt, *src;  // level-major pyramids: level l at + B * off[l] pixels
    int prow;
    int Hl[RGBD_MAX_LEVELS], Wl[RGBD_MAX_LEVELS];
    int64_t off[RGBD_MAX_LEVELS + 1];  // pixels per batch element in the levels before l
};
static size_t rgbd_layout(int B, int H, int W, int levels, void *ws, RgbdWs *w) {
    Carve c{(char *)ws};
    RgbdWs t;
    t.off[0] = 0;
    for (int l = 0; l < levels; ++l) {
        t.Hl[l] = H >> l;
        t.Wl[l] = W >> l;
        t.off[l + 1] = t.off[l] + (int64_t)t.Hl[l] * t.Wl[l];
    }
    t.prow = cdiv((int64_t)H * W, RGBD_T);
    t.T = c.take<float>(sizeof(float) * 16 * B);
    t.partials = c.take<float>(sizeof(float) * NACC * (size_t)t.prow * B);
    t.tgt = c.take<float2>(sizeof(float2) * (size_t)t.off[levels] * B);
    t.src = c.take<float2>(sizeof(float2) * (size_t)t.off[levels] * B);
    if (w) *w = t;
    return c.off;
}
static bool rgbd_shape_ok(int B, int H, int W, int levels) {
    return B >= 1 && B <= 65535 && levels >= 1 && levels <= RGBD_MAX_LEVELS && H >= 1 && W >= 1 && (int64_t)H * W <= (1 << 24) &&
           (int64_t)B * H * W <= (1 << 30) && (H >> (levels - 1)) >= RGBD_MIN_SIDE && (W >> (levels - 1)) >= RGBD_MIN_SIDE;
}
#define RGBD_REQUIRE_SHAPE(name)                                                                                                  \
    do {                                                                                                                          \
        GS_REQUIRE(B >= 1 && B <= 65535, name ": B must be in [1, 65535], got %d", B);                                            \
        GS_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= (1 << 24), name ": H x W must be positive and at most 2^24 pixels, got %d x %d", H, W); \
        GS_REQUIRE((int64_t)B * H * W <= (1 << 30), name ": B H W must be at most 2^30, got %d x %d x %d", B, H, W);              \
        GS_REQUIRE(levels >= 1 && levels <= RGBD_MAX_LEVELS, name ": levels must be in [1, %d], got %d", RGBD_MAX_LEVELS, levels); \
        GS_REQUIRE((H >> (levels - 1)) >= RGBD_MIN_SIDE && (W >> (levels - 1)) >= RGBD_MIN_SIDE,                                  \
                   name ": the coarsest of %d levels of a %d x %d image would be smaller than 4 x 4", levels, H, W);               \
    } while (0)
#define RGBD_REQUIRE_PARAMS(name)                                                                                                 \
    do {                                                                                                                          \
        GS_REQUIRE(depth_diff_max > 0.0f && depth_diff_max < INFINITY, name ": depth_diff_max must be finite and positive, got %g", (double)depth_diff_max); \
        GS_REQUIRE(fabsf(rgb_scale) < INFINITY, name ": rgb_scale must be finite, got %g", (double)rgb_scale);                     \
    } while (0)
#define RGBD_REQUIRE_LAMBDA(name) \
    GS_REQUIRE(lambda_geo >= 0.0f && lambda_geo <= 1.0f, name ": lambda_geo must be in [0, 1], got %g", (double)lambda_geo)

// the pyramid of one frame into `pyr` (level-major, level l at + B * off[l])
static int rgbd_build_pyramid(const char *name, const float *depth, const float *rgb, int B, int levels, const RgbdWs &w, float ddm,
                              float rgb_scale, float2 *pyr, hipStream_t st) {
    const int64_t n0 = (int64_t)B * w.Hl[0] * w.Wl[0];
    hipLaunchKernelGGL(rgbd_level0_k, dim3(cdiv(n0, 256)), dim3(256), 0, st, depth, rgb, n0, rgb_scale, pyr);
    GS_LAUNCH_CHECK(name);
    for (int l = 1; l < levels; ++l) {
        hipLaunchKernelGGL(rgbd_down_k, dim3(cdiv((int64_t)w.Hl[l] * w.Wl[l], 256), B), dim3(256), 0, st, pyr + B * w.off[l - 1],
                           w.Hl[l - 1], w.Wl[l - 1], w.Hl[l], w.Wl[l], ddm, pyr + B * w.off[l]);
        GS_LAUNCH_CHECK(name);
    }
    return 0;
}


// the reverse pass's workspace: the forward's pyramids again (f: its sizes and offsets; f.T and f.partials are not carved)
struct RgbdBwdWs {
    RgbdWs f;
    float *gT;          // B x 16: the carried adjoint of T
    float *adj;         // max(iterations, 1) x B x RGBD_ADJ_WORDS, in the order the iterations ran
    float *partials12;  // B x prow x 12
    float2 *gtgt, *gsrc;  // the pyramids' adjoints, the forward's layout, one piece (adj_pyr_bytes)
    size_t adj_pyr_bytes;
    Fold fold;          // B H W rows x 2 channels; a coarser level uses its first rows
    void *fold_base;
    size_t fold_bytes;
};
static size_t rgbd_bwd_layout(int B, int H, int W, int levels, int64_t iterations, void *ws, RgbdBwdWs *out) {
    Carve c{(char *)ws};
    RgbdBwdWs t;
    rgbd_layout(B, H, W, levels, nullptr, &t.f);
    t.f.T = nullptr;
    t.f.partials = nullptr;
    const size_t pyr = sizeof(float2) * (size_t)t.f.off[levels] * B;
    t.gT = c.take<float>(sizeof(float) * 16 * B);
    t.adj = c.take<float>(sizeof(float) * RGBD_ADJ_WORDS * (size_t)std::max<int64_t>(iterations, 1) * B);
    t.partials12 = c.take<float>(sizeof(float) * 12 * (size_t)t.f.prow * B);
    t.f.tgt = c.take<float2>(pyr);
    t.f.src = c.take<float2>(pyr);
    t.adj_pyr_bytes = 2 * pyr;
    t.gtgt = c.take<float2>(t.adj_pyr_bytes);
    t.gsrc = t.gtgt ? t.gtgt + (size_t)t.f.off[levels] * B : nullptr;
    const size_t before = c.off;
    t.fold = fold_carve(c, (size_t)B * H * W, 2);
    t.fold_base = t.fold.maxbits;
    t.fold_bytes = c.off - before;
    if (out) *out = t;
    return c.off;
}

}  // namespace gs

using namespace gs;

extern "C" {

size_t gs_rgbd_odometry_ws_bytes(int B, int H, int W, int levels) {
    if (!rgbd_shape_ok(B, H, W, levels)) return 0;
    return rgbd_layout(B, H, W, levels, nullptr, nullptr);
}

int gs_rgbd_pyramid(const float *depth, const float *rgb, int B, int H, int W, int levels, float depth_diff_max, float rgb_scale,
                    float *out, gs_stream_t stream) {
    GS_REQUIRE(depth && rgb && out, "gs_rgbd_pyramid: null pointer");
    RGBD_REQUIRE_SHAPE("gs_rgbd_pyramid");
    RGBD_REQUIRE_PARAMS("gs_rgbd_pyramid");
    RgbdWs w;
    rgbd_layout(B, H, W, levels, nullptr, &w);
    return rgbd_build_pyramid("gs_rgbd_pyramid", depth, rgb, B, levels, w, depth_diff_max, rgb_scale, (float2 *)out, (hipStream_t)stream);
}

int gs_rgbd_rows(const float *tgt_depth, const float *tgt_rgb, const float *src_depth, const float *src_rgb, int B, int H, int W,
                 const float *intrinsics, const float *T, float lambda_geo, float depth_diff_max, float rgb_scale, int32_t *valid,
                 float *rows, float *sums, void *ws, size_t ws_bytes, gs_stream_t stream) {
    GS_REQUIRE(tgt_depth && tgt_rgb && src_depth && src_rgb && intrinsics && T && valid && rows && sums, "gs_rgbd_rows: null pointer");
    const int levels = 1;
    RGBD_REQUIRE_SHAPE("gs_rgbd_rows");
    RGBD_REQUIRE_LAMBDA("gs_rgbd_rows");
    RGBD_REQUIRE_PARAMS("gs_rgbd_rows");
    const size_t need = gs_rgbd_odometry_ws_bytes(B, H, W, levels);
    GS_REQUIRE_WS("gs_rgbd_rows", ws, ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    RgbdWs w;
    rgbd_layout(B, H, W, levels, ws, &w);
    int rc = rgbd_build_pyramid("gs_rgbd_rows/pyramid", tgt_depth, tgt_rgb, B, levels, w, depth_diff_max, rgb_scale, w.tgt, st);
    if (rc) return rc;
    rc = rgbd_build_pyramid("gs_rgbd_rows/pyramid", src_depth, src_rgb, B, levels, w, depth_diff_max, rgb_scale, w.src, st);
    if (rc) return rc;
    const float wI = sqrtf(1.0f - lambda_geo), wD = sqrtf(lambda_geo);
    hipLaunchKernelGGL(rgbd_linearize_k<true>, dim3(w.prow, B), dim3(RGBD_T), 0, st, w.tgt, w.src, H, W, 0, intrinsics, T, wI, wD,
                       depth_diff_max, w.partials, w.prow, valid, rows);
    GS_LAUNCH_CHECK("gs_rgbd_rows/linearize");
    hipLaunchKernelGGL(rgbd_step_k<false>, dim3(B), dim3(1024), 0, st, w.T, w.partials, w.prow, w.prow, 0.0f, 0, 1, 0, 0, (float *)nullptr,
                       (float *)nullptr, sums, (float *)nullptr);
    GS_LAUNCH_CHECK("gs_rgbd_rows/sums");
    return 0;
}

}  // extern "C"

// gs_rgbd_odometry (tape = NULL) and gs_rgbd_odometry_taped: one loop, the same launches
static int rgbd_run(const float *tgt_depth, const float *tgt_rgb, const float *src_depth, const float *src_rgb, int B, int H, int W,
                    const float *intrinsics, const float *init, int levels, const int *numiters, float lambda_geo, float depth_diff_max,
                    float damp, float rgb_scale, float *out_T, float *info, void *ws, size_t ws_bytes, gs_stream_t stream, float *tape) {
    const size_t need = gs_rgbd_odometry_ws_bytes(B, H, W, levels);
    GS_REQUIRE_WS(tape ? "gs_rgbd_odometry_taped" : "gs_rgbd_odometry", ws, ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    RgbdWs w;
    rgbd_layout(B, H, W, levels, ws, &w);
    const int n_info = B * levels * 4;
    hipLaunchKernelGGL(rgbd_init_k, dim3(cdiv(std::max(16 * B, n_info), 256)), dim3(256), 0, st, init, B, n_info, w.T, out_T, info);
    GS_LAUNCH_CHECK("gs_rgbd_odometry/init");
    int rc = rgbd_build_pyramid("gs_rgbd_odometry/pyramid", tgt_depth, tgt_rgb, B, levels, w, depth_diff_max, rgb_scale, w.tgt, st);
    if (rc) return rc;
    rc = rgbd_build_pyramid("gs_rgbd_odometry/pyramid", src_depth, src_rgb, B, levels, w, depth_diff_max, rgb_scale, w.src, st);
    if (rc) return rc;
    const float wI = sqrtf(1.0f - lambda_geo), wD = sqrtf(lambda_geo);
    float *rec = tape;  // one row per (iteration, batch element), in the order the iterations run
    for (int l = levels - 1; l >= 0; --l) {
        const int nblocks = cdiv((int64_t)w.Hl[l] * w.Wl[l], RGBD_T);
        for (int it = 0; it < numiters[l]; ++it) {
            hipLaunchKernelGGL(rgbd_linearize_k<false>, dim3(nblocks, B), dim3(RGBD_T), 0, st, w.tgt + B * w.off[l], w.src + B * w.off[l],
                               w.Hl[l], w.Wl[l], l, intrinsics, w.T, wI, wD, depth_diff_max, w.partials, w.prow, (int32_t *)nullptr,
                               (float *)nullptr);
            GS_LAUNCH_CHECK("gs_rgbd_odometry/linearize");
            if (tape) {
                hipLaunchKernelGGL(rgbd_step_k<true>, dim3(B), dim3(1024), 0, st, w.T, w.partials, nblocks, w.prow, damp, l, levels, it, 1,
                                   out_T, info, (float *)nullptr, rec);
                rec += (size_t)RGBD_TAPE_WORDS * B;
            } else {
                hipLaunchKernelGGL(rgbd_step_k<false>, dim3(B), dim3(1024), 0, st, w.T, w.partials, nblocks, w.prow, damp, l, levels, it, 1,
                                   out_T, info, (float *)nullptr, (float *)nullptr);
            }
            GS_LAUNCH_CHECK("gs_rgbd_odometry/step");
        }
    }
    return 0;
}

// the reverse pass of the loop: rgbd_backward_run.  `T`: (B, tstride) floats, batch element b's transform at T + tstride b (a tape
// row or a plain (B,16)); `adj`: (B, RGBD_ADJ_WORDS) adjoints of the 29 sums.
static int rgbd_pixel_bwd_launch(const char *name, int mode, const RgbdBwdWs &w, int B, int l, const float *K, const float *T, int tstride,
                                 const float *adj, float wI, float wD, float ddm, int lg, hipStream_t st) {
    const int nblocks = cdiv((int64_t)w.f.Hl[l] * w.f.Wl[l], RGBD_T);
    const float2 *tgt = w.f.tgt + B * w.f.off[l], *src = w.f.src + B * w.f.off[l];
    float2 *gsrc = w.gsrc + B * w.f.off[l];
    if (mode == RGBD_BWD_MAX)
        hipLaunchKernelGGL(rgbd_pixel_bwd_k<RGBD_BWD_MAX>, dim3(nblocks, B), dim3(RGBD_T), 0, st, tgt, src, w.f.Hl[l], w.f.Wl[l], l, K, T, tstride,
                           adj, wI, wD, ddm, w.fold, lg, gsrc, w.partials12, w.f.prow);
    else
        hipLaunchKernelGGL(rgbd_pixel_bwd_k<RGBD_BWD_ACC>, dim3(nblocks, B), dim3(RGBD_T), 0, st, tgt, src, w.f.Hl[l], w.f.Wl[l], l, K, T, tstride,
                           adj, wI, wD, ddm, w.fold, lg, gsrc, w.partials12, w.f.prow);
    GS_LAUNCH_CHECK(name);
    return 0;
}
static int rgbd_fold_finish_launch(const char *name, const RgbdBwdWs &w, int B, int l, int lg, hipStream_t st) {
    const int64_t n = (int64_t)B * w.f.Hl[l] * w.f.Wl[l];
    hipLaunchKernelGGL(rgbd_fold_finish_k, dim3(cdiv(n, 256)), dim3(256), 0, st, w.fold, lg, n, w.gtgt + B * w.f.off[l]);
    GS_LAUNCH_CHECK(name);
    return 0;
}
// both pyramids (rebuilt: the forward's workspace need not have survived), the adjoint pyramids zeroed
static int rgbd_bwd_prepare(const char *name, const float *tgt_depth, const float *tgt_rgb, const float *src_depth, const float *src_rgb,
                            int B, int levels, const RgbdBwdWs &w, float ddm, float rgb_scale, hipStream_t st) {
    int rc = rgbd_build_pyramid(name, tgt_depth, tgt_rgb, B, levels, w.f, ddm, rgb_scale, w.f.tgt, st);
    if (rc) return rc;
    rc = rgbd_build_pyramid(name, src_depth, src_rgb, B, levels, w.f, ddm, rgb_scale, w.f.src, st);
    if (rc) return rc;
    GS_HIP(hipMemsetAsync(w.gtgt, 0, w.adj_pyr_bytes, st), name);  // gtgt | gsrc
    return 0;
}
// the adjoint pyramids, coarsest to finest, then level 0 into the images; any of the four may be NULL
static int rgbd_pyramid_bwd(const char *name, const float *depth, const float2 *pyr, float2 *gpyr, int B, int levels, const RgbdWs &f,
                            float ddm, float rgb_scale, float *g_depth, float *g_rgb, hipStream_t st) {
    if (!g_depth && !g_rgb) return 0;
    for (int l = levels - 1; l >= 1; --l) {
        hipLaunchKernelGGL(rgbd_down_bwd_k, dim3(cdiv((int64_t)f.Hl[l - 1] * f.Wl[l - 1], 256), B), dim3(256), 0, st, pyr + B * f.off[l - 1],
                           f.Hl[l - 1], f.Wl[l - 1], f.Hl[l], f.Wl[l], ddm, gpyr + B * f.off[l], gpyr + B * f.off[l - 1]);
        GS_LAUNCH_CHECK(name);
    }
    const int64_t n0 = (int64_t)B * f.Hl[0] * f.Wl[0];
    hipLaunchKernelGGL(rgbd_level0_bwd_k, dim3(cdiv(n0, 256)), dim3(256), 0, st, depth, gpyr, n0, rgb_scale, g_depth, g_rgb);
    GS_LAUNCH_CHECK(name);
    return 0;
}

extern "C" {

#define RGBD_REQUIRE_ODOMETRY(name)                                                                                               \
    do {                                                                                                                          \
        RGBD_REQUIRE_SHAPE(name);                                                                                                 \
        RGBD_REQUIRE_LAMBDA(name);                                                                                                \
        RGBD_REQUIRE_PARAMS(name);                                                                                                \
        GS_REQUIRE(damp >= 0.0f && damp < INFINITY, name ": damp must be finite and not negative, got %g", (double)damp);         \
        for (int l = 0; l < levels; ++l)                                                                                          \
            GS_REQUIRE(numiters[l] >= 0 && numiters[l] <= (1 << 20), name ": numiters[%d] must be in [0, 2^20], got %d", l, numiters[l]); \
    } while (0)

int gs_rgbd_odometry(const float *tgt_depth, const float *tgt_rgb, const float *src_depth, const float *src_rgb, int B, int H, int W,
                     const float *intrinsics, const float *init, int levels, const int *numiters, float lambda_geo,
                     float depth_diff_max, float damp, float rgb_scale, float *out_T, float *info, void *ws, size_t ws_bytes,
                     gs_stream_t stream) {
    GS_REQUIRE(tgt_depth && tgt_rgb && src_depth && src_rgb && intrinsics && numiters && out_T && info, "gs_rgbd_odometry: null pointer");
    RGBD_REQUIRE_ODOMETRY("gs_rgbd_odometry");
    return rgbd_run(tgt_depth, tgt_rgb, src_depth, src_rgb, B, H, W, intrinsics, init, levels, numiters, lambda_geo, depth_diff_max, damp,
                    rgb_scale, out_T, info, ws, ws_bytes, stream, nullptr);
}

// (numiters here: the SUM of the levels' counts)
size_t gs_rgbd_odometry_tape_size(int B, int levels, int numiters) {
    if (B < 1 || B > 65535 || levels < 1 || levels > RGBD_MAX_LEVELS || numiters < 0 || numiters > levels * (1 << 20)) return 0;
    return one_piece_bytes(sizeof(float) * RGBD_TAPE_WORDS * (size_t)std::max(numiters, 1) * B);
}

int gs_rgbd_odometry_taped(const float *tgt_depth, const float *tgt_rgb, const float *src_depth, const float *src_rgb, int B, int H,
                           int W, const float *intrinsics, const float *init, int levels, const int *numiters, float lambda_geo,
                           float depth_diff_max, float damp, float rgb_scale, float *out_T, float *info, void *ws, size_t ws_bytes,
                           gs_stream_t stream, float *tape) {
    GS_REQUIRE(tgt_depth && tgt_rgb && src_depth && src_rgb && intrinsics && numiters && out_T && info && tape,
               "gs_rgbd_odometry_taped: null pointer");
    RGBD_REQUIRE_ODOMETRY("gs_rgbd_odometry_taped");
    return rgbd_run(tgt_depth, tgt_rgb, src_depth, src_rgb, B, H, W, intrinsics, init, levels, numiters, lambda_geo, depth_diff_max, damp,
                    rgb_scale, out_T, info, ws, ws_bytes, stream, tape);
}

size_t gs_rgbd_odometry_bwd_ws_size(int B, int H, int W, int levels, int numiters) {
    if (!rgbd_shape_ok(B, H, W, levels) || numiters < 0 || numiters > levels * (1 << 20)) return 0;
    return rgbd_bwd_layout(B, H, W, levels, numiters, nullptr, nullptr);
}

int gs_rgbd_odometry_bwd(const float *tgt_depth, const float *tgt_rgb, const float *src_depth, const float *src_rgb, int B, int H, int W,
                         const float *intrinsics, int levels, const int *numiters, float lambda_geo, float depth_diff_max, float damp,
                         float rgb_scale, const float *tape, const float *grad_T, float *g_tgt_depth, float *g_tgt_rgb, float *g_src_depth,
                         float *g_src_rgb, float *g_init, void *ws, size_t ws_bytes, gs_stream_t stream) {
    GS_REQUIRE(tgt_depth && tgt_rgb && src_depth && src_rgb && intrinsics && numiters && tape && grad_T, "gs_rgbd_odometry_bwd: null pointer");
    RGBD_REQUIRE_ODOMETRY("gs_rgbd_odometry_bwd");
    int total = 0, base[RGBD_MAX_LEVELS];  // base[l]: iterations that ran before level l's (the coarser levels')
    for (int l = levels - 1; l >= 0; --l) { base[l] = total; total += numiters[l]; }
    const size_t need = gs_rgbd_odometry_bwd_ws_size(B, H, W, levels, total);
    GS_REQUIRE_WS("gs_rgbd_odometry_bwd", ws, ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    RgbdBwdWs w;
    rgbd_bwd_layout(B, H, W, levels, total, ws, &w);
    int rc = rgbd_bwd_prepare("gs_rgbd_odometry_bwd/pyramid", tgt_depth, tgt_rgb, src_depth, src_rgb, B, levels, w, depth_diff_max, rgb_scale, st);
    if (rc) return rc;
    hipLaunchKernelGGL(rgbd_gT_k, dim3(B), dim3(BWD_T), 0, st, grad_T, (const float *)nullptr, 0, w.f.prow, w.gT, 16);
    GS_LAUNCH_CHECK("gs_rgbd_odometry_bwd/begin");
    const float wI = sqrtf(1.0f - lambda_geo), wD = sqrtf(lambda_geo);
    int prev_nblocks = 0;  // rows the pixel pass before left for the next step's fold
    // without a target gradient nothing reads the corner sums: no fold (only its maximum's word, which <MAX> touches, is zeroed)
    const bool want_tgt = g_tgt_depth || g_tgt_rgb;
    for (int l = 0; l < levels; ++l) {
        const int n = numiters[l];
        if (n == 0) continue;
        const int nblocks = cdiv((int64_t)w.f.Hl[l] * w.f.Wl[l], RGBD_T);
        const int lg = fold_lg((int64_t)w.f.Hl[l] * w.f.Wl[l] * n);  // a corner receives at most one term per source pixel and iteration
        GS_HIP(hipMemsetAsync(w.fold_base, 0, want_tgt ? w.fold_bytes : sizeof(uint32_t), st), "gs_rgbd_odometry_bwd/zero");
        for (int it = n - 1; it >= 0; --it) {
            const float *rec = tape + (size_t)(base[l] + it) * B * RGBD_TAPE_WORDS;
            float *adj = w.adj + (size_t)(base[l] + it) * B * RGBD_ADJ_WORDS;
            hipLaunchKernelGGL(rgbd_step_bwd_k, dim3(B), dim3(BWD_T), 0, st, w.gT, w.partials12, prev_nblocks, w.f.prow, rec, damp, adj);
            GS_LAUNCH_CHECK("gs_rgbd_odometry_bwd/step");
            rc = rgbd_pixel_bwd_launch("gs_rgbd_odometry_bwd/pixels", RGBD_BWD_MAX, w, B, l, intrinsics, rec, RGBD_TAPE_WORDS, adj, wI, wD,
                                       depth_diff_max, lg, st);
            if (rc) return rc;
            prev_nblocks = nblocks;
        }
        if (!want_tgt) continue;
        for (int it = n - 1; it >= 0; --it) {
            rc = rgbd_pixel_bwd_launch("gs_rgbd_odometry_bwd/corners", RGBD_BWD_ACC, w, B, l, intrinsics,
                                       tape + (size_t)(base[l] + it) * B * RGBD_TAPE_WORDS, RGBD_TAPE_WORDS,
                                       w.adj + (size_t)(base[l] + it) * B * RGBD_ADJ_WORDS, wI, wD, depth_diff_max, lg, st);
            if (rc) return rc;
        }
        rc = rgbd_fold_finish_launch("gs_rgbd_odometry_bwd/finish", w, B, l, lg, st);
        if (rc) return rc;
    }
    if (g_init) {
        hipLaunchKernelGGL(rgbd_gT_k, dim3(B), dim3(BWD_T), 0, st, (const float *)w.gT, (const float *)w.partials12, prev_nblocks, w.f.prow,
                           g_init, 16);
        GS_LAUNCH_CHECK("gs_rgbd_odometry_bwd/init");
    }
    rc = rgbd_pyramid_bwd("gs_rgbd_odometry_bwd/target", tgt_depth, w.f.tgt, w.gtgt, B, levels, w.f, depth_diff_max, rgb_scale, g_tgt_depth,
                          g_tgt_rgb, st);
    if (rc) return rc;
    return rgbd_pyramid_bwd("gs_rgbd_odometry_bwd/source", src_depth, w.f.src, w.gsrc, B, levels, w.f, depth_diff_max, rgb_scale, g_src_depth,
                            g_src_rgb, st);
}

int gs_rgbd_rows_bwd(const float *tgt_depth, const float *tgt_rgb, const float *src_depth, const float *src_rgb, int B, int H, int W,
                     const float *intrinsics, const float *T, float lambda_geo, float depth_diff_max, float rgb_scale, const float *g_sums,
                     float *g_tgt_depth, float *g_tgt_rgb, float *g_src_depth, float *g_src_rgb, float *g_T, void *ws, size_t ws_bytes,
                     gs_stream_t stream) {
    GS_REQUIRE(tgt_depth && tgt_rgb && src_depth && src_rgb && intrinsics && T && g_sums, "gs_rgbd_rows_bwd: null pointer");
    const int levels = 1;
    RGBD_REQUIRE_SHAPE("gs_rgbd_rows_bwd");
    RGBD_REQUIRE_LAMBDA("gs_rgbd_rows_bwd");
    RGBD_REQUIRE_PARAMS("gs_rgbd_rows_bwd");
    const size_t need = gs_rgbd_odometry_bwd_ws_size(B, H, W, levels, 1);
    GS_REQUIRE_WS("gs_rgbd_rows_bwd", ws, ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    RgbdBwdWs w;
    rgbd_bwd_layout(B, H, W, levels, 1, ws, &w);
    int rc = rgbd_bwd_prepare("gs_rgbd_rows_bwd/pyramid", tgt_depth, tgt_rgb, src_depth, src_rgb, B, levels, w, depth_diff_max, rgb_scale, st);
    if (rc) return rc;
    const bool want_tgt = g_tgt_depth || g_tgt_rgb;  // (as in gs_rgbd_odometry_bwd)
    GS_HIP(hipMemsetAsync(w.fold_base, 0, want_tgt ? w.fold_bytes : sizeof(uint32_t), st), "gs_rgbd_rows_bwd/zero");
    hipLaunchKernelGGL(rgbd_sums_adj_k, dim3(cdiv((int64_t)B * RGBD_ADJ_WORDS, 256)), dim3(256), 0, st, g_sums, B, w.adj);
    GS_LAUNCH_CHECK("gs_rgbd_rows_bwd/adjoints");
    const float wI = sqrtf(1.0f - lambda_geo), wD = sqrtf(lambda_geo);
    const int lg = fold_lg((int64_t)H * W);
    rc = rgbd_pixel_bwd_launch("gs_rgbd_rows_bwd/pixels", RGBD_BWD_MAX, w, B, 0, intrinsics, T, 16, w.adj, wI, wD, depth_diff_max, lg, st);
    if (rc) return rc;
    if (want_tgt) {
        rc = rgbd_pixel_bwd_launch("gs_rgbd_rows_bwd/corners", RGBD_BWD_ACC, w, B, 0, intrinsics, T, 16, w.adj, wI, wD, depth_diff_max, lg, st);
        if (rc) return rc;
        rc = rgbd_fold_finish_launch("gs_rgbd_rows_bwd/finish", w, B, 0, lg, st);
        if (rc) return rc;
    }
    if (g_T) {
        hipLaunchKernelGGL(rgbd_gT_k, dim3(B), dim3(BWD_T), 0, st, (const float *)nullptr, (const float *)w.partials12, w.f.prow, w.f.prow, g_T, 12);
        GS_LAUNCH_CHECK("gs_rgbd_rows_bwd/transform");
    }
    rc = rgbd_pyramid_bwd("gs_rgbd_rows_bwd/target", tgt_depth, w.f.tgt, w.gtgt, B, levels, w.f, depth_diff_max, rgb_scale, g_tgt_depth,
                          g_tgt_rgb, st);
    if (rc) return rc;
    return rgbd_pyramid_bwd("gs_rgbd_rows_bwd/source", src_depth, w.f.src, w.gsrc, B, levels, w.f, depth_diff_max, rgb_scale, g_src_depth,
                            g_src_rgb, st);
}

}  // extern "C"
