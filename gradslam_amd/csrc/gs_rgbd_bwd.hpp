// gs_rgbd_bwd.hpp -- the dense RGB-D odometry's own kernels of its reverse pass (the rule: include/gradslam_hip.h).  Included by
// rgbd.hip, which launches them (rgbd_bwd_run); the pixel's forward values and the pyramid's rules are gs_rgbd_pixel.hpp's, the
// forward's own code.  The step reverse, the fold of the 12-wide rows, the seam's adjoint row and the layouts of the tape row
// (GN_TAPE_*) and of the adjoint row (GN_ADJ_*) are gs_gn_step.hpp's, shared with sdf.hip; rgbd.hip includes it before this header.
// Per iteration, last to first:
// Xb step reverse (gn_step_bwd_k<false>): folds the 12-sum rows the pixel pass before left into the carried adjoint of T and
//    leaves the adjoints of the iteration's 28 sums.
// Lb pixel reverse, the forward's geometry: the pixel's forward values again from the taped T_k (rgbd_pixel_fwd, rgbd_chan_row),
//    the adjoints of its two rows and residuals from those of the sums, pulled back to q, the eight corner values, the source
//    pixel and T.  <MAX> does all of it but the corner sums, of which it takes the largest magnitude; <ACC> only adds the corner
//    terms into the level's exact fold (gs_fixed128.hpp).  One fold and one finish per level.
// Pb the pyramids' adjoints, coarsest to finest, after all levels: a gather per fine pixel, then level 0 into the images.
#pragma once

#include "gs_fixed128.hpp"
#include "gs_gn_step.hpp"
#include "gs_rgbd_pixel.hpp"

namespace gs {

enum { RGBD_BWD_MAX = 0, RGBD_BWD_ACC = 1 };

// One channel F (I or D) of a valid pixel: its row J (6) and residual r again (rgbd_chan_row), their adjoints from those of the
// sums (M: the symmetric 6 x 6 that J-bar = M J + g r needs, g: the adjoints of the six sums J r, e2 = twice err's), pulled back
// to the four corners cb (00, 10, 01, 11), to q, iz, gx, gy and to the cell coordinates a, b.  Returns the adjoint of `minus`.
__device__ __forceinline__ float rgbd_chan_bwd(float F00, float F10, float F01, float F11, float minus, float cz, float w, const RgbdPix &P,
                                               float gx, float gy, const float *__restrict__ M, const float *__restrict__ g, float e2,
                                               float (&cb)[4], float &qxb, float &qyb, float &qzb, float &izb, float &gxb, float &gyb,
                                               float &ab, float &bbb) {
    const float qx = P.qx, qy = P.qy, qz = P.qz, iz = P.iz, a = P.a, bb = P.bb;
    const RgbdChan C = rgbd_chan_row(F00, F10, F01, F11, minus, cz, w, P, gx, gy);
    const float X0 = C.X0, X1 = C.X1, top = C.top, bot = C.bot, Fx = C.Fx, Fy = C.Fy, c0 = C.c0, c1 = C.c1, c2 = C.c2, t = C.t;
    float Jb[6], rb = e2 * C.r;
#pragma unroll
    for (int u = 0; u < 6; ++u) {
        float v = g[u] * C.r;
#pragma unroll
        for (int k = 0; k < 6; ++k) v += M[6 * u + k] * C.J[k];
        Jb[u] = v;
        rb += g[u] * C.J[u];
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
    static_assert(RGBD_T == BWD_T, "the 12-wide rows are block_row<12, BWD_WAVES>'s: blocks of BWD_T threads");
    __shared__ float M[36], g[6], e2s;
    const int b = blockIdx.y, npix = Hl * Wl;
    const int p = blockIdx.x * RGBD_T + threadIdx.x;
    const float *__restrict__ A = adj + GN_ADJ_WORDS * b;
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
    if (p < npix && A[GN_ADJ_LIVE] != 0.0f) {
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
        block_row<12, BWD_WAVES>(acc, [&](unsigned n) { return &partials12[(int64_t)b * prow * 12 + (blockIdx.x * 12 + n)]; });
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
    const RgbdSel sel = rgbd_down_select(c, ddm);
    const float2 go = gout[(int64_t)blockIdx.y * Hl * Wl + (int64_t)cv * Wl + cu];
    const bool taken = (sel.taken >> (2 * (v & 1) + (u & 1))) & 1;
    float2 *o = gin + (int64_t)blockIdx.y * Hp * Wp + p;
    const float2 old = *o;
    *o = make_float2(old.x + 0.25f * go.x, old.y + (taken ? go.y / (float)sel.n : 0.0f));
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
    if (g_depth) g_depth[i] = rgbd_depth_kept(depth[i]) ? gi.y : 0.0f;
}

}  // namespace gs
