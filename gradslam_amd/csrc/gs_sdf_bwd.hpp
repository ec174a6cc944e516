// gs_sdf_bwd.hpp -- the SDF odometry's own kernels of its reverse pass (the rule: include/gradslam_hip.h).  Included by sdf.hip after
// its forward kernel (SDF_T, SdfGrid, SdfVolume are sdf.hip's), which launches them (sdf_bwd_run); the pixel's forward values are
// gs_sdf_pixel.hpp's, the forward's own code.  The step reverse, the fold of the 12-wide rows, the seam's adjoint row and the
// layouts of the tape row (GN_TAPE_*) and of the adjoint row (GN_ADJ_*) are gs_gn_step.hpp's, shared with rgbd.hip.
// Per iteration, last to first:
// Xb step reverse (gn_step_bwd_k<true>): folds the 12-sum rows the pixel pass before left into the carried adjoint of D and
//    leaves the adjoints of the iteration's 28 sums; it also folds the pixel pass's 12-sum rows of the POSES' adjoint onto the
//    running g_poses.
// Lb pixel reverse, the forward's geometry: the pixel's forward values again at the taped D_k (sdf_pixel_fwd: the same 16 gathers in
//    one batch), the adjoints of its row and residual from those of the sums, pulled back to the eight corner values, to q, to D,
//    to the pose and to the depth.  <MAX> does all of it but the corner sums, of which it takes the largest magnitude; <ACC> only
//    adds the corner terms into the exact fold (gs_fixed128.hpp): ONE fold over the volume for the whole loop, one finish.
#pragma once

#include "gs_fixed128.hpp"
#include "gs_gn_step.hpp"
#include "gs_sdf_pixel.hpp"

namespace gs {

enum { SDF_BWD_MAX = 0, SDF_BWD_ACC = 1 };

// the loop's start: gD[b] = rows 0..2 of grad_T[b] (the bottom row zero), gP[b] = 0.  One thread per word of (B, 16).
__global__ __launch_bounds__(256) void sdf_bwd_begin_k(const float *__restrict__ grad_T, int B, float *__restrict__ gD,
                                                      float *__restrict__ gP) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 16 * B) return;
    gD[i] = (i & 15) < 12 ? grad_T[i] : 0.0f;
    gP[i] = 0.0f;
}

// grid (blocks of SDF_T pixels of the level's grid, B), sdf_linearize_k's.  D: batch element b's delta at Dall + dstride b; adj
// (B, 32).  MAX: g_depth[pixel] += the pixel's depth adjoint (its owner lane, in launch order; NULL: not wanted); the block's 12
// sums of D's adjoint -> partD row blockIdx.x, of the pose's -> partP (NULL: not wanted); the largest corner term -> the fold
// (fold.maxbits NULL: no volume adjoint is wanted).  ACC: the eight corner terms -> the fold's sums (row = the voxel), scaled for
// at most 2^lg terms per sum.
template <int MODE>
__global__ __launch_bounds__(SDF_T) void sdf_pixel_bwd_k(const float *__restrict__ depth, SdfGrid gr, const float *__restrict__ K,
                                                        const float *__restrict__ Pall, const float *__restrict__ Dall, int dstride,
                                                        SdfVolume vo, const float *__restrict__ adj, Fold fold, int lg,
                                                        float *__restrict__ g_depth, float *__restrict__ partD,
                                                        float *__restrict__ partP, int prow) {
    static_assert(SDF_T == BWD_T, "the 12-wide rows are block_row<12, BWD_WAVES>'s: blocks of BWD_T threads");
    __shared__ float M[36], gv[6], e2s;
    const int b = blockIdx.y, npix = gr.Hs * gr.Ws;
    const int p = blockIdx.x * SDF_T + threadIdx.x;
    const float *__restrict__ A = adj + GN_ADJ_WORDS * b;
    if (threadIdx.x < 36) {
        int u = threadIdx.x / 6, v = threadIdx.x % 6;
        const bool diag = u == v;
        if (u > v) { const int t = u; u = v; v = t; }
        const float s = A[u * 6 - (u * (u - 1)) / 2 + (v - u)];
        M[threadIdx.x] = diag ? 2.0f * s : s;
    } else if (threadIdx.x < 42) {
        gv[threadIdx.x - 36] = A[21 + (threadIdx.x - 36)];
    } else if (threadIdx.x == 42) {
        e2s = 2.0f * A[27];
    }
    __syncthreads();
    const SdfCam cam = sdf_cam(K + 16 * b);
    const TsdfVol vol{vo.nx, vo.ny, vo.nz, vo.v, vo.trunc, 0.0f, vo.origin + 3 * b};
    const int64_t nvox = tsdf_nvox(vol);
    const float *__restrict__ P = Pall + 16 * b;
    const float *__restrict__ D = Dall + (int64_t)dstride * b;

    float d = 0.0f;  // (a lane past the grid's last pixel, or a step that was not applied: depth 0, not valid)
    int h = 0, w = 0;
    if (p < npix && A[GN_ADJ_LIVE] != 0.0f) {
        const int i = p / gr.Ws, j = p - i * gr.Ws;
        h = i * gr.s;
        w = j * gr.s;
        d = depth[((int64_t)b * gr.H + h) * gr.W + w];
    }
    SdfPix X;
    const bool ok = sdf_pixel_fwd(d, h, w, cam, P, D, vol, vo.tsdf + b * nvox, vo.weight + b * nvox, vo.minw, vo.kappa, X);
    float accD[12], accP[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { accD[k] = 0.0f; accP[k] = 0.0f; }
    uint32_t mx = 0;
    const bool want_vol = fold.maxbits != nullptr;
    const int E = MODE == SDF_BWD_ACC ? det_scale(*fold.maxbits, lg) : 0;
    if (ok) {
        float Jb[6], rb = e2s * X.r;
#pragma unroll
        for (int u = 0; u < 6; ++u) {
            float v = gv[u] * X.r;
#pragma unroll
            for (int k = 0; k < 6; ++k) v += M[6 * u + k] * X.J[k];
            Jb[u] = v;
            rb += gv[u] * X.J[u];
        }
        const f3 q = X.q, n{X.J[0], X.J[1], X.J[2]}, m{Jb[3], Jb[4], Jb[5]};
        // J_rot = q x n:  n-bar = J-bar[0..2] + m x q,  q-bar = n x m
        const float nbx = Jb[0] + (m.y * q.z - m.z * q.y), nby = Jb[1] + (m.z * q.x - m.x * q.z), nbz = Jb[2] + (m.x * q.y - m.y * q.x);
        const float gbx = vo.kappa * nbx, gby = vo.kappa * nby, gbz = vo.kappa * nbz, fhb = vo.trunc * rb;
        if (MODE == SDF_BWD_ACC || want_vol) {
            const float ax = X.c.ax, ay = X.c.ay, az = X.c.az;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float wx = (c & 1) ? ax : 1.0f - ax, wy = (c & 2) ? ay : 1.0f - ay, wz = (c & 4) ? az : 1.0f - az;
                const float wxy = wx * wy;
                const float W = wxy * wz, dWx = ((c & 1) ? wy : -wy) * wz, dWy = ((c & 2) ? wx : -wx) * wz, dWz = (c & 4) ? wxy : -wxy;
                const float cb = ((fhb * W + gbx * dWx) + gby * dWy) + gbz * dWz;
                if (MODE == SDF_BWD_ACC)
                    fold_add(fold, (int64_t)b * nvox + tsdf_corner(vol, X.c.j, c), 0, cb, E);
                else
                    mx = fold_max(mx, cb);
            }
        }
        if (MODE == SDF_BWD_MAX) {
            const float *f = X.f8;
            const float ax = X.c.ax, ay = X.c.ay, az = X.c.az;
            // the interpolant's second derivatives inside the cell: no pure ones; the mixed differences, lerped over the third axis
            const float Hxy = tsdf_lerp((f[3] - f[2]) - (f[1] - f[0]), (f[7] - f[6]) - (f[5] - f[4]), az);
            const float Hxz = tsdf_lerp((f[5] - f[4]) - (f[1] - f[0]), (f[7] - f[6]) - (f[3] - f[2]), ay);
            const float Hyz = tsdf_lerp((f[6] - f[4]) - (f[2] - f[0]), (f[7] - f[5]) - (f[3] - f[1]), ax);
            const float abx = (fhb * X.g.x + Hxy * gby) + Hxz * gbz;
            const float aby = (fhb * X.g.y + Hxy * gbx) + Hyz * gbz;
            const float abz = (fhb * X.g.z + Hxz * gbx) + Hyz * gby;
            const float qbx = (n.y * m.z - n.z * m.y) + abx / vo.v, qby = (n.z * m.x - n.x * m.z) + aby / vo.v,
                        qbz = (n.x * m.y - n.y * m.x) + abz / vo.v;
            // q = D (pw, 1)
            accD[0] = qbx * X.pw.x; accD[1] = qbx * X.pw.y; accD[2] = qbx * X.pw.z; accD[3] = qbx;
            accD[4] = qby * X.pw.x; accD[5] = qby * X.pw.y; accD[6] = qby * X.pw.z; accD[7] = qby;
            accD[8] = qbz * X.pw.x; accD[9] = qbz * X.pw.y; accD[10] = qbz * X.pw.z; accD[11] = qbz;
            const float pwbx = (D[0] * qbx + D[4] * qby) + D[8] * qbz, pwby = (D[1] * qbx + D[5] * qby) + D[9] * qbz,
                        pwbz = (D[2] * qbx + D[6] * qby) + D[10] * qbz;
            // pw = P (px, py, d, 1)
            accP[0] = pwbx * X.px; accP[1] = pwbx * X.py; accP[2] = pwbx * X.d; accP[3] = pwbx;
            accP[4] = pwby * X.px; accP[5] = pwby * X.py; accP[6] = pwby * X.d; accP[7] = pwby;
            accP[8] = pwbz * X.px; accP[9] = pwbz * X.py; accP[10] = pwbz * X.d; accP[11] = pwbz;
            if (g_depth) {
                const float ux = ((float)w - cam.cx) / cam.fx, vy = ((float)h - cam.cy) / cam.fy;
                const float pxb = (P[0] * pwbx + P[4] * pwby) + P[8] * pwbz, pyb = (P[1] * pwbx + P[5] * pwby) + P[9] * pwbz;
                const float db = (((P[2] * pwbx + P[6] * pwby) + P[10] * pwbz) + pxb * ux) + pyb * vy;
                float *o = g_depth + ((int64_t)b * gr.H + h) * gr.W + w;
                *o = *o + db;
            }
        }
    }
    if (MODE == SDF_BWD_MAX) {
        if (want_vol) {
            // The fold's maximum only grows, so a term no larger than a value it has held needs no atomic: after the first blocks
            // almost none is issued (thousands of waves, one address).  The maximum is the same whichever are skipped.
            if (mx <= __hip_atomic_load(fold.maxbits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) mx = 0;
            fold_max_commit(fold.maxbits, mx);
        }
        block_row<12, BWD_WAVES>(accD, [&](unsigned k) { return &partD[(int64_t)b * prow * 12 + (blockIdx.x * 12 + k)]; });
        if (partP) {
            __syncthreads();
            block_row<12, BWD_WAVES>(accP, [&](unsigned k) { return &partP[(int64_t)b * prow * 12 + (blockIdx.x * 12 + k)]; });
        }
    }
}

// the volume's adjoint from the fold: n = B nx ny nz rows, one channel
__global__ __launch_bounds__(256) void sdf_fold_finish_k(Fold fold, int lg, int64_t n, float *__restrict__ g_tsdf) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int E = det_scale(*fold.maxbits, lg);
    g_tsdf[i] = fold_result(fold, i, 0, E);
}

}  // namespace gs
