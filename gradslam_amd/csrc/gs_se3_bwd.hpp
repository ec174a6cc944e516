// gs_se3_bwd.hpp -- the O(1) adjoints of a Gauss-Newton step on SE(3): device functions, no kernels, so that every translation
// unit with a reverse pass (icp.hip through gs_icp_bwd.hpp, rgbd.hip) can include it.
//   T' = dT T, dT = exp(xi), xi = (H + damp I)^-1 g:  top3_times_Tt / pull_gT, se3_exp_bwd, solve_bwd (fp64 on one lane)
//   the adjoint of a transform is a sum of 12 terms per point or pixel, in gs_rowsum.hpp's order: block_row<12, BWD_WAVES> by
//   blocks of BWD_T threads, fold_rows<12, BWD_GROUPS, 16> over their rows
#pragma once

#include "gs_icp_step.hpp"
#include "gs_rowsum.hpp"

namespace gs {

constexpr int BWD_T = 256, BWD_WAVES = BWD_T / kWave, BWD_GROUPS = BWD_T / 16;

// ---- O(1) adjoints, fp64 on one lane
// adjoint of T = se3_exp(xi) (se3_exp_dev above, both branches) given gT (top 3 rows, row-major 3x4)
__device__ void se3_exp_bwd(const float *xi, const double *gT, double *gxi) {
    const double v[3] = {xi[0], xi[1], xi[2]}, w[3] = {xi[3], xi[4], xi[5]};
    const double Wh[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    const float thf = sqrtf(__fmaf_rn(xi[5], xi[5], __fmaf_rn(xi[4], xi[4], xi[3] * xi[3])));  // the branch the forward took
    double gR[9], gV[9], gt[3] = {gT[3], gT[7], gT[11]};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { gR[3 * i + j] = gT[4 * i + j]; gV[3 * i + j] = gt[i] * v[j]; }
    double V[9], gWh[9], gw[3] = {0.0, 0.0, 0.0};
    if (thf < 1e-6f) {
        for (int i = 0; i < 9; ++i) { V[i] = ((i % 4 == 0) ? 1.0 : 0.0) + Wh[i]; gWh[i] = gR[i] + gV[i]; }
    } else {
        const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        const double s = sin(th), c = cos(th);
        double W2[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) W2[3 * i + j] = Wh[3 * i] * Wh[j] + Wh[3 * i + 1] * Wh[3 + j] + Wh[3 * i + 2] * Wh[6 + j];
        const double th2 = th * th, th3 = th2 * th, th4 = th2 * th2;
        const double A = s / th, Bc = (1.0 - c) / th2, C = (th - s) / th3;
        double gA = 0.0, gB = 0.0, gC = 0.0, gW2[9];
        for (int i = 0; i < 9; ++i) {
            V[i] = ((i % 4 == 0) ? 1.0 : 0.0) + Bc * Wh[i] + C * W2[i];
            gA += gR[i] * Wh[i];
            gB += gR[i] * W2[i] + gV[i] * Wh[i];
            gC += gV[i] * W2[i];
            gWh[i] = A * gR[i] + Bc * gV[i];
            gW2[i] = Bc * gR[i] + C * gV[i];
        }
        for (int i = 0; i < 3; ++i)      // W2 = Wh Wh : gWh += gW2 Wh^T + Wh^T gW2
            for (int j = 0; j < 3; ++j) {
                double a = 0.0;
                for (int k = 0; k < 3; ++k) a += gW2[3 * i + k] * Wh[3 * j + k] + Wh[3 * k + i] * gW2[3 * k + j];
                gWh[3 * i + j] += a;
            }
        const double dA = (c * th - s) / th2, dB = (s * th - 2.0 * (1.0 - c)) / th3, dC = ((1.0 - c) * th - 3.0 * (th - s)) / th4;
        const double gth = gA * dA + gB * dB + gC * dC;
        for (int k = 0; k < 3; ++k) gw[k] = gth * w[k] / th;
    }
    gw[0] += gWh[7] - gWh[5];
    gw[1] += gWh[2] - gWh[6];
    gw[2] += gWh[3] - gWh[1];
    for (int j = 0; j < 3; ++j) gxi[j] = V[j] * gt[0] + V[3 + j] * gt[1] + V[6 + j] * gt[2];  // V^T gt
    gxi[3] = gw[0]; gxi[4] = gw[1]; gxi[5] = gw[2];
}

__device__ __forceinline__ void top3_times_Tt(const float *gTn, const float *T, double *out12) {  // (gTn . T^T) rows 0..2
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
            double a = 0.0;
            for (int k = 0; k < 4; ++k) a += (double)gTn[4 * i + k] * (double)T[4 * j + k];
            out12[4 * i + j] = a;
        }
}
__device__ __forceinline__ void pull_gT(float *gT, const float *dT) {  // gT <- dT^T gT
    float r[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double a = 0.0;
            for (int k = 0; k < 4; ++k) a += (double)dT[4 * k + i] * (double)gT[4 * k + j];
            r[4 * i + j] = (float)a;
        }
    for (int i = 0; i < 16; ++i) gT[i] = r[i];
}
// xi = (H + damp I)^-1 g : given gxi -> G (Hbar, gbar), returns damp_bar
__device__ double solve_bwd(const float *H, float damp, const float *xi, const double *gxi, float *G) {
    float gx[6], y[6];
    double lu[42];
    for (int i = 0; i < 6; ++i) gx[i] = (float)gxi[i];
    solve6(H, gx, damp, y, lu);  // M symmetric: M^-T = M^-1
    double gd = 0.0;
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < 6; ++j) G[6 * i + j] = -y[i] * xi[j];
        G[36 + i] = y[i];
        gd -= (double)y[i] * (double)xi[i];
    }
    return gd;
}

}  // namespace gs
