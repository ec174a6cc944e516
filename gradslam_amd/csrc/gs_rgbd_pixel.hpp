// gs_rgbd_pixel.hpp -- what the forward kernels of the dense RGB-D odometry (rgbd.hip) and its reverse pass (gs_rgbd_bwd.hpp)
// must agree on, bit for bit, stated once: device functions and constants only, no kernels.
//   the pixel     rgbd_cam, rgbd_pixel_fwd (warp, cell, four corner loads, the four gates), rgbd_chan_row (one channel's row and
//                 residual).  Both passes run THIS code -- the rule of include/gradslam_hip.h, every fp32 operation in its order --
//                 so the reverse pass differentiates exactly the pixels the forward pass used.
//   the pyramid   rgbd_depth_kept (level 0), rgbd_down_select (the 2 x 2 reduction's depth selection).
// (The layout of an iteration's tape row, written by gn_step_k<true> and read by gn_step_bwd_k, is the step's: gs_gn_step.hpp.)
#pragma once

#include "gs_icp_reduce.hpp"

namespace gs {

constexpr int RGBD_T = LIN_T;  // lanes (= source pixels) per linearise block: linearize_k's geometry (icp.hip)

struct RgbdCam { float fx, fy, cx, cy; };
// intrinsics (4 x 4 row-major) at pyramid level `level`: fx, fy halve; cx' = (cx + 0.5) / 2 - 0.5 (pixel centres at integers)
__device__ __forceinline__ RgbdCam rgbd_cam(const float *__restrict__ K, int level) {
    RgbdCam c{K[0], K[5], K[2], K[6]};
    for (int l = 0; l < level; ++l) {
        c.fx = c.fx * 0.5f; c.fy = c.fy * 0.5f;
        c.cx = (c.cx + 0.5f) * 0.5f - 0.5f; c.cy = (c.cy + 0.5f) * 0.5f - 0.5f;
    }
    return c;
}

// ------------------------------ the pyramid's rules: level 0 keeps a depth that is positive and finite (anything else becomes 0)
__device__ __forceinline__ bool rgbd_depth_kept(float d) { return d > 0.0f && d < INFINITY; }

// The 2 x 2 reduction's depth selection, c = the block's four (I, D) in the order 00, 10, 01, 11 (x offset first): dmin, the
// smallest positive depth (INFINITY: none); bit k of `taken`: c[k]'s depth is positive and within ddm of dmin -- foreground and
// background are never averaged; n = how many are.  The coarse depth is the mean of the taken ones (0 if n = 0).
struct RgbdSel { float dmin; int taken, n; };
__device__ __forceinline__ RgbdSel rgbd_down_select(const float2 (&c)[4], float ddm) {
    float dmin = INFINITY;
    int taken = 0, n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) dmin = (c[k].y > 0.0f && c[k].y < dmin) ? c[k].y : dmin;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (c[k].y > 0.0f && c[k].y - dmin <= ddm) { taken |= 1 << k; ++n; }
    return RgbdSel{dmin, taken, n};
}

// ------------------------------------------------------------------ the pixel: its forward values (set only when it is valid)
struct RgbdPix {
    float px, py, d, ux, vy;  // the back-projection: px = d ux, py = d vy
    float qx, qy, qz, iz, a, bb;
    int corner;               // c00's index in the level's image
    float2 c00, c10, c01, c11;  // c_xy: x offset first
    float Is;
};
// The source pixel s = (I, D) at (u, v) of a Hl x Wl level, warped by T (a batch element's 12 leading floats) into the target
// level `timg`: back-projection, transform, projection, the bilinear cell, its four corners (one 8-byte load each) and the four
// gates in their order -- source depth positive; q_z positive; the cell inside (0 <= i <= W - 2, 0 <= j <= H - 2: a NaN fails
// every comparison); four corner depths positive; |D^ - q_z| <= ddm, D^ the depth interpolant.  Shaped after the forward kernel,
// the hot one: nested, no early return, the corners loaded before their gate.
__device__ __forceinline__ bool rgbd_pixel_fwd(const float2 *__restrict__ timg, const float2 s, int u, int v, int Hl, int Wl,
                                               const RgbdCam cam, const float *__restrict__ T, float ddm, RgbdPix &P) {
    bool ok = s.y > 0.0f;
    if (ok) {
        const float d = s.y;
        const float ux = ((float)u - cam.cx) / cam.fx, vy = ((float)v - cam.cy) / cam.fy;
        const float px = d * ux, py = d * vy;
        const float qx = ((T[0] * px + T[1] * py) + T[2] * d) + T[3];
        const float qy = ((T[4] * px + T[5] * py) + T[6] * d) + T[7];
        const float qz = ((T[8] * px + T[9] * py) + T[10] * d) + T[11];
        ok = qz > 0.0f;
        const float iz = 1.0f / qz;
        const float x = (cam.fx * qx) * iz + cam.cx, y = (cam.fy * qy) * iz + cam.cy;
        const float xf = floorf(x), yf = floorf(y);
        ok = ok && xf >= 0.0f && xf <= (float)(Wl - 2) && yf >= 0.0f && yf <= (float)(Hl - 2);
        if (ok) {
            const int i = (int)xf, j = (int)yf;
            const float a = x - xf, bb = y - yf;
            const int corner = j * Wl + i;
            const float2 *c = timg + corner;
            const float2 c00 = c[0], c10 = c[1], c01 = c[Wl], c11 = c[Wl + 1];
            ok = c00.y > 0.0f && c10.y > 0.0f && c01.y > 0.0f && c11.y > 0.0f;
            const float dX0 = c10.y - c00.y, dX1 = c11.y - c01.y;
            const float dTop = c00.y + a * dX0, dBot = c01.y + a * dX1;
            const float Dh = dTop + bb * (dBot - dTop);
            ok = ok && fabsf(Dh - qz) <= ddm;
            P.px = px; P.py = py; P.d = d; P.ux = ux; P.vy = vy;
            P.qx = qx; P.qy = qy; P.qz = qz; P.iz = iz; P.a = a; P.bb = bb;
            P.corner = corner;
            P.c00 = c00; P.c10 = c10; P.c01 = c01; P.c11 = c11;
            P.Is = s.x;
        }
    }
    return ok;
}

// One channel F (I or D) of a valid pixel: the bilinear interpolant F^ of the four corner values and its exact derivatives; the
// row of d(value) / dq as (c0, c1, c2) with gx = fx iz, gy = fy iz; d q / d xi = [I | -q^]  ->  J = w (c | q x c); r = w (F^ -
// minus).  `minus`: the other term of the residual (I_s or q_z); cz = d(minus) / d q_z: 0 for the intensity (-(t iz) - 0 is
// -(t iz), and the compiler folds it), 1 for the depth.  The intermediate values are what the adjoint needs.
struct RgbdChan { float X0, X1, top, bot, Fx, Fy, c0, c1, c2, t, J[6], r; };
__device__ __forceinline__ RgbdChan rgbd_chan_row(float F00, float F10, float F01, float F11, float minus, float cz, float w,
                                                  const RgbdPix &P, float gx, float gy) {
    const float qx = P.qx, qy = P.qy, qz = P.qz;
    RgbdChan C;
    C.X0 = F10 - F00; C.X1 = F11 - F01;
    C.top = F00 + P.a * C.X0; C.bot = F01 + P.a * C.X1;
    const float Fh = C.top + P.bb * (C.bot - C.top);
    C.Fx = C.X0 + P.bb * (C.X1 - C.X0); C.Fy = C.bot - C.top;
    C.c0 = C.Fx * gx; C.c1 = C.Fy * gy; C.t = C.c0 * qx + C.c1 * qy; C.c2 = -(C.t * P.iz) - cz;
    C.J[0] = w * C.c0; C.J[1] = w * C.c1; C.J[2] = w * C.c2;
    C.J[3] = w * (qy * C.c2 - qz * C.c1); C.J[4] = w * (qz * C.c0 - qx * C.c2); C.J[5] = w * (qx * C.c1 - qy * C.c0);
    C.r = w * (Fh - minus);
    return C;
}

}  // namespace gs
