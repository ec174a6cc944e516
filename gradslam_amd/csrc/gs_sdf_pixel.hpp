// gs_sdf_pixel.hpp -- the pixel of the SDF odometry (sdf.hip), stated once: device functions and constants only, no kernels.
// sdf_pixel_fwd is the rule of include/gradslam_hip.h, every fp32 operation in its order: back-projection, the two transforms,
// the cell, the gates in their order, the row.  A reverse pass includes THIS header, so that it differentiates exactly the pixels
// the forward pass used.
#pragma once

#include "gs_tsdf.hpp"

namespace gs {

struct SdfCam { float fx, fy, cx, cy; };
__device__ __forceinline__ SdfCam sdf_cam(const float *__restrict__ K) { return SdfCam{K[0], K[5], K[2], K[6]}; }

// the depth gate: positive and finite (a NaN fails both comparisons)
__device__ __forceinline__ bool sdf_depth_kept(float d) { return d > 0.0f && d < INFINITY; }

// the pixel's forward values (set only as far as its gates were passed)
struct SdfPix {
    float px, py, d;
    f3 pw, q;         // world point under the frame's pose; under the loop's delta
    TsdfCell c;
    float w8[8], f8[8];
    float fh;         // the interpolant
    f3 g;             // its gradient in voxel units
    float J[6], r;
};

// Full-resolution pixel (h, w) with depth d; P, D: a batch element's pose and delta (12 leading floats each); vol.origin: the
// batch element's origin; tsdf, weight: its volume.  The gates in their order: depth positive and finite; the cell inside (a NaN
// or an infinity is outside); 8 corner weights >= minw; 8 corner values < 1.  The 16 gathers are requested in ONE batch behind
// the cell gate (the cell bounds every address) -- the weights are not waited for before the values are asked for; testing the
// weights first, as tsdf_sample_at does, takes the same decisions and leaves the same bits.  Nested, no early return.
__device__ __forceinline__ bool sdf_pixel_fwd(float d, int h, int w, const SdfCam cam, const float *__restrict__ P,
                                              const float *__restrict__ D, const TsdfVol &vol, const float *__restrict__ tsdf,
                                              const float *__restrict__ weight, float minw, float kappa, SdfPix &X) {
    bool ok = sdf_depth_kept(d);
    if (ok) {
        const float px = d * (((float)w - cam.cx) / cam.fx), py = d * (((float)h - cam.cy) / cam.fy);
        const f3 pw{((P[0] * px + P[1] * py) + P[2] * d) + P[3], ((P[4] * px + P[5] * py) + P[6] * d) + P[7],
                    ((P[8] * px + P[9] * py) + P[10] * d) + P[11]};
        const f3 q{((D[0] * pw.x + D[1] * pw.y) + D[2] * pw.z) + D[3], ((D[4] * pw.x + D[5] * pw.y) + D[6] * pw.z) + D[7],
                   ((D[8] * pw.x + D[9] * pw.y) + D[10] * pw.z) + D[11]};
        X.px = px; X.py = py; X.d = d; X.pw = pw; X.q = q;
        ok = tsdf_cell(vol, vol.origin, q, X.c);
        if (ok) {
            tsdf_gather8(vol, weight, X.c.j, X.w8);
            tsdf_gather8(vol, tsdf, X.c.j, X.f8);
            bool seen = true, near = true;
#pragma unroll
            for (int c = 0; c < 8; ++c) seen = seen && X.w8[c] >= minw;
#pragma unroll
            for (int c = 0; c < 8; ++c) near = near && X.f8[c] < 1.0f;
            ok = seen && near;
            X.fh = tsdf_trilerp(X.f8, X.c);
            X.g = tsdf_trigrad(X.f8, X.c);
            X.r = vol.trunc * X.fh;
            const float nx = kappa * X.g.x, ny = kappa * X.g.y, nz = kappa * X.g.z;
            X.J[0] = nx; X.J[1] = ny; X.J[2] = nz;
            X.J[3] = q.y * nz - q.z * ny; X.J[4] = q.z * nx - q.x * nz; X.J[5] = q.x * ny - q.y * nx;
        }
    }
    return ok;
}

}  // namespace gs
