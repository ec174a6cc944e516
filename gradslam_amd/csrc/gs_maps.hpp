// gs_maps.hpp -- the body of the maps kernel (maps.hip: vertex_normal_k) as a device function of a VIRTUAL block index, so
// that another launch can carry its tiles (project.hip: setup_count_k, the fused front end of gs_slam_localize).
#pragma once

#include "gs_common.hpp"

namespace gs {

constexpr int TW = 64, TH = 4;

struct Kinv4 {
    float a, c, e, f;  // x = a*w + c ; y = e*h + f   (reference geometry/projutils.py:444-449)
};

__device__ __forceinline__ Kinv4 load_kinv(const float *__restrict__ K) {
    const float eps = 1e-6f;
    const float fx = K[0] + eps, fy = K[5] + eps;
    return Kinv4{1.0f / fx, (-1.0f * K[2]) / fx, 1.0f / fy, (-1.0f * K[6]) / fy};
}

// local vertex of pixel (h, w) with depth d:  (Kinv . [w,h,1]) * d * (d > 0)
// the reference's einsum contracts [a,0,c].[w,h,1] as fma(c,1,fma(0,h,a*w)) == a*w + c
__device__ __forceinline__ f3 vertex_of(const Kinv4 k, int h, int w, float d) {
    const float m = d > 0.0f ? 1.0f : 0.0f;
    const float x = k.a * (float)w + k.c;
    const float y = k.e * (float)h + k.f;
    return f3{(x * d) * m, (y * d) * m, (1.0f * d) * m};
}

// What the PointFusion update lets ride on this pass over the pixels (slam.hip, fusion.hip; all optional): the sample
// confidence alpha = get_alpha(local vertex) (slam/fusionutils.py:69-73, the arithmetic of alpha_k below), the
// "no candidate / no winner" initialisation of the correspondence stage's per-pixel state, and the zeroing of its counter
// block -- three launches (alpha_k, two memsets) that become stores of a kernel that visits every pixel anyway.
struct VnExtra {
    float *alpha;                  // (B*L*H*W) or NULL
    float alpha_den, alpha_eps;    // 2 sigma^2, lower clamp
    unsigned long long *pix_key;   // (B*L*H*W) or NULL: set to ~0
    unsigned int *pix_n;           // (B*L*H*W) or NULL: set to ~0
    int32_t *zero;                 // n_zero words zeroed by the first block, or NULL
    int n_zero;
    float *cam_out;                // (B*L, 32) or NULL: a copy of every frame's pose | intrinsics at an address of the CALLEE's
                                   // choosing (gs_slam_localize: its workspace -- what a captured graph of the ICP loops may bake in)
};

// (bx, by, bz) = the tile's block index in vertex_normal_k's grid (cdiv(W, TW), cdiv(H, TH), B * L)
__device__ __forceinline__ void vertex_normal_body(const float *__restrict__ depth, const float *__restrict__ Ks,
                                                   const float *__restrict__ poses, int L, int H, int W,
                                                   float *__restrict__ vertex, float *__restrict__ normal,
                                                   float *__restrict__ gvertex, float *__restrict__ gnormal, const VnExtra &ex,
                                                   int bx, int by, int bz) {
    __shared__ float sd[TH + 1][TW + 1];
    if (ex.zero && bx == 0 && by == 0 && bz == 0)
        for (int i = threadIdx.x; i < ex.n_zero; i += TW * TH) ex.zero[i] = 0;
    if (ex.cam_out && poses && bx == 0 && by == 0 && threadIdx.x < 32) {
        const int blz = bz;
        ex.cam_out[32 * blz + threadIdx.x] = threadIdx.x < 16 ? poses[16 * (int64_t)blz + threadIdx.x] : Ks[16 * (blz / L) + threadIdx.x - 16];
    }
    const int bl = bz;  // b*L + l
    const int b = bl / L;
    const int w0 = bx * TW, h0 = by * TH;
    const int tx = threadIdx.x & (TW - 1), ty = threadIdx.x / TW;
    const float *dimg = depth + (int64_t)bl * H * W;

    // stage the depth tile (+1 halo column/row, clamped at the image edge)
    for (int i = threadIdx.x; i < (TH + 1) * (TW + 1); i += TW * TH) {
        const int r = i / (TW + 1), c = i - r * (TW + 1);
        const int hh = min(h0 + r, H - 1), ww = min(w0 + c, W - 1);
        sd[r][c] = dimg[(int64_t)hh * W + ww];
    }
    __syncthreads();

    const int h = h0 + ty, w = w0 + tx;
    if (h >= H || w >= W) return;
    const Kinv4 k = load_kinv(Ks + 16 * b);
    const float d = sd[ty][tx];
    const f3 v = vertex_of(k, h, w, d);

    // forward differences; the last column / row re-use the previous difference
    // (reference structures/rgbdimages.py:724-731).  Neighbour validity is NOT checked.
    f3 dh, dv;
    if (w < W - 1) {
        const f3 vr = vertex_of(k, h, w + 1, sd[ty][tx + 1]);
        dh = f3{vr.x - v.x, vr.y - v.y, vr.z - v.z};
    } else {  // w == W-1: V(h,W-1) - V(h,W-2); W-2 may sit in the previous tile -> global read
        const float dl = (tx > 0) ? sd[ty][tx - 1] : dimg[(int64_t)h * W + (w - 1)];
        const f3 vl = vertex_of(k, h, w - 1, dl);
        dh = f3{v.x - vl.x, v.y - vl.y, v.z - vl.z};
    }
    if (h < H - 1) {
        const f3 vd = vertex_of(k, h + 1, w, sd[ty + 1][tx]);
        dv = f3{vd.x - v.x, vd.y - v.y, vd.z - v.z};
    } else {
        const float du = (ty > 0) ? sd[ty - 1][tx] : dimg[(int64_t)(h - 1) * W + w];
        const f3 vu = vertex_of(k, h - 1, w, du);
        dv = f3{v.x - vu.x, v.y - vu.y, v.z - vu.z};
    }
    // torch.cross contracts each component as fma(a1, b2, -(a2*b1))
    f3 n;
    n.x = __fmaf_rn(dh.y, dv.z, -(dh.z * dv.y));
    n.y = __fmaf_rn(dh.z, dv.x, -(dh.x * dv.z));
    n.z = __fmaf_rn(dh.x, dv.y, -(dh.y * dv.x));
    // .norm(dim) contracts as sqrt(fma(z,z,fma(y,y,x*x)))
    float nn = sqrtf(__fmaf_rn(n.z, n.z, __fmaf_rn(n.y, n.y, n.x * n.x)));
    nn = (nn == 0.0f) ? 1.0f : nn;
    const float m = d > 0.0f ? 1.0f : 0.0f;
    n = f3{(n.x / nn) * m, (n.y / nn) * m, (n.z / nn) * m};

    const int64_t pix = (int64_t)bl * H * W + (int64_t)h * W + w;
    if (ex.alpha) {  // alpha_k's arithmetic on the local vertex
        const float ss = (v.x * v.x + v.y * v.y) + v.z * v.z;
        ex.alpha[pix] = fminf(fmaxf(expf((-ss) / ex.alpha_den), ex.alpha_eps), 1.01f);
    }
    if (ex.pix_key) ex.pix_key[pix] = ~0ull;
    if (ex.pix_n) ex.pix_n[pix] = ~0u;
    if (vertex) st3(vertex, pix, v);
    if (normal) st3(normal, pix, n);
    if (gvertex || gnormal) {
        if (poses) {
            const float *T = poses + 16 * (int64_t)bl;
            if (gvertex) {
                f3 g = xform(T, v);
                st3(gvertex, pix, f3{g.x * m, g.y * m, g.z * m});
            }
            if (gnormal) {
                st3(gnormal, pix,
                    f3{dot3_fma(T[0], T[1], T[2], n.x, n.y, n.z), dot3_fma(T[4], T[5], T[6], n.x, n.y, n.z),
                       dot3_fma(T[8], T[9], T[10], n.x, n.y, n.z)});
            }
        } else {
            if (gvertex) st3(gvertex, pix, v);
            if (gnormal) st3(gnormal, pix, n);
        }
    }
}

}  // namespace gs
