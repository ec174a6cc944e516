// gs_fusion_row.hpp -- the PointFusion row algebra, each formula stated ONCE (device code, force-inlined).
//
// fusion.hip's kernels keep their own loads, phases and stores; what they compute between a load and a store is here:
// the similarity test (slam/fusionutils.py:381-401), the uniqueness key (:489-546) and the confidence-weighted merge
// with its adjoint (:654-699).  The reference's rounding is part of its observable result, so every expression is
// written in the reference's order and nothing is fused that the reference does not fuse (the library is built with
// -ffp-contract=off):
//   (a - b).norm(dim=-1)    sqrt(fma(z, z, fma(y, y, x * x)))
//   (a * b).sum(-1)         (x + y) + z, unfused
//   1 / (c + 1e-20)         a true division
//   the merge               the two products, their sum, then ONE multiplication by inv = 1 / where(c2 == 0, 1, c2),
//                           c2 = c + a: no division per component and no fma
// Every map point goes through the merge, matched or not: an unmatched point becomes (c*x + 0*0) * (1/c), which is NOT
// bit-identical to x -- fusionutils.py:678-699 operate on the whole padded tensors.
#pragma once

#include "gs_common.hpp"

namespace gs {

struct MapRow {  // one map point: position, normal, colour, confidence count
    f3 x, y, z;
    float c;
};
struct FrameRow {  // what the frame holds at one pixel: global vertex, normal, colour, alpha.  FrameRow{} = "unmatched"
    f3 p{0, 0, 0}, n{0, 0, 0}, c{0, 0, 0};
    float a = 0.0f;
};

// "matched: load, else zeros"
__device__ __forceinline__ FrameRow gather_frame(bool match, int64_t pix, const float *gv, const float *gn,
                                                 const float *rgb, const float *alpha) {
    FrameRow f;
    if (match) { f.a = alpha[pix]; f.p = ld3(gv, pix); f.n = ld3(gn, pix); f.c = ld3(rgb, pix); }
    return f;
}

// the tape's record of a map row: 10 floats
__device__ __forceinline__ MapRow ld_row10(const float *rec, int64_t i) {
    const float *o = rec + 10 * i;
    return MapRow{f3{o[0], o[1], o[2]}, f3{o[3], o[4], o[5]}, f3{o[6], o[7], o[8]}, o[9]};
}
__device__ __forceinline__ void st_row10(float *rec, int64_t i, MapRow r) {
    float *o = rec + 10 * i;
    o[0] = r.x.x; o[1] = r.x.y; o[2] = r.x.z; o[3] = r.y.x; o[4] = r.y.y; o[5] = r.y.z; o[6] = r.z.x; o[7] = r.z.y; o[8] = r.z.z; o[9] = r.c;
}

// ------------------------------------------------------------------ C: is map point (p, q) similar to the frame's (fv, fn)?
__device__ __forceinline__ bool similar_pair(f3 fv, f3 fn, f3 p, f3 q, float dist_th, float dot_th, float &dot) {
    const float dx = fv.x - p.x, dy = fv.y - p.y, dz = fv.z - p.z;
    const float dist = sqrtf(__fmaf_rn(dz, dz, __fmaf_rn(dy, dy, dx * dx)));
    const float d = dot3_plain(fn.x, fn.y, fn.z, q.x, q.y, q.z);
    dot = d;  // (the test reads the local: read back through the reference, the callers' fmaxf(md, dot) gains a canonicalising v_max)
    return dist < dist_th && d > dot_th;
}

// ------------------------------------------------------------------ U: key = (1/(c + 1e-20), squared ray distance) as
// order-preserving bits (both are >= +0); the smallest key wins the pixel
__device__ __forceinline__ unsigned long long unique_key(float c, f3 p, f3 fv) {
    const float inv_c = 1.0f / (c + 1e-20f);
    const float dx = p.x - fv.x, dy = p.y - fv.y, dz = p.z - fv.z;
    return ((unsigned long long)fbits(inv_c) << 32) | fbits(dot3_plain(dx, dy, dz, dx, dy, dz));
}

// ------------------------------------------------------------------ F: running average of a map row with a frame row
// The weights of one merge: the one statement of the c2 == 0 rule (inv takes the constant 1 there, and its derivative
// dinv is 0) and of the blend.  A kernel that loads its row piecewise builds the weights first and blends as it goes.
struct MergeW {
    float c, a, c2, inv, dinv;
    __device__ __forceinline__ MergeW(float c_, float a_)
        : c(c_), a(a_), c2(c_ + a_), inv(1.0f / (c2 == 0.0f ? 1.0f : c2)), dinv((c2 == 0.0f) ? 0.0f : 1.0f) {}
    __device__ __forceinline__ f3 avg(f3 x, f3 v) const {
        return f3{((c * x.x) + (a * v.x)) * inv, ((c * x.y) + (a * v.y)) * inv, ((c * x.z) + (a * v.z)) * inv};
    }
    // the adjoint's pieces.  x' = (c x + a xf) / c2 (c2 != 0):
    //   x_bar = (c/c2) x'_bar ; xf_bar = (a/c2) x'_bar ; c_bar = c2_bar + sum (x - x').x'_bar / c2 ;
    //   a_bar = c2_bar + sum (xf - x').x'_bar / c2      (sums over points, normals, colours: merge_sums)
    // d x'/d c2 = -(c x + a xf) inv^2 = -x' inv: zero when c2 == 0, where the where() picks the constant 1.
    __device__ __forceinline__ f3 map_bar(f3 g) const { return f3{c * inv * g.x, c * inv * g.y, c * inv * g.z}; }
    __device__ __forceinline__ f3 frame_bar(f3 g) const { return f3{a * inv * g.x, a * inv * g.y, a * inv * g.z}; }
    __device__ __forceinline__ float weight_bar(float c2_bar, float s, float s_out) const {  // s = sum x.x'_bar (c_bar) or sum xf.x'_bar (a_bar)
        return c2_bar + (s - dinv * s_out) * inv;
    }
};

// the adjoint's three sums over points, normals and colours: x'.x'_bar, x.x'_bar and xf.x'_bar
struct MergeSums {
    float out, in, f;
};
__device__ __forceinline__ MergeSums merge_sums(const MergeW &w, const MapRow &in, const FrameRow &f, const MapRow &g) {
    const auto dot = [&](f3 x, f3 y, f3 z) {
        return dot3_plain(x.x, x.y, x.z, g.x.x, g.x.y, g.x.z) + dot3_plain(y.x, y.y, y.z, g.y.x, g.y.y, g.y.z) +
               dot3_plain(z.x, z.y, z.z, g.z.x, g.z.y, g.z.z);
    };
    return MergeSums{dot(w.avg(in.x, f.p), w.avg(in.y, f.n), w.avg(in.z, f.c)), dot(in.x, in.y, in.z), dot(f.p, f.n, f.c)};
}

}  // namespace gs
