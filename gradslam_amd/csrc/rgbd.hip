// rgbd.hip -- dense RGB-D odometry: joint photometric + depth alignment of two frames over an image pyramid, coarse to fine
// (gs_rgbd_odometry, gs_rgbd_rows, gs_rgbd_pyramid) and its reverse pass (gs_rgbd_odometry_taped, gs_rgbd_odometry_bwd,
// gs_rgbd_rows_bwd).  The rule -- every fp32 operation in order -- is stated in include/gradslam_hip.h above the entry points;
// the code follows it line by line (the library is built without contraction).  One translation unit, the device code by role:
//   gs_rgbd_pixel.hpp  what forward and reverse kernels must agree on bit for bit, once: the pixel, the pyramid's rules
//   gs_gn_step.hpp     what this loop shares with the SDF odometry's (sdf.hip): constants, the tape and adjoint rows' layout, the
//                      start-up, X the step, Xb its reverse and the fold of the 12-wide rows as whole kernels, host rules and checks
//   gs_rgbd_bwd.hpp    Lb, Pb: the reverse pass's own kernels
//   this file          P, L: the forward's own kernels; the drivers, the workspaces and the C entry points
// P  pyramid: level 0 is (intensity, depth or 0) per pixel as ONE float2, so that a bilinear corner is one 8-byte load; every
//    further level is a 2 x 2 reduction of the level before.  One launch per frame and level.
// L  linearise: one source pixel per lane: warp, four corner loads, the two Jacobian rows and residuals, the lane's 29 terms;
//    a transposing wave butterfly, then the waves in order, leave one partial row per block (gs_icp_reduce.hpp's geometry).
// X  step (gn_step_k): a launch of its own, one 1024-thread block per batch element: reduce_partials (fixed order), then one lane
//    solves (gs::solve6, fp64) and composes T <- exp(xi) T.  Two launches per iteration, no float atomics, nothing synchronises
//    the host; the loop state (T per batch element) lives in the workspace.
#include <math.h>
#include <stddef.h>
#include <algorithm>
#include <type_traits>

#include "gs_gn_step.hpp"  // the loop's shared constants, kernels and host rules
#include "gs_rgbd_pixel.hpp"
#include "gs_rowsum.hpp"  // block_row_transposed

namespace gs {

// ------------------------------------------------------------------ P: pyramid
__global__ __launch_bounds__(256) void rgbd_level0_k(const float *__restrict__ depth, const float *__restrict__ rgb, int64_t n,
                                                    float rgb_scale, float2 *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
    const float I = rgb_scale * ((0.299f * r + 0.587f * g) + 0.114f * b);
    const float d = depth[i];
    out[i] = make_float2(I, rgbd_depth_kept(d) ? d : 0.0f);
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
    const RgbdSel sel = rgbd_down_select(c, ddm);
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if ((sel.taken >> k) & 1) s = s + c[k].y;
    out[(int64_t)blockIdx.y * Hl * Wl + p] = make_float2(I, sel.n > 0 ? s / (float)sel.n : 0.0f);
}

// ------------------------------------------------------------------ L: linearise
// The block's 29 sums -> partials[blockIdx.x]: gs_rowsum.hpp's transposing butterfly (block_row_transposed), in the geometry of
// linearize_k's block row (icp.hip).
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
    float2 s = make_float2(0.0f, 0.0f);  // (a lane past the level's last pixel: depth 0, not valid)
    int v = 0, u = 0;
    if (p < npix) {
        v = p / Wl;
        u = p - v * Wl;
        s = src[(int64_t)b * npix + p];
    }
    RgbdPix P;
    const bool ok = rgbd_pixel_fwd(timg, s, u, v, Hl, Wl, cam, T, ddm, P);
    if (ok) {
        const float gx = cam.fx * P.iz, gy = cam.fy * P.iz;
        const RgbdChan cI = rgbd_chan_row(P.c00.x, P.c10.x, P.c01.x, P.c11.x, P.Is, 0.0f, wI, P, gx, gy);
        const RgbdChan cD = rgbd_chan_row(P.c00.y, P.c10.y, P.c01.y, P.c11.y, P.qz, 1.0f, wD, P, gx, gy);
#pragma unroll
        for (int k = 0; k < 6; ++k) { JI[k] = cI.J[k]; JD[k] = cD.J[k]; }
        rI = cI.r;
        rD = cD.r;
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
    block_row_transposed<NACC, RGBD_T / 64>(acc, partials + (int64_t)b * prow * NACC);
}

}  // namespace gs

#include "gs_rgbd_bwd.hpp"  // Lb, Pb: the reverse pass's own kernels, after the forward ones

namespace gs {

// ------------------------------------------------------------------ host
struct RgbdWs {
    float *T;         // B x 16
    float *partials;  // B x prow x NACC
    float2 *tgt, *src;  // level-major pyramids: level l at + B * off[l] pixels
    int prow;
    int Hl[GN_MAX_LEVELS], Wl[GN_MAX_LEVELS];
    int64_t off[GN_MAX_LEVELS + 1];  // pixels per batch element in the levels before l
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
// The bounds on (B, H, W, levels), once: 0 if the entry points take the shape, else the number of the first bound it breaks, in
// the order RGBD_REQUIRE_SHAPE words them.  A size query returns 0 for a shape that breaks one.
static int rgbd_shape_fault(int B, int H, int W, int levels) {
    if (const int fault = gn_image_fault(B, H, W)) return fault;
    if (!(levels >= 1 && levels <= GN_MAX_LEVELS)) return 4;
    if (!((H >> (levels - 1)) >= GN_MIN_SIDE && (W >> (levels - 1)) >= GN_MIN_SIDE)) return 5;
    return 0;
}
static bool rgbd_shape_ok(int B, int H, int W, int levels) { return rgbd_shape_fault(B, H, W, levels) == 0; }
#define RGBD_REQUIRE_SHAPE(name)                                                                                                  \
    do {                                                                                                                          \
        const int fault__ = rgbd_shape_fault(B, H, W, levels);                                                                    \
        GN_REQUIRE_IMAGE(name, fault__);                                                                                          \
        GS_REQUIRE(fault__ != 4, name ": levels must be in [1, %d], got %d", GN_MAX_LEVELS, levels);                              \
        GS_REQUIRE(fault__ != 5, name ": the coarsest of %d levels of a %d x %d image would be smaller than 4 x 4", levels, H, W); \
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
    float *adj;         // max(iterations, 1) x B x GN_ADJ_WORDS, in the order the iterations ran
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
    t.adj = c.take<float>(sizeof(float) * GN_ADJ_WORDS * (size_t)std::max<int64_t>(iterations, 1) * B);
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
    gn_launch_step(B, w.T, w.partials, w.prow, w.prow, 0.0f, 0, 1, 0, 0, nullptr, nullptr, sums, nullptr, st);
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
    gn_launch_init(init, B, levels, w.T, out_T, info, st);
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
            gn_launch_step(B, w.T, w.partials, nblocks, w.prow, damp, l, levels, it, 1, out_T, info, nullptr, rec, st);
            GS_LAUNCH_CHECK("gs_rgbd_odometry/step");
            if (tape) rec += (size_t)GN_TAPE_WORDS * B;
        }
    }
    return 0;
}

// The reverse pass, for both of its entry points (`nm`: the entry point's launch names).  The loop (gs_rgbd_odometry_bwd): per
// level, finest first, its iterations last to first -- Xb, then Lb<MAX> at the tape row's T -- then, if a target gradient is wanted,
// Lb<ACC> over the same iterations and the level's finish.  The seam (gs_rgbd_rows_bwd, `tape` NULL) is that with one level, one
// iteration, the caller's `T` (B,16) and the adjoints of `g_sums` for the tape row and Xb, and a 12-wide g_T for the 16-wide g_init.
struct RgbdBwdNames { const char *op, *pyramid, *begin, *zero, *step, *pixels, *corners, *finish, *last, *target, *source; };
#define RGBD_BWD_NAMES(op, begin, last) \
    RgbdBwdNames { op, op "/pyramid", op begin, op "/zero", op "/step", op "/pixels", op "/corners", op "/finish", op last, op "/target", op "/source" }
// the adjoint pyramids, coarsest to finest, then level 0 into the images; either output may be NULL
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
static int rgbd_bwd_run(const RgbdBwdNames &nm, const float *tgt_depth, const float *tgt_rgb, const float *src_depth, const float *src_rgb,
                        int B, int H, int W, const float *intrinsics, int levels, const int *numiters, float lambda_geo, float ddm, float damp,
                        float rgb_scale, const float *tape, const float *grad_T, const float *T, const float *g_sums, float *g_tgt_depth,
                        float *g_tgt_rgb, float *g_src_depth, float *g_src_rgb, float *g_T, void *ws, size_t ws_bytes, hipStream_t st) {
    const bool seam = !tape;
    const GnSchedule sch = gn_schedule(levels, numiters);
    const size_t need = gs_rgbd_odometry_bwd_ws_size(B, H, W, levels, sch.total);
    GS_REQUIRE_WS(nm.op, ws, ws_bytes, need);
    RgbdBwdWs w;
    rgbd_bwd_layout(B, H, W, levels, sch.total, ws, &w);
    // both pyramids again (the forward's workspace need not have survived), the adjoint pyramids zeroed
    int rc = rgbd_build_pyramid(nm.pyramid, tgt_depth, tgt_rgb, B, levels, w.f, ddm, rgb_scale, w.f.tgt, st);
    if (rc) return rc;
    rc = rgbd_build_pyramid(nm.pyramid, src_depth, src_rgb, B, levels, w.f, ddm, rgb_scale, w.f.src, st);
    if (rc) return rc;
    GS_HIP(hipMemsetAsync(w.gtgt, 0, w.adj_pyr_bytes, st), nm.pyramid);  // gtgt | gsrc
    if (!seam) {
        hipLaunchKernelGGL(gn_fold12_k, dim3(B), dim3(BWD_T), 0, st, grad_T, (const float *)nullptr, 0, w.f.prow, w.gT, 16);
        GS_LAUNCH_CHECK(nm.begin);
    }
    const float wI = sqrtf(1.0f - lambda_geo), wD = sqrtf(lambda_geo);
    int prev_nblocks = 0;  // rows the pixel pass before left for the next step's fold
    // without a target gradient nothing reads the corner sums: no fold (only its maximum's word, which <MAX> touches, is zeroed)
    const bool want_tgt = g_tgt_depth || g_tgt_rgb;
    for (int l = 0; l < levels; ++l) {
        const int n = numiters[l];
        if (n == 0) continue;
        const int lg = fold_lg((int64_t)w.f.Hl[l] * w.f.Wl[l] * n);  // a corner receives at most one term per source pixel and iteration
        GS_HIP(hipMemsetAsync(w.fold_base, 0, want_tgt ? w.fold_bytes : sizeof(uint32_t), st), nm.zero);
        if (seam) {
            hipLaunchKernelGGL(gn_sums_adj_k, dim3(cdiv((int64_t)B * GN_ADJ_WORDS, 256)), dim3(256), 0, st, g_sums, B, w.adj);
            GS_LAUNCH_CHECK(nm.begin);
        }
        const int nblocks = cdiv((int64_t)w.f.Hl[l] * w.f.Wl[l], RGBD_T);
        // iteration `it`'s transform (the seam's T, or the head of its tape row) and the adjoints of its sums
        const auto T_of = [&](int it) { return seam ? T : tape + (size_t)(sch.base[l] + it) * B * GN_TAPE_WORDS; };
        const auto adj_of = [&](int it) { return w.adj + (size_t)(sch.base[l] + it) * B * GN_ADJ_WORDS; };
        const auto pixels = [&](decltype(&rgbd_pixel_bwd_k<RGBD_BWD_MAX>) kernel, const char *name, int it) {
            hipLaunchKernelGGL(kernel, dim3(nblocks, B), dim3(RGBD_T), 0, st, (const float2 *)(w.f.tgt + B * w.f.off[l]),
                               (const float2 *)(w.f.src + B * w.f.off[l]), w.f.Hl[l], w.f.Wl[l], l, intrinsics, T_of(it),
                               seam ? 16 : GN_TAPE_WORDS, (const float *)adj_of(it), wI, wD, ddm, w.fold, lg, w.gsrc + B * w.f.off[l],
                               w.partials12, w.f.prow);
            GS_LAUNCH_CHECK(name);
            return 0;
        };
        for (int it = n - 1; it >= 0; --it) {
            if (!seam) {
                hipLaunchKernelGGL(gn_step_bwd_k<false>, dim3(B), dim3(BWD_T), 0, st, w.gT, (const float *)w.partials12, prev_nblocks, w.f.prow,
                                   T_of(it), damp, adj_of(it), (float *)nullptr, (const float *)nullptr);
                GS_LAUNCH_CHECK(nm.step);
            }
            if ((rc = pixels(rgbd_pixel_bwd_k<RGBD_BWD_MAX>, nm.pixels, it))) return rc;
            prev_nblocks = nblocks;
        }
        if (!want_tgt) continue;
        for (int it = n - 1; it >= 0; --it)
            if ((rc = pixels(rgbd_pixel_bwd_k<RGBD_BWD_ACC>, nm.corners, it))) return rc;
        const int64_t npix = (int64_t)B * w.f.Hl[l] * w.f.Wl[l];
        hipLaunchKernelGGL(rgbd_fold_finish_k, dim3(cdiv(npix, 256)), dim3(256), 0, st, w.fold, lg, npix, w.gtgt + B * w.f.off[l]);
        GS_LAUNCH_CHECK(nm.finish);
    }
    if (g_T) {  // the carried adjoint (the seam has none) + what the last pixel pass left: g_init (B,16), or the seam's g_T (B,12)
        hipLaunchKernelGGL(gn_fold12_k, dim3(B), dim3(BWD_T), 0, st, seam ? (const float *)nullptr : (const float *)w.gT,
                           (const float *)w.partials12, prev_nblocks, w.f.prow, g_T, seam ? 12 : 16);
        GS_LAUNCH_CHECK(nm.last);
    }
    rc = rgbd_pyramid_bwd(nm.target, tgt_depth, w.f.tgt, w.gtgt, B, levels, w.f, ddm, rgb_scale, g_tgt_depth, g_tgt_rgb, st);
    if (rc) return rc;
    return rgbd_pyramid_bwd(nm.source, src_depth, w.f.src, w.gsrc, B, levels, w.f, ddm, rgb_scale, g_src_depth, g_src_rgb, st);
}

extern "C" {

#define RGBD_REQUIRE_ODOMETRY(name)                                                                                               \
    do {                                                                                                                          \
        RGBD_REQUIRE_SHAPE(name);                                                                                                 \
        RGBD_REQUIRE_LAMBDA(name);                                                                                                \
        RGBD_REQUIRE_PARAMS(name);                                                                                                \
        GN_REQUIRE_LOOP(name);                                                                                                    \
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
    if (B < 1 || B > 65535 || levels < 1 || levels > GN_MAX_LEVELS || !gn_total_ok(levels, numiters)) return 0;
    return one_piece_bytes(sizeof(float) * GN_TAPE_WORDS * (size_t)std::max(numiters, 1) * B);
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
    if (!rgbd_shape_ok(B, H, W, levels) || !gn_total_ok(levels, numiters)) return 0;
    return rgbd_bwd_layout(B, H, W, levels, numiters, nullptr, nullptr);
}

int gs_rgbd_odometry_bwd(const float *tgt_depth, const float *tgt_rgb, const float *src_depth, const float *src_rgb, int B, int H, int W,
                         const float *intrinsics, int levels, const int *numiters, float lambda_geo, float depth_diff_max, float damp,
                         float rgb_scale, const float *tape, const float *grad_T, float *g_tgt_depth, float *g_tgt_rgb, float *g_src_depth,
                         float *g_src_rgb, float *g_init, void *ws, size_t ws_bytes, gs_stream_t stream) {
    GS_REQUIRE(tgt_depth && tgt_rgb && src_depth && src_rgb && intrinsics && numiters && tape && grad_T, "gs_rgbd_odometry_bwd: null pointer");
    RGBD_REQUIRE_ODOMETRY("gs_rgbd_odometry_bwd");
    return rgbd_bwd_run(RGBD_BWD_NAMES("gs_rgbd_odometry_bwd", "/begin", "/init"), tgt_depth, tgt_rgb, src_depth, src_rgb, B, H, W, intrinsics,
                        levels, numiters, lambda_geo, depth_diff_max, damp, rgb_scale, tape, grad_T, nullptr, nullptr, g_tgt_depth, g_tgt_rgb,
                        g_src_depth, g_src_rgb, g_init, ws, ws_bytes, (hipStream_t)stream);
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
    const int one = 1;  // one level, one iteration
    return rgbd_bwd_run(RGBD_BWD_NAMES("gs_rgbd_rows_bwd", "/adjoints", "/transform"), tgt_depth, tgt_rgb, src_depth, src_rgb, B, H, W, intrinsics,
                        levels, &one, lambda_geo, depth_diff_max, 0.0f, rgb_scale, nullptr, nullptr, T, g_sums, g_tgt_depth, g_tgt_rgb,
                        g_src_depth, g_src_rgb, g_T, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
