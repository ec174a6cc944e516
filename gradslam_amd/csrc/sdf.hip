// sdf.hip -- SDF odometry: a camera tracked directly against the TSDF volume (gs_sdf_odometry, gs_sdf_rows).  Gauss-Newton on
// sum phi(D P p)^2 over the frame's pixels, phi the volume's interpolated distance: no ray cast, no association, no cloud.  The
// rule -- every fp32 operation in order -- is stated in include/gradslam_hip.h above the entry points; the code follows it line
// by line (the library is built without contraction).
//   gs_sdf_pixel.hpp  the pixel, once: back-projection, the gates in their order, the row
//   gs_gn_step.hpp    what this loop shares with the RGB-D odometry's (rgbd.hip): constants, the tape and adjoint rows' layout, the
//                     start-up, X the step, Xb its reverse and the fold of the 12-wide rows as whole kernels, host rules and checks
//   gs_sdf_bwd.hpp    Lb: the reverse pass's own kernels (gs_sdf_odometry_taped, gs_sdf_odometry_bwd, gs_sdf_rows_bwd)
//   this file         L: the forward's own kernel; the drivers, the workspace, the tape, the room and the C entry points
// L  linearise: one pixel of the level's grid per lane: depth, two transforms, the cell, 16 gathers in one batch, the row, the
//    lane's 29 terms; gs_rowsum.hpp's transposing butterfly leaves one partial row per block.
// X  step (gn_step_k): one 1024-thread block per batch element: reduce_partials (fixed order), then one lane solves (gs::solve6,
//    fp64) and composes D <- exp(xi) D.  Two launches per iteration plus one to start, no float atomics, nothing synchronises the host; the
//    loop state (D per batch element) lives in the workspace.
#include <math.h>
#include <stddef.h>
#include <algorithm>

#include "gs_gn_step.hpp"  // the loop's shared constants, kernels and host rules
#include "gs_sdf_pixel.hpp"

namespace gs {

constexpr int SDF_T = LIN_T;  // lanes (= pixels) per linearise block

// what a level's grid is: pixels (i s, j s) of the H x W image, Hs x Ws of them
struct SdfGrid { int H, W, s, Hs, Ws; };
// the volume as the kernels take it (origin: (B,3); tsdf, weight: (B, nz, ny, nx))
struct SdfVolume {
    const float *tsdf, *weight, *origin;
    int nx, ny, nz;
    float v, trunc, kappa, minw;
};

// ------------------------------------------------------------------ L: linearise
// grid (blocks of SDF_T pixels of the level's grid, B).  K (B,16), P (B,16), Dall (B,16).  partials: row blockIdx.x of batch
// element b at partials + (b * prow + blockIdx.x) * NACC.  ROWS: also the per-pixel valid flag and the 7 floats J | r (zeros
// where not valid).
template <bool ROWS>
__global__ __launch_bounds__(SDF_T) void sdf_linearize_k(const float *__restrict__ depth, SdfGrid gr, const float *__restrict__ K,
                                                        const float *__restrict__ Pall, const float *__restrict__ Dall, SdfVolume vo,
                                                        float *__restrict__ partials, int prow, int32_t *__restrict__ valid,
                                                        float *__restrict__ rows) {
    const int b = blockIdx.y, npix = gr.Hs * gr.Ws;
    const int p = blockIdx.x * SDF_T + threadIdx.x;
    const SdfCam cam = sdf_cam(K + 16 * b);
    const TsdfVol vol{vo.nx, vo.ny, vo.nz, vo.v, vo.trunc, 0.0f, vo.origin + 3 * b};
    const int64_t nvox = tsdf_nvox(vol);

    float d = 0.0f;  // (a lane past the grid's last pixel: depth 0, not valid)
    int h = 0, w = 0;
    if (p < npix) {
        const int i = p / gr.Ws, j = p - i * gr.Ws;
        h = i * gr.s;
        w = j * gr.s;
        d = depth[((int64_t)b * gr.H + h) * gr.W + w];
    }
    SdfPix X;
    const bool ok = sdf_pixel_fwd(d, h, w, cam, Pall + 16 * b, Dall + 16 * b, vol, vo.tsdf + b * nvox, vo.weight + b * nvox, vo.minw,
                                  vo.kappa, X);
    float J[6], r = ok ? X.r : 0.0f;
#pragma unroll
    for (int k = 0; k < 6; ++k) J[k] = ok ? X.J[k] : 0.0f;
    if (ROWS && p < npix) {
        const int64_t o = (int64_t)b * npix + p;
        valid[o] = ok ? 1 : 0;
        float *out = rows + 7 * o;
#pragma unroll
        for (int k = 0; k < 6; ++k) out[k] = J[k];
        out[6] = r;
    }
    // the lane's 29 terms: upper triangle of J^T J | J^T r | r^2 | 1
    float acc[32];
    int q = 0;
#pragma unroll
    for (int m = 0; m < 6; ++m)
#pragma unroll
        for (int n = m; n < 6; ++n) acc[q++] = J[m] * J[n];
#pragma unroll
    for (int m = 0; m < 6; ++m) acc[21 + m] = J[m] * r;
    acc[27] = r * r;
    acc[28] = ok ? 1.0f : 0.0f;
    acc[29] = 0.0f; acc[30] = 0.0f; acc[31] = 0.0f;
    block_row_transposed<NACC, SDF_T / 64>(acc, partials + (int64_t)b * prow * NACC);
}

}  // namespace gs

#include "gs_sdf_bwd.hpp"  // Lb: the reverse pass's own kernels, after the forward one

namespace gs {

// ------------------------------------------------------------------ host
static SdfGrid sdf_grid(int H, int W, int stride, int level) {
    const int s = stride << level;
    return SdfGrid{H, W, s, cdiv(H, s), cdiv(W, s)};
}
struct SdfWs {
    float *D;         // B x 16
    float *partials;  // B x prow x NACC
    int prow;         // partial rows of level 0, the largest grid
};
// the loop's state, which opens the workspace and the tape alike
static SdfWs sdf_carve_loop(Carve &c, int B, int H, int W, int stride) {
    SdfWs t;
    const SdfGrid g = sdf_grid(H, W, stride, 0);
    t.prow = cdiv((int64_t)g.Hs * g.Ws, SDF_T);
    t.D = c.take<float>(sizeof(float) * 16 * B);
    t.partials = c.take<float>(sizeof(float) * NACC * (size_t)t.prow * B);
    return t;
}
static size_t sdf_layout(int B, int H, int W, int stride, void *ws, SdfWs *w) {
    Carve c{(char *)ws};
    const SdfWs t = sdf_carve_loop(c, B, H, W, stride);
    if (w) *w = t;
    return c.off;
}
// the taped forward's buffer: the loop's state, then one tape row per (iteration, batch element) in the order the iterations run
struct SdfTape {
    SdfWs f;
    float *rows;  // max(iterations, 1) x B x GN_TAPE_WORDS
};
static size_t sdf_tape_layout(int B, int H, int W, int stride, int64_t iterations, void *tape, SdfTape *out) {
    Carve c{(char *)tape};
    SdfTape t;
    t.f = sdf_carve_loop(c, B, H, W, stride);
    t.rows = c.take<float>(sizeof(float) * GN_TAPE_WORDS * (size_t)std::max<int64_t>(iterations, 1) * B);
    if (out) *out = t;
    return c.off;
}
// the reverse pass's working memory; without a volume adjoint there is no fold (fold.maxbits is NULL)
struct SdfRoom {
    float *gD, *gP;        // B x 16 each: the carried adjoint of D, the running adjoint of the poses
    float *adj;            // max(iterations, 1) x B x GN_ADJ_WORDS, in the order the iterations ran
    float *partD, *partP;  // B x prow x 12 each
    int prow;
    Fold fold;             // B nx ny nz rows x 1 channel
    void *fold_base;
    size_t fold_bytes;
};
static size_t sdf_room_layout(int B, int H, int W, int stride, int64_t iterations, int64_t nvox, bool want_tsdf, void *room, SdfRoom *out) {
    Carve c{(char *)room};
    SdfRoom t;
    const SdfGrid g = sdf_grid(H, W, stride, 0);
    t.prow = cdiv((int64_t)g.Hs * g.Ws, SDF_T);
    t.gD = c.take<float>(sizeof(float) * 16 * B);
    t.gP = c.take<float>(sizeof(float) * 16 * B);
    t.adj = c.take<float>(sizeof(float) * GN_ADJ_WORDS * (size_t)std::max<int64_t>(iterations, 1) * B);
    t.partD = c.take<float>(sizeof(float) * 12 * (size_t)t.prow * B);
    t.partP = c.take<float>(sizeof(float) * 12 * (size_t)t.prow * B);
    t.fold = Fold{nullptr, nullptr, nullptr, 1};
    t.fold_base = nullptr;
    t.fold_bytes = 0;
    if (want_tsdf) {
        const size_t before = c.off;
        t.fold = fold_carve(c, (size_t)B * nvox, 1);
        t.fold_base = t.fold.maxbits;
        t.fold_bytes = c.off - before;
    }
    if (out) *out = t;
    return c.off;
}
// The bounds on (B, H, W, stride, levels), once: 0 if the entry points take the shape, else the number of the first bound it
// breaks, in the order SDF_REQUIRE_SHAPE words them.  A size query returns 0 for a shape that breaks one.
static int sdf_shape_fault(int B, int H, int W, int stride, int levels) {
    if (const int fault = gn_image_fault(B, H, W)) return fault;
    if (!(stride >= 1)) return 4;
    if (!(levels >= 1 && levels <= GN_MAX_LEVELS)) return 5;
    const int64_t s = (int64_t)stride << (levels - 1);  // (stride < 2^31, levels <= 8: no overflow)
    if (!((H + s - 1) / s >= GN_MIN_SIDE && (W + s - 1) / s >= GN_MIN_SIDE)) return 6;
    return 0;
}
static bool sdf_pos(float x) { return x > 0.0f && x < INFINITY; }
#define SDF_REQUIRE_SHAPE(name)                                                                                                    \
    do {                                                                                                                           \
        const int fault__ = sdf_shape_fault(B, H, W, stride, levels);                                                              \
        GN_REQUIRE_IMAGE(name, fault__);                                                                                           \
        GS_REQUIRE(fault__ != 4, name ": stride must be at least 1, got %d", stride);                                              \
        GS_REQUIRE(fault__ != 5, name ": levels must be in [1, %d], got %d", GN_MAX_LEVELS, levels);                               \
        GS_REQUIRE(fault__ != 6, name ": the coarsest of %d grids of a %d x %d image at stride %d would be smaller than 4 x 4",    \
                   levels, H, W, stride);                                                                                          \
    } while (0)
#define SDF_REQUIRE_VOLUME(name)                                                                                                   \
    do {                                                                                                                           \
        GS_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1 && (int64_t)nx * ny * nz <= TSDF_NMAX,                                            \
                   name ": bad volume dims=(%d, %d, %d) (positive, nx ny nz <= 2^29)", nx, ny, nz);                                \
        GS_REQUIRE(sdf_pos(voxel_size), name ": voxel_size must be finite and positive, got %g", (double)voxel_size);              \
        GS_REQUIRE(sdf_pos(trunc), name ": trunc must be finite and positive, got %g", (double)trunc);                             \
        GS_REQUIRE(min_weight == min_weight, name ": min_weight must be a number");                                                \
    } while (0)

static void sdf_launch_linearize(bool rows_out, const float *depth, int B, const SdfGrid &g, const float *K, const float *P, const float *D,
                                 const SdfVolume &vo, const SdfWs &w, int32_t *valid, float *rows, hipStream_t st) {
    const int nblocks = cdiv((int64_t)g.Hs * g.Ws, SDF_T);
    if (rows_out)
        hipLaunchKernelGGL(sdf_linearize_k<true>, dim3(nblocks, B), dim3(SDF_T), 0, st, depth, g, K, P, D, vo, w.partials, w.prow, valid, rows);
    else
        hipLaunchKernelGGL(sdf_linearize_k<false>, dim3(nblocks, B), dim3(SDF_T), 0, st, depth, g, K, P, D, vo, w.partials, w.prow,
                           (int32_t *)nullptr, (float *)nullptr);
}

}  // namespace gs

using namespace gs;

extern "C" {

size_t gs_sdf_odometry_ws_size(int B, int H, int W, int stride) {
    if (sdf_shape_fault(B, H, W, stride, 1) != 0) return 0;
    return sdf_layout(B, H, W, stride, nullptr, nullptr);
}

int gs_sdf_rows(const float *depth, int B, int H, int W, const float *intrinsics, const float *poses, const float *D, const float *tsdf,
                const float *weight, int nx, int ny, int nz, const float *origin, float voxel_size, float trunc, float min_weight,
                int stride, int32_t *valid, float *rows, float *sums, void *ws, size_t ws_bytes, gs_stream_t stream) {
    GS_REQUIRE(depth && intrinsics && poses && D && tsdf && weight && origin && valid && rows && sums, "gs_sdf_rows: null pointer");
    const int levels = 1;
    SDF_REQUIRE_SHAPE("gs_sdf_rows");
    SDF_REQUIRE_VOLUME("gs_sdf_rows");
    const size_t need = gs_sdf_odometry_ws_size(B, H, W, stride);
    GS_REQUIRE_WS("gs_sdf_rows", ws, ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    SdfWs w;
    sdf_layout(B, H, W, stride, ws, &w);
    const SdfVolume vo{tsdf, weight, origin, nx, ny, nz, voxel_size, trunc, trunc / voxel_size, min_weight};
    sdf_launch_linearize(true, depth, B, sdf_grid(H, W, stride, 0), intrinsics, poses, D, vo, w, valid, rows, st);
    GS_LAUNCH_CHECK("gs_sdf_rows/linearize");
    gn_launch_step(B, w.D, w.partials, w.prow, w.prow, 0.0f, 0, 1, 0, 0, nullptr, nullptr, sums, nullptr, st);
    GS_LAUNCH_CHECK("gs_sdf_rows/sums");
    return 0;
}

}  // extern "C"

// gs_sdf_odometry (rec = NULL) and gs_sdf_odometry_taped: one loop, the same launches
static int sdf_run(const float *depth, int B, int H, int W, const float *intrinsics, const float *poses, const float *init,
                   const SdfVolume &vo, int stride, int levels, const int *numiters, float damp, float *out_T, float *info, const SdfWs &w,
                   float *rec, hipStream_t st) {
    gn_launch_init(init, B, levels, w.D, out_T, info, st);
    GS_LAUNCH_CHECK("gs_sdf_odometry/init");
    for (int l = levels - 1; l >= 0; --l) {
        const SdfGrid g = sdf_grid(H, W, stride, l);
        const int nblocks = cdiv((int64_t)g.Hs * g.Ws, SDF_T);
        for (int it = 0; it < numiters[l]; ++it) {
            sdf_launch_linearize(false, depth, B, g, intrinsics, poses, w.D, vo, w, nullptr, nullptr, st);
            GS_LAUNCH_CHECK("gs_sdf_odometry/linearize");
            gn_launch_step(B, w.D, w.partials, nblocks, w.prow, damp, l, levels, it, 1, out_T, info, nullptr, rec, st);
            GS_LAUNCH_CHECK("gs_sdf_odometry/step");
            if (rec) rec += (size_t)GN_TAPE_WORDS * B;  // one row per (iteration, batch element), in the order the iterations run
        }
    }
    return 0;
}

#define SDF_REQUIRE_ROOM(name, ptr, have, need) GS_REQUIRE_BYTES_("room", GS_ERR_WORKSPACE_TOO_SMALL, name, ptr, have, need)
static bool sdf_dims_ok(int nx, int ny, int nz) { return nx >= 1 && ny >= 1 && nz >= 1 && (int64_t)nx * ny * nz <= TSDF_NMAX; }

// The reverse pass, for both of its entry points (`nm`: the entry point's launch names).  The loop (gs_sdf_odometry_bwd): the
// levels finest first, each level's iterations last to first -- Xb, then Lb<MAX> at the tape row's D -- then, if the volume's
// gradient is wanted, Lb<ACC> over the same iterations at the kept adjoint rows and one finish.  The seam (gs_sdf_rows_bwd,
// `rows` NULL) is that with one level, one iteration, the caller's `D` (B,16) and the adjoints of `g_sums` for the tape row and
// Xb, and 12-wide g_poses and g_D for the loop's 16-wide g_poses and g_init.
struct SdfBwdNames { const char *op, *zero, *begin, *step, *pixels, *corners, *finish, *last; };
#define SDF_BWD_NAMES(op, begin) SdfBwdNames { op, op "/zero", op begin, op "/step", op "/pixels", op "/corners", op "/finish", op "/last" }
static int sdf_bwd_run(const SdfBwdNames &nm, const float *depth, int B, int H, int W, const float *intrinsics, const float *poses,
                       const SdfVolume &vo, int stride, int levels, const int *numiters, float damp, const float *rows, const float *grad_T,
                       const float *D, const float *g_sums, float *g_depth, float *g_poses, float *g_D, float *g_tsdf, void *room,
                       size_t room_cap, hipStream_t st) {
    const bool seam = !rows, want_tsdf = g_tsdf != nullptr;
    const GnSchedule sch = gn_schedule(levels, numiters);
    int64_t terms = 0;  // a pixel gives a voxel at most one term per iteration
    for (int l = 0; l < levels; ++l) {
        const SdfGrid g = sdf_grid(H, W, stride, l);
        terms += (int64_t)numiters[l] * g.Hs * g.Ws;
    }
    const int64_t nvox = (int64_t)vo.nx * vo.ny * vo.nz;
    const size_t need = sdf_room_layout(B, H, W, stride, sch.total, nvox, want_tsdf, nullptr, nullptr);
    SDF_REQUIRE_ROOM(nm.op, room, room_cap, need);
    SdfRoom w;
    sdf_room_layout(B, H, W, stride, sch.total, nvox, want_tsdf, room, &w);
    if (g_depth) GS_HIP(hipMemsetAsync(g_depth, 0, sizeof(float) * (size_t)B * H * W, st), nm.zero);
    if (want_tsdf) GS_HIP(hipMemsetAsync(w.fold_base, 0, w.fold_bytes, st), nm.zero);
    if (seam) {
        hipLaunchKernelGGL(gn_sums_adj_k, dim3(cdiv((int64_t)B * GN_ADJ_WORDS, 256)), dim3(256), 0, st, g_sums, B, w.adj);
    } else {
        hipLaunchKernelGGL(sdf_bwd_begin_k, dim3(cdiv(16 * B, 256)), dim3(256), 0, st, grad_T, B, w.gD, w.gP);
    }
    GS_LAUNCH_CHECK(nm.begin);
    const int lg = fold_lg(std::max<int64_t>(terms, 1));
    float *partP = g_poses ? w.partP : nullptr;
    int prev_nblocks = 0;  // rows the pixel pass before left for the next step's fold
    // iteration `it` of level l: its delta (the seam's D, or the head of its tape row) and the adjoints of its sums
    const auto D_of = [&](int l, int it) { return seam ? D : rows + (size_t)(sch.base[l] + it) * B * GN_TAPE_WORDS; };
    const auto adj_of = [&](int l, int it) { return w.adj + (size_t)(sch.base[l] + it) * B * GN_ADJ_WORDS; };
    const auto pixels = [&](decltype(&sdf_pixel_bwd_k<SDF_BWD_MAX>) kernel, const char *name, int l, int it) {
        const SdfGrid g = sdf_grid(H, W, stride, l);
        hipLaunchKernelGGL(kernel, dim3(cdiv((int64_t)g.Hs * g.Ws, SDF_T), B), dim3(SDF_T), 0, st, depth, g, intrinsics, poses, D_of(l, it),
                           seam ? 16 : GN_TAPE_WORDS, vo, (const float *)adj_of(l, it), w.fold, lg, g_depth, w.partD, partP, w.prow);
        GS_LAUNCH_CHECK(name);
        return 0;
    };
    int rc;
    for (int l = 0; l < levels; ++l) {
        const SdfGrid g = sdf_grid(H, W, stride, l);
        const int nblocks = cdiv((int64_t)g.Hs * g.Ws, SDF_T);
        for (int it = numiters[l] - 1; it >= 0; --it) {
            if (!seam) {
                hipLaunchKernelGGL(gn_step_bwd_k<true>, dim3(B), dim3(BWD_T), 0, st, w.gD, (const float *)w.partD, prev_nblocks, w.prow,
                                   D_of(l, it), damp, adj_of(l, it), w.gP, (const float *)partP);
                GS_LAUNCH_CHECK(nm.step);
            }
            if ((rc = pixels(sdf_pixel_bwd_k<SDF_BWD_MAX>, nm.pixels, l, it))) return rc;
            prev_nblocks = nblocks;
        }
    }
    if (want_tsdf) {
        for (int l = 0; l < levels; ++l)
            for (int it = numiters[l] - 1; it >= 0; --it)
                if ((rc = pixels(sdf_pixel_bwd_k<SDF_BWD_ACC>, nm.corners, l, it))) return rc;
        const int64_t n = (int64_t)B * nvox;
        hipLaunchKernelGGL(sdf_fold_finish_k, dim3(cdiv(n, 256)), dim3(256), 0, st, w.fold, lg, n, g_tsdf);
        GS_LAUNCH_CHECK(nm.finish);
    }
    // the carried adjoints (the seam has none) + what the last pixel pass left: g_init and g_poses (B,16), or the seam's (B,12)
    if (g_D) {
        hipLaunchKernelGGL(gn_fold12_k, dim3(B), dim3(BWD_T), 0, st, seam ? (const float *)nullptr : (const float *)w.gD,
                           (const float *)w.partD, prev_nblocks, w.prow, g_D, seam ? 12 : 16);
        GS_LAUNCH_CHECK(nm.last);
    }
    if (g_poses) {
        hipLaunchKernelGGL(gn_fold12_k, dim3(B), dim3(BWD_T), 0, st, seam ? (const float *)nullptr : (const float *)w.gP,
                           (const float *)w.partP, prev_nblocks, w.prow, g_poses, seam ? 12 : 16);
        GS_LAUNCH_CHECK(nm.last);
    }
    return 0;
}

extern "C" {

size_t gs_sdf_odometry_tape_bytes_for(int B, int H, int W, int stride, int levels, int numiters_total) {
    if (sdf_shape_fault(B, H, W, stride, levels) != 0 || !gn_total_ok(levels, numiters_total)) return 0;
    return sdf_tape_layout(B, H, W, stride, numiters_total, nullptr, nullptr);
}

size_t gs_sdf_odometry_bwd_room(int B, int H, int W, int stride, int levels, int numiters_total, int nx, int ny, int nz, int want_tsdf) {
    if (sdf_shape_fault(B, H, W, stride, levels) != 0 || !gn_total_ok(levels, numiters_total) || !sdf_dims_ok(nx, ny, nz)) return 0;
    return sdf_room_layout(B, H, W, stride, numiters_total, (int64_t)nx * ny * nz, want_tsdf != 0, nullptr, nullptr);
}

int gs_sdf_odometry(const float *depth, int B, int H, int W, const float *intrinsics, const float *poses, const float *init,
                    const float *tsdf, const float *weight, int nx, int ny, int nz, const float *origin, float voxel_size, float trunc,
                    float min_weight, int stride, int levels, const int *numiters, float damp, float *out_T, float *info, void *ws,
                    size_t ws_bytes, gs_stream_t stream) {
    GS_REQUIRE(depth && intrinsics && poses && tsdf && weight && origin && numiters && out_T && info, "gs_sdf_odometry: null pointer");
    SDF_REQUIRE_SHAPE("gs_sdf_odometry");
    SDF_REQUIRE_VOLUME("gs_sdf_odometry");
    GN_REQUIRE_LOOP("gs_sdf_odometry");
    const size_t need = gs_sdf_odometry_ws_size(B, H, W, stride);
    GS_REQUIRE_WS("gs_sdf_odometry", ws, ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    SdfWs w;
    sdf_layout(B, H, W, stride, ws, &w);
    const SdfVolume vo{tsdf, weight, origin, nx, ny, nz, voxel_size, trunc, trunc / voxel_size, min_weight};
    return sdf_run(depth, B, H, W, intrinsics, poses, init, vo, stride, levels, numiters, damp, out_T, info, w, nullptr, st);
}

int gs_sdf_odometry_taped(const float *depth, int B, int H, int W, const float *intrinsics, const float *poses, const float *init,
                          const float *tsdf, const float *weight, int nx, int ny, int nz, const float *origin, float voxel_size,
                          float trunc, float min_weight, int stride, int levels, const int *numiters, float damp, float *out_T,
                          float *info, void *tape, size_t tape_cap, gs_stream_t stream) {
    GS_REQUIRE(depth && intrinsics && poses && tsdf && weight && origin && numiters && out_T && info, "gs_sdf_odometry_taped: null pointer");
    SDF_REQUIRE_SHAPE("gs_sdf_odometry_taped");
    SDF_REQUIRE_VOLUME("gs_sdf_odometry_taped");
    GN_REQUIRE_LOOP("gs_sdf_odometry_taped");
    const int total = gn_schedule(levels, numiters).total;
    const size_t need = sdf_tape_layout(B, H, W, stride, total, nullptr, nullptr);
    GS_REQUIRE_TAPE("gs_sdf_odometry_taped", tape, tape_cap, need, GS_ERR_WORKSPACE_TOO_SMALL);
    SdfTape t;
    sdf_tape_layout(B, H, W, stride, total, tape, &t);
    const SdfVolume vo{tsdf, weight, origin, nx, ny, nz, voxel_size, trunc, trunc / voxel_size, min_weight};
    return sdf_run(depth, B, H, W, intrinsics, poses, init, vo, stride, levels, numiters, damp, out_T, info, t.f, t.rows, (hipStream_t)stream);
}

int gs_sdf_odometry_bwd(const float *depth, int B, int H, int W, const float *intrinsics, const float *poses, const float *tsdf,
                        const float *weight, int nx, int ny, int nz, const float *origin, float voxel_size, float trunc,
                        float min_weight, int stride, int levels, const int *numiters, float damp, const void *tape, size_t tape_cap,
                        const float *grad_T, float *g_depth, float *g_poses, float *g_init, float *g_tsdf, void *room, size_t room_cap,
                        gs_stream_t stream) {
    GS_REQUIRE(depth && intrinsics && poses && tsdf && weight && origin && numiters && grad_T, "gs_sdf_odometry_bwd: null pointer");
    SDF_REQUIRE_SHAPE("gs_sdf_odometry_bwd");
    SDF_REQUIRE_VOLUME("gs_sdf_odometry_bwd");
    GN_REQUIRE_LOOP("gs_sdf_odometry_bwd");
    const int total = gn_schedule(levels, numiters).total;
    const size_t need = sdf_tape_layout(B, H, W, stride, total, nullptr, nullptr);
    GS_REQUIRE_TAPE("gs_sdf_odometry_bwd", tape, tape_cap, need, GS_ERR_WORKSPACE_TOO_SMALL);
    SdfTape t;
    sdf_tape_layout(B, H, W, stride, total, const_cast<void *>(tape), &t);
    const SdfVolume vo{tsdf, weight, origin, nx, ny, nz, voxel_size, trunc, trunc / voxel_size, min_weight};
    return sdf_bwd_run(SDF_BWD_NAMES("gs_sdf_odometry_bwd", "/begin"), depth, B, H, W, intrinsics, poses, vo, stride, levels, numiters, damp,
                       t.rows, grad_T, nullptr, nullptr, g_depth, g_poses, g_init, g_tsdf, room, room_cap, (hipStream_t)stream);
}

int gs_sdf_rows_bwd(const float *depth, int B, int H, int W, const float *intrinsics, const float *poses, const float *D,
                    const float *tsdf, const float *weight, int nx, int ny, int nz, const float *origin, float voxel_size, float trunc,
                    float min_weight, int stride, const float *g_sums, float *g_depth, float *g_poses, float *g_D, float *g_tsdf,
                    void *room, size_t room_cap, gs_stream_t stream) {
    GS_REQUIRE(depth && intrinsics && poses && D && tsdf && weight && origin && g_sums, "gs_sdf_rows_bwd: null pointer");
    const int levels = 1;
    SDF_REQUIRE_SHAPE("gs_sdf_rows_bwd");
    SDF_REQUIRE_VOLUME("gs_sdf_rows_bwd");
    const int one = 1;  // one level, one iteration
    const SdfVolume vo{tsdf, weight, origin, nx, ny, nz, voxel_size, trunc, trunc / voxel_size, min_weight};
    return sdf_bwd_run(SDF_BWD_NAMES("gs_sdf_rows_bwd", "/adjoints"), depth, B, H, W, intrinsics, poses, vo, stride, levels, &one, 0.0f,
                       nullptr, nullptr, D, g_sums, g_depth, g_poses, g_D, g_tsdf, room, room_cap, (hipStream_t)stream);
}

}  // extern "C"
