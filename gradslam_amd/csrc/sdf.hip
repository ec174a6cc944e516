// sdf.hip -- SDF odometry: a camera tracked directly against the TSDF volume (gs_sdf_odometry, gs_sdf_rows).  Gauss-Newton on
// sum phi(D P p)^2 over the frame's pixels, phi the volume's interpolated distance: no ray cast, no association, no cloud.  The
// rule -- every fp32 operation in order -- is stated in include/gradslam_hip.h above the entry points; the code follows it line
// by line (the library is built without contraction).
//   gs_sdf_pixel.hpp  the pixel, once: back-projection, the gates in their order, the row
//   this file         L, X: the kernels; every launch, the workspace and the C entry points
// L  linearise: one pixel of the level's grid per lane: depth, two transforms, the cell, 16 gathers in one batch, the row, the
//    lane's 29 terms; gs_rowsum.hpp's transposing butterfly leaves one partial row per block.
// X  step: one 1024-thread block per batch element: reduce_partials (fixed order), then one lane solves (gs::solve6, fp64) and
//    composes D <- exp(xi) D.  Two launches per iteration plus one to start, no float atomics, nothing synchronises the host; the
//    loop state (D per batch element) lives in the workspace.
#include <math.h>
#include <stddef.h>
#include <algorithm>

#include "gs_gn_step.hpp"  // constants, the start-up, the shared host checks; it brings gs_icp_step.hpp (solve6, se3_exp_dev, reduce_partials)
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

// ------------------------------------------------------------------ X: step
// grid B, 1024 threads.  Reduces batch element b's `nblocks` partial rows; `sums` (B, 29: H upper | g = -sum | err | cnt) is
// written when given; with `apply`, lane 0 solves and composes D[b] <- exp(xi) D[b], and writes out_T[b] and the level's info
// row (cnt, err, status bits of the level so far, iterations run at the level).
__global__ __launch_bounds__(1024) void sdf_step_k(float *__restrict__ Dall, const float *__restrict__ partials, int nblocks, int prow,
                                                  float damp, int level, int levels, int it, int apply, float *__restrict__ out_T,
                                                  float *__restrict__ info, float *__restrict__ sums) {
    __shared__ float acc[NACC];
    __shared__ double lu_sm[42];
    const int b = blockIdx.x;
    reduce_partials(partials + (int64_t)b * prow * NACC, nblocks, acc);
    if (threadIdx.x != 0) return;
    if (sums) {
        for (int k = 0; k < NACC; ++k) sums[NACC * b + k] = (k >= 21 && k < 27) ? -acc[k] : acc[k];
    }
    if (!apply) return;
    float *D = Dall + 16 * b;
    float *row = info + ((int64_t)b * levels + level) * 4;
    int status = it == 0 ? 0 : (int)row[2];
    const float cnt = acc[28];
    if (cnt < 6.0f) {
        status |= GN_STATUS_FEW;
    } else {
        float hg[44], xi[6], dT[16], Dn[16];
        expand44(acc, hg);
        for (int k = 0; k < 6; ++k) hg[36 + k] = -hg[36 + k];
        solve6(hg, hg + 36, damp, xi, lu_sm);
        bool fin = true;
        for (int k = 0; k < 6; ++k) fin = fin && fabsf(xi[k]) < INFINITY;
        if (fin) {
            se3_exp_dev(xi, dT);
            compose44(dT, D, Dn);
            for (int k = 0; k < 12; ++k) fin = fin && fabsf(Dn[k]) < INFINITY;
        }
        if (fin) {
            for (int k = 0; k < 16; ++k) D[k] = Dn[k];
        } else {
            status |= GN_STATUS_SOLVE;
        }
    }
    row[0] = cnt;
    row[1] = acc[27];
    row[2] = (float)status;
    row[3] = (float)(it + 1);
    for (int k = 0; k < 16; ++k) out_T[16 * b + k] = D[k];
}

__global__ __launch_bounds__(256) void sdf_init_k(const float *__restrict__ init, int B, int n_info, float *__restrict__ Dall,
                                                 float *__restrict__ out_T, float *__restrict__ info) {
    gn_init(init, B, n_info, Dall, out_T, info);
}

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
static size_t sdf_layout(int B, int H, int W, int stride, void *ws, SdfWs *w) {
    Carve c{(char *)ws};
    SdfWs t;
    const SdfGrid g = sdf_grid(H, W, stride, 0);
    t.prow = cdiv((int64_t)g.Hs * g.Ws, SDF_T);
    t.D = c.take<float>(sizeof(float) * 16 * B);
    t.partials = c.take<float>(sizeof(float) * NACC * (size_t)t.prow * B);
    if (w) *w = t;
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
    hipLaunchKernelGGL(sdf_step_k, dim3(B), dim3(1024), 0, st, w.D, w.partials, w.prow, w.prow, 0.0f, 0, 1, 0, 0, (float *)nullptr,
                       (float *)nullptr, sums);
    GS_LAUNCH_CHECK("gs_sdf_rows/sums");
    return 0;
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
    const int n_info = B * levels * 4;
    hipLaunchKernelGGL(sdf_init_k, dim3(cdiv(std::max(16 * B, n_info), 256)), dim3(256), 0, st, init, B, n_info, w.D, out_T, info);
    GS_LAUNCH_CHECK("gs_sdf_odometry/init");
    for (int l = levels - 1; l >= 0; --l) {
        const SdfGrid g = sdf_grid(H, W, stride, l);
        const int nblocks = cdiv((int64_t)g.Hs * g.Ws, SDF_T);
        for (int it = 0; it < numiters[l]; ++it) {
            sdf_launch_linearize(false, depth, B, g, intrinsics, poses, w.D, vo, w, nullptr, nullptr, st);
            GS_LAUNCH_CHECK("gs_sdf_odometry/linearize");
            hipLaunchKernelGGL(sdf_step_k, dim3(B), dim3(1024), 0, st, w.D, w.partials, nblocks, w.prow, damp, l, levels, it, 1, out_T, info,
                               (float *)nullptr);
            GS_LAUNCH_CHECK("gs_sdf_odometry/step");
        }
    }
    return 0;
}

}  // extern "C"
