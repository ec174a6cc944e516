// rgbd.hip -- dense RGB-D odometry: joint photometric + depth alignment of two frames over an image pyramid, coarse to fine
// (gs_rgbd_odometry, gs_rgbd_rows, gs_rgbd_pyramid).  The rule -- every fp32 operation in order -- is stated in
// include/gradslam_hip.h above the entry points; this file follows it line by line (the library is built without contraction).
//
// P  pyramid: level 0 is (intensity, depth or 0) per pixel as ONE float2, so that a bilinear corner is one 8-byte load; every
//    further level is a 2 x 2 reduction of the level before.  One launch per frame and level.
// L  linearise: one source pixel per lane: warp, four corner loads, the two Jacobian rows and residuals, the lane's 29 terms;
//    a transposing wave butterfly, then the waves in order, leave one partial row per block (gs_icp_reduce.hpp's geometry).
// X  step: a launch of its own, one 1024-thread block per batch element: reduce_partials (fixed order), then one lane solves
//    (gs::solve6, fp64) and composes T <- exp(xi) T.  Two launches per iteration, no float atomics, nothing synchronises the
//    host; the loop state (T per batch element) lives in the workspace.
#include <math.h>
#include <stddef.h>
#include <algorithm>
#include <type_traits>

// gs_icp_step.hpp (solve6, se3_exp_dev; it brings gs_icp_reduce.hpp) also DEFINES icp.hip's stand-alone step kernel, a plain
// __global__ with external linkage: a second translation unit that includes the header as it is would define the symbol a
// second time.  This unit's copy gets a name of its own; nothing launches it.
#define icp_step_k icp_step_k_in_rgbd_unit
#include "gs_icp_step.hpp"
#undef icp_step_k

namespace gs {

constexpr int RGBD_T = LIN_T;        // lanes (= source pixels) per linearise block: block_reduce_store's geometry
constexpr int RGBD_MAX_LEVELS = 8;
constexpr int RGBD_MIN_SIDE = 4;     // the coarsest level is at least 4 x 4
constexpr int RGBD_STATUS_FEW = 1;   // fewer than 6 valid pixels
constexpr int RGBD_STATUS_SOLVE = 2; // the solve (or the composed transform) was not finite

struct RgbdCam {
    float fx, fy, cx, cy;
};
// intrinsics (4 x 4 row-major) at pyramid level `level`: fx, fy halve; cx' = (cx + 0.5) / 2 - 0.5 (pixel centres at integers)
__device__ __forceinline__ RgbdCam rgbd_cam(const float *__restrict__ K, int level) {
    RgbdCam c{K[0], K[5], K[2], K[6]};
    for (int l = 0; l < level; ++l) {
        c.fx = c.fx * 0.5f;
        c.fy = c.fy * 0.5f;
        c.cx = (c.cx + 0.5f) * 0.5f - 0.5f;
        c.cy = (c.cy + 0.5f) * 0.5f - 0.5f;
    }
    return c;
}

// ------------------------------------------------------------------ P: pyramid
__global__ __launch_bounds__(256) void rgbd_level0_k(const float *__restrict__ depth, const float *__restrict__ rgb, int64_t n,
                                                    float rgb_scale, float2 *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
    const float I = rgb_scale * ((0.299f * r + 0.587f * g) + 0.114f * b);
    const float d = depth[i];
    out[i] = make_float2(I, (d > 0.0f && d < INFINITY) ? d : 0.0f);
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
    float dmin = INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k) dmin = (c[k].y > 0.0f && c[k].y < dmin) ? c[k].y : dmin;
    float s = 0.0f;
    int n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (c[k].y > 0.0f && c[k].y - dmin <= ddm) { s = s + c[k].y; ++n; }
    out[(int64_t)blockIdx.y * Hl * Wl + p] = make_float2(I, n > 0 ? s / (float)n : 0.0f);
}

// ------------------------------------------------------------------ L: linearise
// The block's 29 sums -> partials[blockIdx.x], in block_reduce_store's geometry and order of magnitude (six pairwise steps in
// the wave, then the waves in order), but as a TRANSPOSING butterfly: at step s a lane keeps one half of its values and hands
// the other half to its partner (the lane 2^s away), so the 32 (29 + 3 zeros) values per lane halve at every step -- 31
// exchanges per lane instead of 29 x 6 -- and steps 0 .. 3 are DPP moves in the vector pipeline (quad permutes, rotations of
// the 16-lane row), not LDS permutes: at one source pixel per lane the permutes of 29 plain butterflies were the kernel's whole
// time (16 us at 480 x 640).  Partners: lane ^ 1, lane ^ 2, the lane 4 further round its row (same low bits, bit 2 flipped),
// lane ^ 8, lane ^ 16, lane ^ 32.  Value k ends in the lanes whose low five bits are k's bits reversed.  Every addition is
// keep + received, in a fixed order: the same bits from run to run.
template <int CTRL>
__device__ __forceinline__ float rgbd_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int N, int CTRL>
__device__ __forceinline__ void rgbd_fold_dpp(float (&a)[32], bool up) {  // N values -> N / 2; `up` lanes keep the upper half
#pragma unroll
    for (int j = 0; j < N / 2; ++j) {
        const float send = up ? a[j] : a[j + N / 2], keep = up ? a[j + N / 2] : a[j];
        a[j] = keep + rgbd_dpp<CTRL>(send);
    }
}
__device__ __forceinline__ void rgbd_block_reduce_store(float (&a)[32], float *__restrict__ partials) {
    __shared__ float sm[RGBD_T / 64][32];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    rgbd_fold_dpp<32, 0xB1>(a, lane & 1);    // quad_perm [1, 0, 3, 2]
    rgbd_fold_dpp<16, 0x4E>(a, lane & 2);    // quad_perm [2, 3, 0, 1]
    rgbd_fold_dpp<8, 0x124>(a, lane & 4);    // row_ror 4
    rgbd_fold_dpp<4, 0x128>(a, lane & 8);    // row_ror 8
    {
        const bool up = lane & 16;
        const float send = up ? a[0] : a[1], keep = up ? a[1] : a[0];
        a[0] = keep + __shfl_xor(send, 16, kWave);
    }
    a[0] = a[0] + __shfl_xor(a[0], 32, kWave);
    const int k = ((lane & 1) << 4) | ((lane & 2) << 2) | (lane & 4) | ((lane & 8) >> 2) | ((lane & 16) >> 4);
    if (lane < 32) sm[wid][k] = a[0];
    __syncthreads();
    if (threadIdx.x < NACC) {
        float v = 0.0f;
#pragma unroll
        for (int w = 0; w < RGBD_T / 64; ++w) v += sm[w][threadIdx.x];
        partials[blockIdx.x * NACC + threadIdx.x] = v;
    }
}

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
    bool ok = p < npix;
    float2 s = make_float2(0.0f, 0.0f);
    int v = 0, u = 0;
    if (ok) {
        v = p / Wl;
        u = p - v * Wl;
        s = src[(int64_t)b * npix + p];
        ok = s.y > 0.0f;
    }
    if (ok) {
        const float d = s.y;
        const float px = d * (((float)u - cam.cx) / cam.fx), py = d * (((float)v - cam.cy) / cam.fy);
        const float qx = ((T[0] * px + T[1] * py) + T[2] * d) + T[3];
        const float qy = ((T[4] * px + T[5] * py) + T[6] * d) + T[7];
        const float qz = ((T[8] * px + T[9] * py) + T[10] * d) + T[11];
        ok = qz > 0.0f;
        const float iz = 1.0f / qz;
        const float x = (cam.fx * qx) * iz + cam.cx, y = (cam.fy * qy) * iz + cam.cy;
        const float xf = floorf(x), yf = floorf(y);
        // 0 <= i <= W - 2 and 0 <= j <= H - 2 (a NaN fails every comparison)
        ok = ok && xf >= 0.0f && xf <= (float)(Wl - 2) && yf >= 0.0f && yf <= (float)(Hl - 2);
        if (ok) {
            const int i = (int)xf, j = (int)yf;
            const float a = x - xf, bb = y - yf;
            const float2 *c = timg + (int64_t)j * Wl + i;
            const float2 c00 = c[0], c10 = c[1], c01 = c[Wl], c11 = c[Wl + 1];  // c_xy: x offset first
            ok = c00.y > 0.0f && c10.y > 0.0f && c01.y > 0.0f && c11.y > 0.0f;
            // bilinear interpolants and their exact derivatives
            const float iX0 = c10.x - c00.x, iX1 = c11.x - c01.x, dX0 = c10.y - c00.y, dX1 = c11.y - c01.y;
            const float iTop = c00.x + a * iX0, iBot = c01.x + a * iX1, dTop = c00.y + a * dX0, dBot = c01.y + a * dX1;
            const float Ih = iTop + bb * (iBot - iTop), Dh = dTop + bb * (dBot - dTop);
            const float Ix = iX0 + bb * (iX1 - iX0), Iy = iBot - iTop, Dx = dX0 + bb * (dX1 - dX0), Dy = dBot - dTop;
            const float ri = Ih - s.x, rd = Dh - qz;
            ok = ok && fabsf(rd) <= ddm;
            if (ok) {
                const float gx = cam.fx * iz, gy = cam.fy * iz;
                // d(value) / dq as a row (c0, c1, c2); d q / d xi = [I | -q^]  ->  J = w (c | q x c)
                const float i0 = Ix * gx, i1 = Iy * gy, i2 = -((i0 * qx + i1 * qy) * iz);
                const float d0 = Dx * gx, d1 = Dy * gy, d2 = -((d0 * qx + d1 * qy) * iz) - 1.0f;
                JI[0] = wI * i0; JI[1] = wI * i1; JI[2] = wI * i2;
                JI[3] = wI * (qy * i2 - qz * i1); JI[4] = wI * (qz * i0 - qx * i2); JI[5] = wI * (qx * i1 - qy * i0);
                JD[0] = wD * d0; JD[1] = wD * d1; JD[2] = wD * d2;
                JD[3] = wD * (qy * d2 - qz * d1); JD[4] = wD * (qz * d0 - qx * d2); JD[5] = wD * (qx * d1 - qy * d0);
                rI = wI * ri;
                rD = wD * rd;
            }
        }
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
    rgbd_block_reduce_store(acc, partials + (int64_t)b * prow * NACC);
}

// ------------------------------------------------------------------ X: step
// grid B, 1024 threads.  Reduces batch element b's `nblocks` partial rows; `sums` (B, 29: H upper | g = -sum | err | cnt)
// is written when given; with `apply`, lane 0 solves and composes T[b] <- exp(xi) T[b], and writes out_T[b] and the level's
// info row (cnt, err, status bits of the level so far, iterations run at the level).
__global__ __launch_bounds__(1024) void rgbd_step_k(float *__restrict__ Tall, const float *__restrict__ partials, int nblocks, int prow,
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
    float *T = Tall + 16 * b;
    float *row = info + ((int64_t)b * levels + level) * 4;
    int status = it == 0 ? 0 : (int)row[2];
    const float cnt = acc[28];
    if (cnt < 6.0f) {
        status |= RGBD_STATUS_FEW;
    } else {
        float hg[44], xi[6], dT[16], Tn[16];
        expand44(acc, hg);
        for (int k = 0; k < 6; ++k) hg[36 + k] = -hg[36 + k];
        solve6(hg, hg + 36, damp, xi, lu_sm);
        bool fin = true;
        for (int k = 0; k < 6; ++k) fin = fin && fabsf(xi[k]) < INFINITY;
        if (fin) {
            se3_exp_dev(xi, dT);
            compose44(dT, T, Tn);
            for (int k = 0; k < 12; ++k) fin = fin && fabsf(Tn[k]) < INFINITY;
        }
        if (fin) {
            for (int k = 0; k < 16; ++k) T[k] = Tn[k];
        } else {
            status |= RGBD_STATUS_SOLVE;
        }
    }
    row[0] = cnt;
    row[1] = acc[27];
    row[2] = (float)status;
    row[3] = (float)(it + 1);
    for (int k = 0; k < 16; ++k) out_T[16 * b + k] = T[k];
}

// T[b] = out_T[b] = init[b] or the identity; info = 0.  One thread per word.
__global__ __launch_bounds__(256) void rgbd_init_k(const float *__restrict__ init, int B, int n_info, float *__restrict__ Tall,
                                                  float *__restrict__ out_T, float *__restrict__ info) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 16 * B) {
        const float v = init ? init[i] : (((i & 15) % 5 == 0) ? 1.0f : 0.0f);
        Tall[i] = v;
        out_T[i] = v;
    }
    if (i < n_info) info[i] = 0.0f;
}

// ------------------------------------------------------------------ host
struct RgbdWs {
    float *T;         // B x 16
    float *partials;  // B x prow x NACC
    float2 *tgt, *src;  // level-major pyramids: level l at + B * off[l] pixels
    int prow;
    int Hl[RGBD_MAX_LEVELS], Wl[RGBD_MAX_LEVELS];
    int64_t off[RGBD_MAX_LEVELS + 1];  // pixels per batch element in the levels before l
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
static bool rgbd_shape_ok(int B, int H, int W, int levels) {
    return B >= 1 && B <= 65535 && levels >= 1 && levels <= RGBD_MAX_LEVELS && H >= 1 && W >= 1 && (int64_t)H * W <= (1 << 24) &&
           (int64_t)B * H * W <= (1 << 30) && (H >> (levels - 1)) >= RGBD_MIN_SIDE && (W >> (levels - 1)) >= RGBD_MIN_SIDE;
}
#define RGBD_REQUIRE_SHAPE(name)                                                                                                  \
    do {                                                                                                                          \
        GS_REQUIRE(B >= 1 && B <= 65535, name ": B must be in [1, 65535], got %d", B);                                            \
        GS_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= (1 << 24), name ": H x W must be positive and at most 2^24 pixels, got %d x %d", H, W); \
        GS_REQUIRE((int64_t)B * H * W <= (1 << 30), name ": B H W must be at most 2^30, got %d x %d x %d", B, H, W);              \
        GS_REQUIRE(levels >= 1 && levels <= RGBD_MAX_LEVELS, name ": levels must be in [1, %d], got %d", RGBD_MAX_LEVELS, levels); \
        GS_REQUIRE((H >> (levels - 1)) >= RGBD_MIN_SIDE && (W >> (levels - 1)) >= RGBD_MIN_SIDE,                                  \
                   name ": the coarsest of %d levels of a %d x %d image would be smaller than 4 x 4", levels, H, W);               \
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
    hipLaunchKernelGGL(rgbd_step_k, dim3(B), dim3(1024), 0, st, w.T, w.partials, w.prow, w.prow, 0.0f, 0, 1, 0, 0, (float *)nullptr,
                       (float *)nullptr, sums);
    GS_LAUNCH_CHECK("gs_rgbd_rows/sums");
    return 0;
}

int gs_rgbd_odometry(const float *tgt_depth, const float *tgt_rgb, const float *src_depth, const float *src_rgb, int B, int H, int W,
                     const float *intrinsics, const float *init, int levels, const int *numiters, float lambda_geo,
                     float depth_diff_max, float damp, float rgb_scale, float *out_T, float *info, void *ws, size_t ws_bytes,
                     gs_stream_t stream) {
    GS_REQUIRE(tgt_depth && tgt_rgb && src_depth && src_rgb && intrinsics && numiters && out_T && info, "gs_rgbd_odometry: null pointer");
    RGBD_REQUIRE_SHAPE("gs_rgbd_odometry");
    RGBD_REQUIRE_LAMBDA("gs_rgbd_odometry");
    RGBD_REQUIRE_PARAMS("gs_rgbd_odometry");
    GS_REQUIRE(damp >= 0.0f && damp < INFINITY, "gs_rgbd_odometry: damp must be finite and not negative, got %g", (double)damp);
    for (int l = 0; l < levels; ++l)
        GS_REQUIRE(numiters[l] >= 0 && numiters[l] <= (1 << 20), "gs_rgbd_odometry: numiters[%d] must be in [0, 2^20], got %d", l, numiters[l]);
    const size_t need = gs_rgbd_odometry_ws_bytes(B, H, W, levels);
    GS_REQUIRE_WS("gs_rgbd_odometry", ws, ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    RgbdWs w;
    rgbd_layout(B, H, W, levels, ws, &w);
    const int n_info = B * levels * 4;
    hipLaunchKernelGGL(rgbd_init_k, dim3(cdiv(std::max(16 * B, n_info), 256)), dim3(256), 0, st, init, B, n_info, w.T, out_T, info);
    GS_LAUNCH_CHECK("gs_rgbd_odometry/init");
    int rc = rgbd_build_pyramid("gs_rgbd_odometry/pyramid", tgt_depth, tgt_rgb, B, levels, w, depth_diff_max, rgb_scale, w.tgt, st);
    if (rc) return rc;
    rc = rgbd_build_pyramid("gs_rgbd_odometry/pyramid", src_depth, src_rgb, B, levels, w, depth_diff_max, rgb_scale, w.src, st);
    if (rc) return rc;
    const float wI = sqrtf(1.0f - lambda_geo), wD = sqrtf(lambda_geo);
    for (int l = levels - 1; l >= 0; --l) {
        const int nblocks = cdiv((int64_t)w.Hl[l] * w.Wl[l], RGBD_T);
        for (int it = 0; it < numiters[l]; ++it) {
            hipLaunchKernelGGL(rgbd_linearize_k<false>, dim3(nblocks, B), dim3(RGBD_T), 0, st, w.tgt + B * w.off[l], w.src + B * w.off[l],
                               w.Hl[l], w.Wl[l], l, intrinsics, w.T, wI, wD, depth_diff_max, w.partials, w.prow, (int32_t *)nullptr,
                               (float *)nullptr);
            GS_LAUNCH_CHECK("gs_rgbd_odometry/linearize");
            hipLaunchKernelGGL(rgbd_step_k, dim3(B), dim3(1024), 0, st, w.T, w.partials, nblocks, w.prow, damp, l, levels, it, 1, out_T,
                               info, (float *)nullptr);
            GS_LAUNCH_CHECK("gs_rgbd_odometry/step");
        }
    }
    return 0;
}

}  // extern "C"
