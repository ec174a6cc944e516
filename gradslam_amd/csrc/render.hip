// render.hip -- the map seen from a camera (R): z-buffered index, depth, position, normal and colour images, and the
// reverse pass.  Everything else in the library runs from frames to the map; this is the way back.
//
// Semantics, for batch element b, camera (poses[b], intrinsics[b]) and an H x W image:
//  * CANDIDATES: map row n is a candidate iff n < min(counts[b], Nmax) and project_point_z (gs_project.hpp: the in-frame
//    test of find_active_map_points -- z > 0, u > -1e-3, u < W - 0.999, the same for v, rounding half-to-even) accepts it.
//    Its pixel is the (h, w) that function returns; its depth is the z it returns, the camera-frame
//    dot3_fma(p, R[:,2]) + tinv[2] in fp32, before K.
//  * WINNER of a pixel: the candidate with the smallest z as fp32; equal z: the smallest n.  One 64-bit atomicMin on
//    (float_bits(z) << 32) | n does both -- z > 0, so bit order is float order -- and does not depend on arrival order.
//  * OUTPUTS, all fully written (the caller passes uninitialised memory): index (B,H,W) int32 = the winner's n or -1; depth
//    (B,H,W) = its z or 0; points / normals / colors (B,H,W,3) = its map attributes (gathered, not recomputed) or zeros.
//    An attribute image is skipped when its output pointer or its map array is NULL.
// One point is one pixel: no splats, no supersampling, no hole filling.
//
// Three launches, no allocation, no host synchronisation, no memset: keys filled with all-ones; ONE phased pass over the
// map (12 B read per map point + one atomic per candidate); one thread per pixel resolves its key and gathers.
//
// REVERSE PASS.  The pixel assignment and the winner are constants of the graph (like association indices in the ICP and
// fusion reverse passes); what is differentiated is what is differentiable almost everywhere.  With z = sum_j R[j][2] (p_j - t_j):
//    g_points[n]            = g_out_points[pix] + g_depth[pix] * R[:,2]
//    g_normals[n], g_colors[n] = their pixel's adjoint
//    g_poses[b][j][2]       = sum_pix g_depth * (p_j - t_j)          (rotation column 2)
//    g_poses[b][j][3]       = -R[j][2] * sum_pix g_depth             (translation)
// The intrinsics adjoint is zero almost everywhere and not produced.  A map row wins at most one pixel, so the scatter
// is plain stores: no atomics anywhere, and the four pose sums per b go through per-block rows and one fixed-order fold
// (gs_rowsum.hpp) -- the same bits from run to run.
#include "gs_common.hpp"
#include "gs_project.hpp"
#include "gs_rowsum.hpp"

namespace gs {

constexpr int REND_T = 256, REND_I = 4, REND_B = REND_T * REND_I;
constexpr unsigned long long kNoKey = ~0ull;  // no candidate: never a key, float_bits(z) of a z > 0 is below 0x7f800001

__global__ __launch_bounds__(REND_T) void render_fill_k(unsigned long long *__restrict__ pix_key, int64_t npix) {
    for (int64_t i = (int64_t)blockIdx.x * REND_T + threadIdx.x; i < npix; i += (int64_t)gridDim.x * REND_T) pix_key[i] = kNoKey;
}

// The map-wide pass, in corr_pass1_k's form (fusion.hip): the camera through LDS in one round of loads, REND_I items per
// thread, the points of all items requested before any is projected, clamped indices instead of branches around loads.
__global__ __launch_bounds__(REND_T) void render_pass_k(const float *__restrict__ mp, const int32_t *__restrict__ counts, int Nmax,
                                                        const float *__restrict__ poses, const float *__restrict__ Ks, int H, int W,
                                                        float umax, float vmax, unsigned long long *__restrict__ pix_key) {
    __shared__ Cam cam;
    const int b = blockIdx.y;
    block_cam(cam, poses, Ks, b);
    const int cnt = min(counts[b], Nmax);
    const int64_t HW = (int64_t)H * W;
    const int64_t base = (int64_t)b * Nmax;
    const int n0 = blockIdx.x * REND_B + threadIdx.x;
    // phase 1: the points
    f3 p[REND_I];
    bool live[REND_I];
#pragma unroll
    for (int k = 0; k < REND_I; ++k) {
        const int n = n0 + k * REND_T;
        live[k] = n < cnt;
        p[k] = ld3(mp, base + (live[k] ? n : 0));
    }
    __syncthreads();
    // phase 2: projection and the z-buffer atomics
#pragma unroll
    for (int k = 0; k < REND_I; ++k) {
        int h, w;
        float z;
        const bool act = project_point_z(cam, p[k], H, W, umax, vmax, h, w, z) && live[k];
        if (act)
            atomicMin(pix_key + b * HW + (h * W + w), ((unsigned long long)fbits(z) << 32) | (unsigned int)(n0 + k * REND_T));
    }
}

// one thread per pixel: key -> (n, z), then the winner's attributes
__global__ __launch_bounds__(REND_T) void render_resolve_k(const unsigned long long *__restrict__ pix_key, int64_t npix, int64_t HW,
                                                           int Nmax, const float *__restrict__ mp, const float *__restrict__ mn,
                                                           const float *__restrict__ mc, int32_t *__restrict__ out_index,
                                                           float *__restrict__ out_depth, float *__restrict__ op,
                                                           float *__restrict__ on, float *__restrict__ oc) {
    const int64_t i = (int64_t)blockIdx.x * REND_T + threadIdx.x;
    if (i >= npix) return;
    const unsigned long long key = pix_key[i];
    const bool hit = key != kNoKey;
    const int n = hit ? (int)(unsigned int)key : 0;
    const int64_t pt = (i / HW) * (int64_t)Nmax + n;
    const f3 zero{0.0f, 0.0f, 0.0f};
    f3 x = zero, y = zero, c = zero;
    if (op) x = ld3(mp, pt);
    if (on) y = ld3(mn, pt);
    if (oc) c = ld3(mc, pt);
    out_index[i] = hit ? n : -1;
    out_depth[i] = hit ? bitsf((uint32_t)(key >> 32)) : 0.0f;
    if (op) st3(op, i, hit ? x : zero);
    if (on) st3(on, i, hit ? y : zero);
    if (oc) st3(oc, i, hit ? c : zero);
}

// ------------------------------------------------------------------ reverse pass
// rows that won no pixel (and rows beyond the count) receive zero: every row is zeroed, the winners are overwritten
__global__ __launch_bounds__(REND_T) void render_bwd_zero_k(int64_t nfloats, float *__restrict__ gp, float *__restrict__ gn,
                                                            float *__restrict__ gc) {
    for (int64_t i = (int64_t)blockIdx.x * REND_T + threadIdx.x; i < nfloats; i += (int64_t)gridDim.x * REND_T) {
        if (gp) gp[i] = 0.0f;
        if (gn) gn[i] = 0.0f;
        if (gc) gc[i] = 0.0f;
    }
}

constexpr int REND_PART = 4;  // per-block partial sums: g_depth * (p_j - t_j), j = 0..2, and g_depth
// one thread per pixel: the pixel's adjoints go to the row that won it; per-block partials of the pose sums
__global__ __launch_bounds__(REND_T) void render_bwd_pix_k(const int32_t *__restrict__ index, const int32_t *__restrict__ counts,
                                                           int Nmax, int HW, const float *__restrict__ mp,
                                                           const float *__restrict__ poses, const float *__restrict__ g_depth,
                                                           const float *__restrict__ gop, const float *__restrict__ gon,
                                                           const float *__restrict__ goc, float *__restrict__ gp,
                                                           float *__restrict__ gn, float *__restrict__ gc, float *__restrict__ part) {
    const int b = blockIdx.y;
    const int q = blockIdx.x * REND_T + threadIdx.x;
    const bool in = q < HW;
    const int64_t pix = (int64_t)b * HW + (in ? q : 0);
    const float *T = poses + 16 * b;
    const int cnt = min(counts[b], Nmax);
    const int n = index[pix];
    const bool hit = in && n >= 0 && n < cnt;  // (an index image that is not this map's forward output cannot reach outside it)
    const int64_t pt = (int64_t)b * Nmax + (hit ? n : 0);
    const f3 zero{0.0f, 0.0f, 0.0f};
    // every load of the pixel and of its row requested before anything is consumed
    const float gd = g_depth ? g_depth[pix] : 0.0f;
    const f3 a = gop ? ld3(gop, pix) : zero;
    const f3 u = (gon && gn) ? ld3(gon, pix) : zero;
    const f3 v = (goc && gc) ? ld3(goc, pix) : zero;
    const f3 p = part ? ld3(mp, pt) : zero;
    const float r0 = T[2], r1 = T[6], r2 = T[10], t0 = T[3], t1 = T[7], t2 = T[11];
    if (hit) {
        if (gp) st3(gp, pt, f3{__fmaf_rn(gd, r0, a.x), __fmaf_rn(gd, r1, a.y), __fmaf_rn(gd, r2, a.z)});
        if (gn) st3(gn, pt, u);
        if (gc) st3(gc, pt, v);
    }
    if (!part) return;  // (uniform: no pose adjoint wanted)
    const float m = hit ? gd : 0.0f;
    float acc[REND_PART] = {hit ? m * (p.x - t0) : 0.0f, hit ? m * (p.y - t1) : 0.0f, hit ? m * (p.z - t2) : 0.0f, m};
    block_row<REND_PART, REND_T / kWave>(acc, [&](unsigned n) { return &part[((int64_t)b * gridDim.x + blockIdx.x) * REND_PART + n]; });
}

// one block per b: the per-block partials added up in a fixed order, all 16 entries of g_poses[b] written
__global__ __launch_bounds__(REND_T) void render_bwd_final_k(const float *__restrict__ part, int nblocks,
                                                             const float *__restrict__ poses, float *__restrict__ g_poses) {
    __shared__ float tot[REND_PART];
    const int b = blockIdx.x;
    fold_rows<REND_PART, REND_T / REND_PART, REND_PART>(part + (int64_t)b * nblocks * REND_PART, nblocks, REND_PART, tot);
    if (threadIdx.x < 16) {
        const int i = threadIdx.x >> 2, j = threadIdx.x & 3;
        float out = 0.0f;
        if (i < 3 && j == 2) out = tot[i];
        if (i < 3 && j == 3) out = (-poses[16 * b + 4 * i + 2]) * tot[3];
        g_poses[16 * b + threadIdx.x] = out;
    }
}

// ---- workspaces: the forward's is the per-pixel keys, the reverse pass's the per-block partials of the pose sums
struct RenderWs {
    unsigned long long *pix_key;  // (B*H*W)
};
static size_t render_layout(int B, int H, int W, void *ws, RenderWs *out) {
    Carve c{(char *)ws};
    RenderWs scratch, &r = out ? *out : scratch;
    r.pix_key = c.take<unsigned long long>((size_t)B * H * W * 8);
    return c.off;
}
static inline int render_pix_blocks(int H, int W) { return cdiv((int64_t)H * W, REND_T); }
struct RenderBwdWs {
    float *part;  // (B, pixel blocks, REND_PART)
};
static size_t render_bwd_layout(int B, int H, int W, void *ws, RenderBwdWs *out) {
    Carve c{(char *)ws};
    RenderBwdWs scratch, &r = out ? *out : scratch;
    r.part = c.take<float>((size_t)B * render_pix_blocks(H, W) * REND_PART * 4);
    return c.off;
}
static inline bool render_shape_ok(int B, int Nmax, int H, int W) {
    return B > 0 && B <= 65535 && Nmax > 0 && H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31);
}
static inline int render_grid1d(int64_t n) { const int g = cdiv(n > 0 ? n : 1, REND_T); return g > 2048 ? 2048 : g; }

}  // namespace gs

using namespace gs;

extern "C" {

size_t gs_render_map_ws_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return render_layout(B, H, W, nullptr, nullptr);
}

int gs_render_map(const float *points, const float *normals, const float *colors, const int32_t *counts, int B, int Nmax,
                  const float *poses, const float *intrinsics, int H, int W, int32_t *out_index, float *out_depth, float *out_points,
                  float *out_normals, float *out_colors, void *ws, size_t ws_bytes, gs_stream_t stream) {
    GS_REQUIRE(points && counts && poses && intrinsics && out_index && out_depth, "gs_render_map: NULL argument");
    GS_REQUIRE(render_shape_ok(B, Nmax, H, W), "gs_render_map: bad shape B=%d Nmax=%d H=%d W=%d", B, Nmax, H, W);
    GS_REQUIRE_WS("gs_render_map", ws, ws_bytes, gs_render_map_ws_bytes(B, H, W));
    hipStream_t st = (hipStream_t)stream;
    RenderWs r;
    render_layout(B, H, W, ws, &r);
    const int64_t HW = (int64_t)H * W, npix = (int64_t)B * HW;
    const float umax = (float)((double)W - 0.999), vmax = (float)((double)H - 0.999);
    hipLaunchKernelGGL(render_fill_k, dim3(render_grid1d(npix)), dim3(REND_T), 0, st, r.pix_key, npix);
    GS_LAUNCH_CHECK("gs_render_map/fill");
    hipLaunchKernelGGL(render_pass_k, dim3(cdiv(Nmax, REND_B), B), dim3(REND_T), 0, st, points, counts, Nmax, poses, intrinsics, H, W, umax,
                       vmax, r.pix_key);
    GS_LAUNCH_CHECK("gs_render_map/pass");
    hipLaunchKernelGGL(render_resolve_k, dim3(cdiv(npix, REND_T)), dim3(REND_T), 0, st, (const unsigned long long *)r.pix_key, npix, HW, Nmax,
                       points, normals, colors, out_index, out_depth, out_points, normals ? out_normals : nullptr,
                       colors ? out_colors : nullptr);
    GS_LAUNCH_CHECK("gs_render_map/resolve");
    return GS_OK;
}

size_t gs_render_map_backward_ws_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return render_bwd_layout(B, H, W, nullptr, nullptr);
}

int gs_render_map_backward(const float *points, const int32_t *counts, int B, int Nmax, const float *poses, int H, int W,
                           const int32_t *index, const float *g_depth, const float *g_out_points, const float *g_out_normals,
                           const float *g_out_colors, float *g_points, float *g_normals, float *g_colors, float *g_poses, void *ws,
                           size_t ws_bytes, gs_stream_t stream) {
    GS_REQUIRE(points && counts && poses && index, "gs_render_map_backward: NULL argument");
    GS_REQUIRE(render_shape_ok(B, Nmax, H, W), "gs_render_map_backward: bad shape B=%d Nmax=%d H=%d W=%d", B, Nmax, H, W);
    GS_REQUIRE_WS("gs_render_map_backward", ws, ws_bytes, gs_render_map_backward_ws_bytes(B, H, W));
    hipStream_t st = (hipStream_t)stream;
    RenderBwdWs r;
    render_bwd_layout(B, H, W, ws, &r);
    const int nblk = render_pix_blocks(H, W);
    if (g_points || g_normals || g_colors) {
        const int64_t nfloats = (int64_t)B * Nmax * 3;
        hipLaunchKernelGGL(render_bwd_zero_k, dim3(render_grid1d(nfloats)), dim3(REND_T), 0, st, nfloats, g_points, g_normals, g_colors);
        GS_LAUNCH_CHECK("gs_render_map_backward/zero");
    }
    hipLaunchKernelGGL(render_bwd_pix_k, dim3(nblk, B), dim3(REND_T), 0, st, index, counts, Nmax, H * W, points, poses, g_depth, g_out_points,
                       g_out_normals, g_out_colors, g_points, g_normals, g_colors, g_poses ? r.part : nullptr);
    GS_LAUNCH_CHECK("gs_render_map_backward/pixels");
    if (g_poses) {
        hipLaunchKernelGGL(render_bwd_final_k, dim3(B), dim3(REND_T), 0, st, (const float *)r.part, nblk, poses, g_poses);
        GS_LAUNCH_CHECK("gs_render_map_backward/final");
    }
    return GS_OK;
}

}  // extern "C"
