// libgradslam_hip -- TSDF volumes (T): fuse posed RGB-D frames into a dense truncated signed-distance grid, take the surface out.
//
//   I  gs_tsdf_integrate: one launch per chunk of up to 32 frames.  One thread per 4 consecutive x-voxels: their tsdf, weight
//      and colour stay in registers while the chunk's frames are applied in order (gs_tsdf.hpp: centre, observe, average), the
//      chunk's cameras sit in LDS; the volume is read and written once per chunk.  Every voxel is read and written by one thread:
//      the outputs may alias the inputs.  No workspace, no atomics, nothing synchronises the host.
//      gs_tsdf_integrate_backward: chunks in reverse order, one thread per voxel.  The thread re-takes the forward's decisions
//      (a 32-bit update mask of the chunk, the number of updates before the chunk), then walks the chunk's frames backwards with
//      the weight rebuilt from the mask.  The depth / rgb adjoints of a pixel are sums over many voxels: the exact fixed-point
//      fold of gs_fixed128.hpp, per chunk   memset -> tsdf_bwd_k<MAX> -> tsdf_bwd_k<ACC> -> tsdf_fold_finish_k
//      (the two passes compute the same terms: storing them would take 16 B per voxel and frame).
//   E  gs_tsdf_extract: the stable compaction of gs_compact.hpp over the 3 nx ny nz edge slots:
//        tsdf_count_k -> tsdf_scan_k -> tsdf_write_k (skipped when cap == 0)
//      gs_tsdf_extract_backward: a memset and six (axis, end) passes over the rows; within a pass no two rows share a voxel, so
//      the adds are plain read-modify-writes in a fixed order.
//   R  gs_tsdf_raycast: the volume seen from a camera (the rule: gs_tsdf.hpp).  One launch, one thread per output pixel, a wave
//      per 8x8 tile; the ray is clipped against the box, then marched sample by sample: 8 weights, then 8 tsdf values.  No
//      workspace, no atomics, nothing synchronises the host.
//      gs_tsdf_raycast_backward: one thread per pixel recomputes its two samples and its hit from the tape k_end; a voxel's
//      adjoint is a sum over many pixels: the same fold, over the voxels
//        memset -> tsdf_raycast_bwd_k<MAX> -> tsdf_raycast_bwd_k<ACC> -> tsdf_cast_finish_k
//   P  gs_tsdf_integrate_backward_poses / gs_tsdf_raycast_backward_poses: the same passes from the same host drivers
//      (tsdf_integrate_backward_run, tsdf_raycast_backward_run); with g_poses the second one (POSE) also reduces a
//      camera's pose sums (4 per frame over the voxels; 12 over the pixels) wave by wave and block by block into one row per
//      block, which tsdf_pose_finish_k / tsdf_cast_pose_finish_k fold in a fixed order (gs_tsdf.hpp: the pose sums): plain fp32,
//      no atomics.  Outputs nobody asks for drop their passes (FOLD = false: no maximum pass, no fold, no finish).
// Batch elements ride in grid.y (R: frames in grid.y, batch elements in grid.z).
#include <cmath>
#include <stddef.h>

#include <algorithm>

#include "gs_compact.hpp"
#include "gs_fixed128.hpp"
#include "gs_tsdf.hpp"

namespace gs {

// ------------------------------------------------------------------ I: integration.  grid (x: quads of x-voxels, y: batch element)
template <bool VEC>
__device__ __forceinline__ void tsdf_ld4(const float *p, int nv, float *r) {
    if (VEC) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = k < nv ? p[k] : 0.0f;
    }
}
template <bool VEC>
__device__ __forceinline__ void tsdf_st4(float *p, int nv, const float *r) {
    if (VEC) {
        *reinterpret_cast<float4 *>(p) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < nv) p[k] = r[k];
    }
}

// VEC: nx is a multiple of 4 and every pointer is 16-byte aligned, so a thread's 4 voxels move as one 16-byte access
// (in / out are not __restrict__: they may alias)
template <bool VEC, bool COLOR>
__global__ __launch_bounds__(TSDF_T) void tsdf_integrate_k(TsdfVol vol, TsdfFrames fr, const float *tsdf_in, const float *weight_in,
                                                           const float *color_in, float *tsdf_out, float *weight_out, float *color_out) {
    __shared__ Cam cams[TSDF_CHUNK];
    const int b = blockIdx.y;
    tsdf_load_cams(cams, fr, b, fr.l0, fr.Lc);
    const int nx4 = (vol.nx + 3) >> 2;
    const int64_t nq = (int64_t)nx4 * vol.ny * vol.nz;
    const int64_t q = (int64_t)blockIdx.x * TSDF_T + threadIdx.x;
    if (q >= nq) return;
    const int row = (int)(q / nx4), x0 = (int)(q - (int64_t)row * nx4) * 4;
    const int iz = row / vol.ny, iy = row - iz * vol.ny;
    const int nv = min(4, vol.nx - x0);
    const int64_t at = (int64_t)b * tsdf_nvox(vol) + (int64_t)row * vol.nx + x0;
    const float *o = vol.origin + 3 * b;
    const float cy = tsdf_centre1(o[1], iy, vol.v), cz = tsdf_centre1(o[2], iz, vol.v);
    float cx[4], f[4], wt[4], col[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) cx[k] = tsdf_centre1(o[0], x0 + k, vol.v);
    tsdf_ld4<VEC>(tsdf_in + at, nv, f);
    tsdf_ld4<VEC>(weight_in + at, nv, wt);
    if (COLOR) {
#pragma unroll
        for (int k = 0; k < 3; ++k) tsdf_ld4<VEC>(color_in + 3 * at + 4 * k, 3 * nv - 4 * k, col + 4 * k);
    }
    const int64_t HW = (int64_t)fr.H * fr.W;
    for (int l = 0; l < fr.Lc; ++l) {
        const int64_t frame = ((int64_t)b * fr.L + fr.l0 + l) * HW;
        const float *dl = fr.depth + frame;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int pix;
            float sdf;
            if (k >= nv || !tsdf_observe(cams[l], f3{cx[k], cy, cz}, dl, fr, vol.trunc, pix, sdf)) continue;
            const float t = tsdf_sample(sdf, vol.trunc);
            f[k] = tsdf_average(wt[k], f[k], t);
            if (COLOR) {
                const f3 c = ld3(fr.rgb, frame + pix);
                col[3 * k] = tsdf_average(wt[k], col[3 * k], c.x);
                col[3 * k + 1] = tsdf_average(wt[k], col[3 * k + 1], c.y);
                col[3 * k + 2] = tsdf_average(wt[k], col[3 * k + 2], c.z);
            }
            wt[k] = tsdf_next_weight(wt[k], vol.maxw);
        }
    }
    tsdf_st4<VEC>(tsdf_out + at, nv, f);
    tsdf_st4<VEC>(weight_out + at, nv, wt);
    if (COLOR) {
#pragma unroll
        for (int k = 0; k < 3; ++k) tsdf_st4<VEC>(color_out + 3 * at + 4 * k, 3 * nv - 4 * k, col + 4 * k);
    }
}

// ------------------------------------------------------------------ reverse pass of the integration
// The fold of one chunk: per pixel (b, l, h, w) of the chunk 4 sums (depth, r, g, b).  With `poses` (the workspace of
// gs_tsdf_integrate_backward_poses; nvox and has_color count for it alone) behind it: one row of 4 pose sums per (b, frame of the
// chunk, block of 256 voxels) | with more than one chunk, the adjoints carried from chunk to chunk when the caller passes no
// g_tsdf_in / g_color_in to carry them in
struct TsdfBwdWs {
    Fold fold;
    size_t fold_bytes;
    float *psum, *carry_t, *carry_c;
};
static inline size_t tsdf_bwd_layout(int B, int L, int H, int W, bool poses, int64_t nvox, bool has_color, void *ws, TsdfBwdWs *out) {
    Carve c{(char *)ws};
    TsdfBwdWs scratch, &r = out ? *out : scratch;
    r.fold = fold_carve(c, (size_t)B * std::min(L, TSDF_CHUNK) * H * W, 4);
    r.fold_bytes = c.off;
    const bool carry = poses && L > TSDF_CHUNK;
    r.psum = poses ? c.take<float>(sizeof(float) * 4 * (size_t)B * std::min(L, TSDF_CHUNK) * cdiv(nvox, TSDF_T)) : nullptr;
    r.carry_t = carry ? c.take<float>(sizeof(float) * (size_t)B * nvox) : nullptr;
    r.carry_c = carry && has_color ? c.take<float>(sizeof(float) * 3 * (size_t)B * nvox) : nullptr;
    return c.off;
}

// grid (x: voxels, y: batch element).  ACC = false: the largest finite |term| of the chunk; ACC = true: the terms go into the
// fold and the adjoints carried to the frames before the chunk are written (g_*_src -> g_*_dst: the same thread reads and writes
// a voxel, so they may alias; a NULL g_*_dst is not written).  No thread leaves early: the camera loads are block-wide.
// POSE (the second pass of gs_tsdf_integrate_backward_poses): per frame of the chunk the block's sums of gd and gd (c - t) go to
// row ((b Lc + l) gridDim.x + blockIdx.x) of `psum` (gs_tsdf.hpp: the pose sums); FOLD = false: nothing goes into the fold.
template <bool ACC, bool POSE = false, bool FOLD = true>
__global__ __launch_bounds__(TSDF_T) void tsdf_bwd_k(TsdfVol vol, TsdfFrames fr, const float *__restrict__ weight_in, const float *g_tsdf_src,
                                                     const float *g_color_src, float *g_tsdf_dst, float *g_color_dst, Fold fold, int lg,
                                                     float *__restrict__ psum = nullptr) {
    __shared__ Cam cams[TSDF_CHUNK];
    __shared__ float red[POSE ? TSDF_CHUNK * TSDF_WAVES * 4 : 1];
    const int b = blockIdx.y;
    const int64_t nvox = tsdf_nvox(vol), j = (int64_t)blockIdx.x * TSDF_T + threadIdx.x;
    const bool live = j < nvox;
    const int64_t at = (int64_t)b * nvox + (live ? j : 0);
    int ix, iy, iz;
    tsdf_unflatten(vol, live ? (int)j : 0, ix, iy, iz);
    const f3 c = tsdf_centre(vol.origin + 3 * b, ix, iy, iz, vol.v);
    const int64_t HW = (int64_t)fr.H * fr.W;
    int pix;
    float sdf;
    int n0 = 0;  // updates of this voxel by the frames before the chunk
    for (int s = 0; s < fr.l0; s += TSDF_CHUNK) {
        const int n = min(TSDF_CHUNK, fr.l0 - s);
        __syncthreads();
        tsdf_load_cams(cams, fr, b, s, n);
        if (live)
            for (int l = 0; l < n; ++l)
                if (tsdf_observe(cams[l], c, fr.depth + ((int64_t)b * fr.L + s + l) * HW, fr, vol.trunc, pix, sdf)) ++n0;
    }
    __syncthreads();
    tsdf_load_cams(cams, fr, b, fr.l0, fr.Lc);
    uint32_t mask = 0;
    if (live)
        for (int l = 0; l < fr.Lc; ++l)
            if (tsdf_observe(cams[l], c, fr.depth + ((int64_t)b * fr.L + fr.l0 + l) * HW, fr, vol.trunc, pix, sdf)) mask |= 1u << l;
    const bool color = g_color_src != nullptr;
    float g = live ? g_tsdf_src[at] : 0.0f;
    f3 gc = (live && color) ? ld3(g_color_src, at) : f3{0.0f, 0.0f, 0.0f};
    const float W0 = live ? weight_in[at] : 0.0f;
    const int E = (ACC && FOLD) ? det_scale(*fold.maxbits, lg) : 0;
    uint32_t mx = 0;
    for (int l = fr.Lc - 1; l >= 0; --l) {
        const bool on = (mask >> l) & 1u;
        if (!POSE && !on) continue;
        float ps[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (on) {
            tsdf_observe(cams[l], c, fr.depth + ((int64_t)b * fr.L + fr.l0 + l) * HW, fr, vol.trunc, pix, sdf);
            const float W = tsdf_weight_after(W0, n0 + __popc(mask & ((1u << l) - 1u)), vol.maxw);
            const float den = W + 1.0f, keep = W / den;
            const float gd = sdf < vol.trunc ? (g / den) / vol.trunc : 0.0f;  // t = 1 beyond trunc: no gradient
            const f3 gr{gc.x / den, gc.y / den, gc.z / den};
            g = g * keep;
            gc = f3{gc.x * keep, gc.y * keep, gc.z * keep};
            if (ACC && FOLD) {
                const int64_t p = ((int64_t)b * fr.Lc + l) * HW + pix;
                fold_add(fold, p, 0, gd, E);
                if (color) {
                    fold_add(fold, p, 1, gr.x, E);
                    fold_add(fold, p, 2, gr.y, E);
                    fold_add(fold, p, 3, gr.z, E);
                }
            } else if (!ACC) {
                mx = fold_max(mx, gd);
                if (color) mx = fold_max(fold_max(fold_max(mx, gr.x), gr.y), gr.z);
            }
            if (POSE) {  // z = sum_j R[j][2] (c_j - t_j) and dL/dz = -gd: the terms of S0 and S_j
                const float *P = fr.poses + ((int64_t)b * fr.L + fr.l0 + l) * 16;
                ps[0] = gd;
                ps[1] = gd * (c.x - P[3]);
                ps[2] = gd * (c.y - P[7]);
                ps[3] = gd * (c.z - P[11]);
            }
        }
        if (POSE) tsdf_pose_wave<4>(ps, on, red + l * TSDF_WAVES * 4);
    }
    if (ACC) {
        if (live) {
            if (g_tsdf_dst) g_tsdf_dst[at] = g;
            if (color && g_color_dst) st3(g_color_dst, at, gc);
        }
    } else {
        fold_max_commit(fold.maxbits, mx);
    }
    if (POSE) {
        __syncthreads();
        if ((int)threadIdx.x < 4 * fr.Lc) {
            const int l = threadIdx.x >> 2, n = threadIdx.x & 3;
            psum[(((int64_t)b * fr.Lc + l) * gridDim.x + blockIdx.x) * 4 + n] = block_row_sum<4, TSDF_WAVES>(red + l * TSDF_WAVES * 4, n);
        }
    }
}

// every pixel of the chunk's frames: each sum rounded once to fp32.  g_rgb may be NULL
__global__ __launch_bounds__(TSDF_T) void tsdf_fold_finish_k(Fold fold, int lg, int B, int L, int l0, int Lc, int64_t HW,
                                                             float *__restrict__ g_depth, float *__restrict__ g_rgb) {
    const int E = det_scale(*fold.maxbits, lg);
    const int64_t total = (int64_t)B * Lc * HW;
    for (int64_t p = (int64_t)blockIdx.x * TSDF_T + threadIdx.x; p < total; p += (int64_t)gridDim.x * TSDF_T) {
        const int64_t bl = p / HW, pix = p - bl * HW;
        const int b = (int)(bl / Lc), l = (int)(bl - (int64_t)b * Lc);
        const int64_t out = ((int64_t)b * L + l0 + l) * HW + pix;
        for (int ch = 0; ch < (g_rgb ? 4 : 1); ++ch) {
            const float r = fold_result(fold, p, ch, E);
            if (ch == 0) {
                if (g_depth) g_depth[out] = r;
            } else {
                g_rgb[3 * out + ch - 1] = r;
            }
        }
    }
}

// The pose adjoint of the chunk's cameras from their blocks' rows.  grid (x: frame of the chunk, y: batch element), TSDF_POSE_T
// threads.  With the sums S0 = sum gd, S_j = sum gd (c_j - t_j):  g_poses[b,l][j][2] = -S_j,  g_poses[b,l][j][3] = R[j][2] S0,
// every other entry 0.
__global__ __launch_bounds__(TSDF_POSE_T) void tsdf_pose_finish_k(const float *__restrict__ psum, int nrow, const float *__restrict__ poses,
                                                                  int L, int l0, int Lc, float *__restrict__ g_poses) {
    __shared__ float S[4];
    const int b = blockIdx.y, l = blockIdx.x;
    fold_rows<4, TSDF_POSE_GROUPS, 16>(psum + ((int64_t)b * Lc + l) * nrow * 4, nrow, 4, S);
    if (threadIdx.x < 16) {
        const int64_t cam = (int64_t)b * L + l0 + l;
        const int i = threadIdx.x >> 2, j = threadIdx.x & 3;
        float r = 0.0f;
        if (i < 3 && j == 2) r = -S[1 + i];
        if (i < 3 && j == 3) r = poses[cam * 16 + 4 * i + 2] * S[0];
        g_poses[cam * 16 + threadIdx.x] = r;
    }
}

// ------------------------------------------------------------------ E: extraction.  grid (x: compaction blocks, y: batch element)
struct TsdfState {
    const float *tsdf, *weight, *color;  // of ONE batch element; color may be NULL
    float minw;
};
struct TsdfCrossPred {
    TsdfVol vol;
    TsdfState s;
    __device__ bool operator()(int64_t e) const {
        TsdfEdge ed;
        if (!tsdf_edge(vol, e, ed)) return false;
        return tsdf_crosses(s.tsdf[ed.j], s.weight[ed.j], s.tsdf[ed.j1], s.weight[ed.j1], s.minw);
    }
};
// D_k(j): the difference of tsdf along one axis over the observed neighbours inside the grid (i: the voxel's index on that axis,
// n: the grid's size, stride: the neighbour's distance in voxels)
__device__ __forceinline__ float tsdf_diff(const TsdfState &s, int j, int i, int n, int stride) {
    const bool hp = i + 1 < n && s.weight[j + stride] >= s.minw, hm = i > 0 && s.weight[j - stride] >= s.minw;
    if (hp && hm) return 0.5f * (s.tsdf[j + stride] - s.tsdf[j - stride]);
    if (hp) return s.tsdf[j + stride] - s.tsdf[j];
    if (hm) return s.tsdf[j] - s.tsdf[j - stride];
    return 0.0f;
}
__device__ __forceinline__ f3 tsdf_grad(const TsdfVol &g, const TsdfState &s, int j, int ix, int iy, int iz) {
    return f3{tsdf_diff(s, j, ix, g.nx, 1), tsdf_diff(s, j, iy, g.ny, g.nx), tsdf_diff(s, j, iz, g.nz, g.nx * g.ny)};
}
struct TsdfRowWriter {
    TsdfVol vol;
    TsdfState s;
    const float *origin;  // of this batch element
    float *points, *normals, *colors;  // (cap, 3) of this batch element; colors may be NULL
    int32_t *edge;
    int cap;
    __device__ void operator()(int64_t e, int64_t pos) const {
        if (pos >= cap) return;
        TsdfEdge ed;
        tsdf_edge(vol, e, ed);
        const float f0 = s.tsdf[ed.j], f1 = s.tsdf[ed.j1];
        const float t = tsdf_cross_s(f0, f1);
        f3 p = tsdf_centre(origin, ed.ix, ed.iy, ed.iz, vol.v);
        if (ed.a == 0) p.x = p.x + t * vol.v;
        else if (ed.a == 1) p.y = p.y + t * vol.v;
        else p.z = p.z + t * vol.v;
        st3(points, pos, p);
        const f3 d0 = tsdf_grad(vol, s, ed.j, ed.ix, ed.iy, ed.iz);
        const f3 d1 = tsdf_grad(vol, s, ed.j1, ed.ix + (ed.a == 0), ed.iy + (ed.a == 1), ed.iz + (ed.a == 2));
        f3 n{d0.x + t * (d1.x - d0.x), d0.y + t * (d1.y - d0.y), d0.z + t * (d1.z - d0.z)};
        float nn = sqrtf(__fmaf_rn(n.z, n.z, __fmaf_rn(n.y, n.y, n.x * n.x)));  // (_compute_normal_map's rule: zero stays zero)
        nn = (nn == 0.0f) ? 1.0f : nn;
        st3(normals, pos, f3{n.x / nn, n.y / nn, n.z / nn});
        if (colors) {
            const f3 c0 = ld3(s.color, ed.j), c1 = ld3(s.color, ed.j1);
            st3(colors, pos, f3{c0.x + t * (c1.x - c0.x), c0.y + t * (c1.y - c0.y), c0.z + t * (c1.z - c0.z)});
        }
        edge[pos] = (int32_t)e;
    }
};
struct TsdfExtractWs {
    int *bcount, *boffset;  // B x nb each
    int nb;
};
static inline size_t tsdf_extract_layout(int B, int64_t nvox, void *ws, TsdfExtractWs *out) {
    const int nb = compact_blocks(3 * nvox);
    Carve c{(char *)ws};
    int *bcount = c.take<int>(sizeof(int) * (size_t)B * nb);
    int *boffset = c.take<int>(sizeof(int) * (size_t)B * nb);
    if (out) *out = TsdfExtractWs{bcount, boffset, nb};
    return c.off;
}
__device__ __forceinline__ TsdfState tsdf_state_of(const float *tsdf, const float *weight, const float *color, float minw, int b, int64_t nvox) {
    return TsdfState{tsdf + b * nvox, weight + b * nvox, color ? color + 3 * b * nvox : nullptr, minw};
}

__global__ __launch_bounds__(kCT) void tsdf_count_k(TsdfVol vol, const float *__restrict__ tsdf, const float *__restrict__ weight, float minw,
                                                    TsdfExtractWs w) {
    const int b = blockIdx.y;
    const int64_t nvox = tsdf_nvox(vol);
    const TsdfCrossPred pred{vol, tsdf_state_of(tsdf, weight, nullptr, minw, b, nvox)};
    compact_count_body(3 * nvox, pred, w.bcount + (int64_t)b * w.nb, (unsigned char *)nullptr, (int)blockIdx.x, w.nb);
}
// grid (x: batch element), one block each; the total is n_points[b]
__global__ __launch_bounds__(1024) void tsdf_scan_k(TsdfExtractWs w, int32_t *__restrict__ n_points) {
    const int b = blockIdx.x;
    compact_scan_body(w.bcount + (int64_t)b * w.nb, w.nb, w.boffset + (int64_t)b * w.nb, (int *)(n_points + b));
}
__global__ __launch_bounds__(kCT) void tsdf_write_k(TsdfVol vol, const float *__restrict__ tsdf, const float *__restrict__ weight,
                                                    const float *__restrict__ color, float minw, TsdfExtractWs w, int cap,
                                                    float *__restrict__ points, float *__restrict__ normals, float *__restrict__ colors,
                                                    int32_t *__restrict__ edge) {
    const int b = blockIdx.y;
    const int64_t nvox = tsdf_nvox(vol), row0 = (int64_t)b * cap;
    const TsdfState s = tsdf_state_of(tsdf, weight, color, minw, b, nvox);
    const TsdfCrossPred pred{vol, s};
    const TsdfRowWriter wr{vol, s, vol.origin + 3 * b, points + 3 * row0, normals + 3 * row0, (colors && color) ? colors + 3 * row0 : nullptr,
                           edge + row0, cap};
    compact_write_body<TsdfCrossPred, TsdfRowWriter, false>(3 * nvox, pred, wr, w.boffset + (int64_t)b * w.nb, (int *)nullptr,
                                                            (const unsigned char *)nullptr, (int)blockIdx.x, w.nb);
}

// One (axis, end) pass of the reverse pass: rows whose edge runs along `axis` add into the voxel at their end `end`.  A voxel is
// end 0 of at most one edge per axis and end 1 of at most one: no two rows of a pass meet.  grid (x: rows, y: batch element)
__global__ __launch_bounds__(TSDF_T) void tsdf_extract_bwd_k(TsdfVol vol, const float *__restrict__ tsdf, const float *__restrict__ color,
                                                             const int32_t *__restrict__ edge, const int32_t *__restrict__ n_points, int cap,
                                                             const float *__restrict__ g_points, const float *__restrict__ g_colors, int axis,
                                                             int end, float *g_tsdf, float *g_color) {
    const int b = blockIdx.y, n = min(max(n_points[b], 0), cap);
    const int r = blockIdx.x * TSDF_T + threadIdx.x;
    if (r >= n) return;
    const int64_t nvox = tsdf_nvox(vol), row = (int64_t)b * cap + r;
    const int64_t e = edge[row];
    TsdfEdge ed;
    if (e < 0 || e >= 3 * nvox || !tsdf_edge(vol, e, ed) || ed.a != axis) return;
    const float *f = tsdf + b * nvox;
    const float f0 = f[ed.j], f1 = f[ed.j1];
    const float t = tsdf_cross_s(f0, f1), den = (f0 - f1) * (f0 - f1);
    const f3 gp = g_points ? ld3(g_points, row) : f3{0.0f, 0.0f, 0.0f};
    float gs = vol.v * (axis == 0 ? gp.x : (axis == 1 ? gp.y : gp.z));
    const int64_t at = b * nvox + (end ? ed.j1 : ed.j);
    if (g_colors && color) {
        const f3 gc = ld3(g_colors, row);
        const f3 c0 = ld3(color, b * nvox + ed.j), c1 = ld3(color, b * nvox + ed.j1);
        gs = ((gs + gc.x * (c1.x - c0.x)) + gc.y * (c1.y - c0.y)) + gc.z * (c1.z - c0.z);
        const float m = end ? t : (-f1) / (f0 - f1);  // 1 - s, without the cancellation of 1.0f - t near s = 1
        const f3 old = ld3(g_color, at);
        st3(g_color, at, f3{old.x + m * gc.x, old.y + m * gc.y, old.z + m * gc.z});
    }
    g_tsdf[at] = g_tsdf[at] + gs * (end ? f0 / den : (-f1) / den);
}

// ------------------------------------------------------------------ R: ray casting.  grid (x: 16x16 tiles of output pixels, y: frame, z: batch element)
struct TsdfCast {
    const float *K, *poses;  // (B,4,4), (B,L,4,4)
    int L, Ho, Wo, s, kmax;  // kmax: the most samples a thread visits
    float step, near, far, minw;
};
constexpr int TSDF_KMAX = 1 << 30;  // samples per ray: the tape is int32
constexpr int TSDF_CAST_TILES = 1 << 22;  // 16x16 tiles per image: grid.x x 256 threads stays below 2^32

// A block of 256 threads covers 16x16 output pixels and each of its 4 waves a compact 8x8 tile, not a 64x1 row: neighbouring rays
// read neighbouring voxels, so the 16 gathers of a sample share cache lines.
__device__ __forceinline__ bool tsdf_cast_pixel(const TsdfCast &c, int &i, int &j) {
    const int tx = (c.Wo + 15) >> 4, by = blockIdx.x / tx, bx = blockIdx.x - by * tx;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    i = by * 16 + (wave >> 1) * 8 + (lane >> 3);
    j = bx * 16 + (wave & 1) * 8 + (lane & 7);
    return i < c.Ho && j < c.Wo;
}

// The samples [ka, kb] outside of which none is inside the grid: the ray clipped against the three slabs of the box
// [o, o + n v], which is half a voxel wider on every side than the positions with a cell, so that the rounding of (lo - t) (far
// less than v / 2 unless |t| > 2^20 v) cannot cut a cell off however small dw is; then widened by one sample and 2^-21 of the
// index on each side for the roundings of the divisions and of k dz.  A ray parallel to an axis (dw_i == 0) is inside that slab
// for every z or for none: no division, and no infinity or NaN decides anything (fminf / fmaxf drop a NaN, the conversions clamp
// in float first and send a NaN to the empty side).  At most kmax samples are visited whatever the arithmetic gave: samples are
// `step` apart and the box's longest chord is below (nx + ny + nz) v.
__device__ __forceinline__ void tsdf_cast_range(const TsdfVol &g, const float *__restrict__ o, const TsdfRay &r, const TsdfCast &c, int &ka,
                                                int &kb) {
    const float t[3] = {r.t.x, r.t.y, r.t.z}, d[3] = {r.dw.x, r.dw.y, r.dw.z};
    const int n[3] = {g.nx, g.ny, g.nz};
    float zin = c.near, zout = c.far;
    bool any = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float lo = o[a], hi = o[a] + (float)n[a] * g.v;
        if (d[a] == 0.0f) {
            any = any && t[a] >= lo && t[a] <= hi;
        } else {
            const float z0 = (lo - t[a]) / d[a], z1 = (hi - t[a]) / d[a];
            zin = fmaxf(zin, fminf(z0, z1));
            zout = fminf(zout, fmaxf(z0, z1));
        }
    }
    ka = 1;
    kb = 0;
    if (!any || !(zin <= zout)) return;
    const float qa = zin / r.dz, qb = zout / r.dz;
    const float fa = floorf(qa - qa * 0x1p-21f) - 1.0f, fb = ceilf(qb + qb * 0x1p-21f) + 1.0f;
    ka = fa >= 1.0f ? (fa < (float)TSDF_KMAX ? (int)fa : TSDF_KMAX) : 1;
    kb = fb >= 0.0f ? (fb < (float)TSDF_KMAX ? (int)fb : TSDF_KMAX - 1) : 0;
    kb = min(kb, TSDF_KMAX - 1);
    if (kb - ka >= c.kmax) kb = ka + c.kmax - 1;
}

template <bool COLOR>
__global__ __launch_bounds__(TSDF_T) void tsdf_raycast_k(TsdfVol vol, TsdfCast cast, const float *__restrict__ tsdf, const float *__restrict__ weight,
                                                         const float *__restrict__ color, float *__restrict__ depth, float *__restrict__ normal,
                                                         float *__restrict__ rgb, int32_t *__restrict__ k_end) {
    int i, j;
    if (!tsdf_cast_pixel(cast, i, j)) return;
    const int l = blockIdx.y, b = blockIdx.z;
    const int64_t nvox = tsdf_nvox(vol), pix = (((int64_t)b * cast.L + l) * cast.Ho + i) * cast.Wo + j;
    const float *o = vol.origin + 3 * b, *f_b = tsdf + b * nvox, *w_b = weight + b * nvox;
    const TsdfRay ray = tsdf_ray(cast.K + 16 * b, cast.poses + ((int64_t)b * cast.L + l) * 16, i * cast.s, j * cast.s, cast.step);
    int ka, kb;
    tsdf_cast_range(vol, o, ray, cast, ka, kb);
    bool prev_ok = false;  // sample k - 1 belongs to the ray, is observed and has f >= 0 (a skipped sample is an unobserved one)
    float f_prev = 0.0f, z = 0.0f;
    int kend = 0;
    TsdfCell c, hc;
    for (int k = ka; k <= kb; ++k) {
        const float zk = tsdf_ray_z(ray, k);
        if (!(zk >= cast.near)) continue;
        if (!(zk <= cast.far)) break;
        float f;
        if (!tsdf_sample_at(vol, o, f_b, w_b, cast.minw, tsdf_ray_at(ray, zk), c, f)) {
            prev_ok = false;
            continue;
        }
        if (f < 0.0f) {
            if (prev_ok && tsdf_hit_at(vol, o, w_b, cast.minw, ray, k, f_prev, f, z, hc)) kend = k;
            break;
        }
        prev_ok = f >= 0.0f;
        f_prev = f;
    }
    f3 nrm{0.0f, 0.0f, 0.0f}, col{0.0f, 0.0f, 0.0f};
    if (kend) {
        float f8[8];
        tsdf_gather8(vol, f_b, hc.j, f8);
        const f3 g = tsdf_trigrad(f8, hc);  // +grad f: the tsdf is positive in free space
        const float nn = sqrtf((g.x * g.x + g.y * g.y) + g.z * g.z);
        if (nn > 0.0f) nrm = f3{g.x / nn, g.y / nn, g.z / nn};
        else kend = 0;  // a zero (or NaN) gradient: a miss
    }
    if (COLOR && kend) {
        const float *c_b = color + 3 * b * nvox;
        float c8[8];
        tsdf_gather8c(vol, c_b, hc.j, 0, c8);
        col.x = tsdf_trilerp(c8, hc);
        tsdf_gather8c(vol, c_b, hc.j, 1, c8);
        col.y = tsdf_trilerp(c8, hc);
        tsdf_gather8c(vol, c_b, hc.j, 2, c8);
        col.z = tsdf_trilerp(c8, hc);
    }
    depth[pix] = kend ? z : 0.0f;
    st3(normal, pix, nrm);
    if (COLOR) st3(rgb, pix, col);
    k_end[pix] = kend;
}

// The fold of the reverse pass: per voxel (b, j) nch sums (tsdf; r, g, b).  With `poses` (the workspace of
// gs_tsdf_raycast_backward_poses; L and tiles count for it alone) behind it: one row of 12 pose sums per (b, l, 16x16 tile)
struct TsdfCastBwdWs {
    Fold fold;
    size_t fold_bytes;
    float *psum;
};
static inline size_t tsdf_cast_bwd_layout(int B, int64_t nvox, int nch, bool poses, int L, int tiles, void *ws, TsdfCastBwdWs *out) {
    Carve c{(char *)ws};
    TsdfCastBwdWs scratch, &r = out ? *out : scratch;
    r.fold = fold_carve(c, (size_t)B * nvox, nch);
    r.fold_bytes = c.off;
    r.psum = poses ? c.take<float>(sizeof(float) * 12 * (size_t)B * L * tiles) : nullptr;
    return c.off;
}
// one term of voxel p: into the maximum, or into the sums
template <bool ACC>
__device__ __forceinline__ void tsdf_cast_term(const Fold &fold, int64_t p, int ch, float x, int E, uint32_t &mx) {
    if (ACC) fold_add(fold, p, ch, x, E);
    else mx = fold_max(mx, x);
}

// One thread per output pixel: the two samples and the hit are recomputed from the tape k_end through the forward's bodies.
// ACC = false: the largest finite |term|; ACC = true: the terms go into the fold.  No thread leaves before the wave's reduction.
// POSE (the second pass of gs_tsdf_raycast_backward_poses): the block's 12 pose sums go to row ((b L + l) gridDim.x + blockIdx.x)
// of `psum` (gs_tsdf.hpp: the pose sums), 3 i + j: (z0 u0 + z1 u1 + z* w)_i d_j, 9 + i: (u0 + u1 + w)_i; FOLD = false: nothing
// goes into the fold.
template <bool ACC, bool POSE = false, bool FOLD = true>
__global__ __launch_bounds__(TSDF_T) void tsdf_raycast_bwd_k(TsdfVol vol, TsdfCast cast, const float *__restrict__ tsdf,
                                                             const float *__restrict__ weight, const float *__restrict__ color,
                                                             const int32_t *__restrict__ k_end, const float *__restrict__ g_depth,
                                                             const float *__restrict__ g_rgb, Fold fold, int lg,
                                                             float *__restrict__ psum = nullptr) {
    __shared__ float red[POSE ? TSDF_WAVES * 12 : 1];
    int i, j;
    const bool live = tsdf_cast_pixel(cast, i, j);
    const int l = blockIdx.y, b = blockIdx.z;
    const int64_t nvox = tsdf_nvox(vol), pix = (((int64_t)b * cast.L + l) * cast.Ho + i) * cast.Wo + j;
    const float *o = vol.origin + 3 * b, *f_b = tsdf + b * nvox, *w_b = weight + b * nvox;
    const int E = (ACC && FOLD) ? det_scale(*fold.maxbits, lg) : 0;
    uint32_t mx = 0;
    float ps[12] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    bool hit = false;
    const int k = live ? k_end[pix] : 0;
    if (k >= 2 && k < TSDF_KMAX) {
        const TsdfRay ray = tsdf_ray(cast.K + 16 * b, cast.poses + ((int64_t)b * cast.L + l) * 16, i * cast.s, j * cast.s, cast.step);
        TsdfCell c0, c1, hc;
        float f0, f1, z;
        const float z0 = tsdf_ray_z(ray, k - 1), z1 = tsdf_ray_z(ray, k);
        // (a tape that does not belong to this volume fails these tests; every gather stays behind tsdf_cell's bounds)
        if (tsdf_sample_at(vol, o, f_b, w_b, cast.minw, tsdf_ray_at(ray, z0), c0, f0) &&
            tsdf_sample_at(vol, o, f_b, w_b, cast.minw, tsdf_ray_at(ray, z1), c1, f1) && f0 >= 0.0f && f1 < 0.0f &&
            tsdf_hit_at(vol, o, w_b, cast.minw, ray, k, f0, f1, z, hc)) {
            hit = true;
            float gz = g_depth ? g_depth[pix] : 0.0f;
            const bool col = color != nullptr && g_rgb != nullptr;
            f3 gc{0.0f, 0.0f, 0.0f}, wv{0.0f, 0.0f, 0.0f};
            if (col) {
                const float *c_b = color + 3 * b * nvox;
                gc = ld3(g_rgb, pix);
                const float gch[3] = {gc.x, gc.y, gc.z};
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {  // g_z = g_depth + sum_ch g_rgb_ch (grad C_ch(p*) . dw) / v
                    float c8[8];
                    tsdf_gather8c(vol, c_b, hc.j, ch, c8);
                    const f3 g = tsdf_trigrad(c8, hc);
                    gz = gz + gch[ch] * (((g.x * ray.dw.x + g.y * ray.dw.y) + g.z * ray.dw.z) / vol.v);
                    if (POSE) wv = f3{wv.x + gch[ch] * (g.x / vol.v), wv.y + gch[ch] * (g.y / vol.v), wv.z + gch[ch] * (g.z / vol.v)};
                }
            }
            const float den = f0 - f1, den2 = den * den, gs = gz * ray.dz;
            const float a0 = gs * ((-f1) / den2), a1 = gs * (f0 / den2);
            const int64_t at = b * nvox;
            if (!ACC || FOLD) {
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    tsdf_cast_term<ACC>(fold, at + tsdf_corner(vol, c0.j, c), 0, a0 * tsdf_corner_weight(c0, c), E, mx);
                    tsdf_cast_term<ACC>(fold, at + tsdf_corner(vol, c1.j, c), 0, a1 * tsdf_corner_weight(c1, c), E, mx);
                    if (col && fold.nch == 4) {
                        const float w = tsdf_corner_weight(hc, c);
                        const int64_t p = at + tsdf_corner(vol, hc.j, c);
                        tsdf_cast_term<ACC>(fold, p, 1, gc.x * w, E, mx);
                        tsdf_cast_term<ACC>(fold, p, 2, gc.y * w, E, mx);
                        tsdf_cast_term<ACC>(fold, p, 3, gc.z * w, E, mx);
                    }
                }
            }
            if (POSE) {  // p = t + z R d: u0 = a0 grad F(p0) / v, u1 = a1 grad F(p1) / v, w = sum_ch g_rgb_ch grad C_ch(p*) / v
                float f8[8], dx, dy;
                tsdf_gather8(vol, f_b, c0.j, f8);
                const f3 t0 = tsdf_trigrad(f8, c0);
                tsdf_gather8(vol, f_b, c1.j, f8);
                const f3 t1 = tsdf_trigrad(f8, c1);
                tsdf_ray_dir(cast.K + 16 * b, i * cast.s, j * cast.s, dx, dy);
                const float u0[3] = {a0 * (t0.x / vol.v), a0 * (t0.y / vol.v), a0 * (t0.z / vol.v)};
                const float u1[3] = {a1 * (t1.x / vol.v), a1 * (t1.y / vol.v), a1 * (t1.z / vol.v)};
                const float w3[3] = {wv.x, wv.y, wv.z};
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float q = (z0 * u0[a] + z1 * u1[a]) + z * w3[a];
                    ps[3 * a] = q * dx;
                    ps[3 * a + 1] = q * dy;
                    ps[3 * a + 2] = q;
                    ps[9 + a] = (u0[a] + u1[a]) + w3[a];
                }
            }
        }
    }
    if (!ACC) fold_max_commit(fold.maxbits, mx);
    if (POSE) {
        tsdf_pose_wave<12>(ps, hit, red);
        __syncthreads();
        if (threadIdx.x < 12)
            psum[((((int64_t)b * cast.L + l) * gridDim.x) + blockIdx.x) * 12 + threadIdx.x] = block_row_sum<12, TSDF_WAVES>(red, threadIdx.x);
    }
}

// The pose adjoint of every camera from its blocks' rows.  grid (x: frame, y: batch element), TSDF_POSE_T threads.  Sum 3 i + j
// is entry [i][j] of the rotation, sum 9 + i entry [i][3]; row 3 is zero.
__global__ __launch_bounds__(TSDF_POSE_T) void tsdf_cast_pose_finish_k(const float *__restrict__ psum, int nrow, float *__restrict__ g_poses) {
    __shared__ float S[12];
    const int64_t cam = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    fold_rows<12, TSDF_POSE_GROUPS, 16>(psum + cam * nrow * 12, nrow, 12, S);
    if (threadIdx.x < 16) {
        const int i = threadIdx.x >> 2, j = threadIdx.x & 3;
        g_poses[cam * 16 + threadIdx.x] = i == 3 ? 0.0f : S[j == 3 ? 9 + i : 3 * i + j];
    }
}

// every voxel: each sum rounded once to fp32.  g_color may be NULL
__global__ __launch_bounds__(TSDF_T) void tsdf_cast_finish_k(Fold fold, int lg, int64_t total, float *__restrict__ g_tsdf,
                                                             float *__restrict__ g_color) {
    const int E = det_scale(*fold.maxbits, lg);
    for (int64_t p = (int64_t)blockIdx.x * TSDF_T + threadIdx.x; p < total; p += (int64_t)gridDim.x * TSDF_T) {
        for (int ch = 0; ch < fold.nch; ++ch) {
            const float r = fold_result(fold, p, ch, E);
            if (ch == 0) g_tsdf[p] = r;
            else if (g_color) g_color[3 * p + ch - 1] = r;
        }
    }
}

static inline bool tsdf_vol_ok(int B, int nx, int ny, int nz) {
    return B > 0 && B <= 65535 && nx > 0 && ny > 0 && nz > 0 && (int64_t)nx * ny * nz <= TSDF_NMAX;
}
static inline bool tsdf_pos(float x) { return x > 0.0f && x < INFINITY; }
static inline bool tsdf_aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
static inline TsdfFrames tsdf_frames(const float *depth, const float *rgb, const float *K, const float *poses, int L, int H, int W) {
    return TsdfFrames{depth, rgb, K, poses, L, H, W, 0, 0, (float)((double)W - 0.999), (float)((double)H - 0.999)};
}

}  // namespace gs

using namespace gs;

// (name: a const char *, so that the drivers two entries share can pass their caller's on)
#define TSDF_REQUIRE_VOLUME(name)                                                                                                          \
    GS_REQUIRE(tsdf_vol_ok(B, nx, ny, nz), "%s: bad volume B=%d dims=(%d, %d, %d) (1 <= B <= 65535, nx ny nz <= 2^29)", name, B, nx, ny, nz); \
    GS_REQUIRE(tsdf_pos(voxel_size), "%s: voxel_size must be finite and positive, got %g", name, (double)voxel_size)
#define TSDF_REQUIRE_FRAMES(name)                                                                                           \
    GS_REQUIRE(L > 0 && H > 0 && W > 0 && (int64_t)H * W <= INT32_MAX, "%s: bad frames L=%d H=%d W=%d", name, L, H, W);      \
    GS_REQUIRE(tsdf_pos(trunc) && tsdf_pos(max_weight), "%s: trunc and max_weight must be finite and positive, got %g and %g", name, \
               (double)trunc, (double)max_weight)
// "<name>/<stage>": what GS_HIP and GS_LAUNCH_CHECK report from a shared driver (built only when they report)
struct TsdfStage {
    char text[64];
    TsdfStage(const char *name, const char *stage) { snprintf(text, sizeof text, "%s/%s", name, stage); }
};

extern "C" {

int gs_tsdf_integrate(const float *depth, const float *rgb, const float *intrinsics, const float *poses, int B, int L, int H, int W, int nx,
                      int ny, int nz, float voxel_size, const float *origin, float trunc, float max_weight, const float *tsdf_in,
                      const float *weight_in, const float *color_in, float *tsdf_out, float *weight_out, float *color_out,
                      gs_stream_t stream) {
    GS_REQUIRE(depth && intrinsics && poses && origin && tsdf_in && weight_in && tsdf_out && weight_out, "gs_tsdf_integrate: NULL argument");
    GS_REQUIRE((color_in != nullptr) == (color_out != nullptr) && (!color_in || rgb),
               "gs_tsdf_integrate: color_in, color_out and rgb go together");
    TSDF_REQUIRE_VOLUME("gs_tsdf_integrate");
    TSDF_REQUIRE_FRAMES("gs_tsdf_integrate");
    const TsdfVol vol{nx, ny, nz, voxel_size, trunc, max_weight, origin};
    TsdfFrames fr = tsdf_frames(depth, color_in ? rgb : nullptr, intrinsics, poses, L, H, W);
    const bool vec = nx % 4 == 0 && tsdf_aligned16(tsdf_in) && tsdf_aligned16(weight_in) && tsdf_aligned16(color_in) &&
                     tsdf_aligned16(tsdf_out) && tsdf_aligned16(weight_out) && tsdf_aligned16(color_out);
    const dim3 grid(cdiv((int64_t)((nx + 3) / 4) * ny * nz, TSDF_T), B);
    for (int l0 = 0; l0 < L; l0 += TSDF_CHUNK) {  // later chunks continue on the outputs
        fr.l0 = l0;
        fr.Lc = std::min(TSDF_CHUNK, L - l0);
        const float *ti = l0 ? tsdf_out : tsdf_in, *wi = l0 ? weight_out : weight_in, *ci = l0 ? color_out : color_in;
        auto k = color_in ? (vec ? tsdf_integrate_k<true, true> : tsdf_integrate_k<false, true>)
                          : (vec ? tsdf_integrate_k<true, false> : tsdf_integrate_k<false, false>);
        hipLaunchKernelGGL(k, grid, dim3(TSDF_T), 0, (hipStream_t)stream, vol, fr, ti, wi, ci, tsdf_out, weight_out, color_out);
        GS_LAUNCH_CHECK("gs_tsdf_integrate");
    }
    return GS_OK;
}

// The reverse pass of the integration behind both entries (their NULL rules come first).  g_poses == NULL: the second pass is
// tsdf_bwd_k<ACC>, without the pose sums and their finish.  What nobody asked for is not computed; adjoints the caller gives no
// g_tsdf_in / g_color_in for are carried from chunk to chunk in the workspace.
static int tsdf_integrate_backward_run(const char *name, const float *depth, const float *intrinsics, const float *poses, int B, int L, int H,
                                       int W, int nx, int ny, int nz, float voxel_size, const float *origin, float trunc, float max_weight,
                                       const float *weight_in, const float *g_tsdf_out, const float *g_color_out, float *g_tsdf_in,
                                       float *g_color_in, float *g_depth, float *g_rgb, float *g_poses /* may be NULL */, void *ws,
                                       size_t ws_bytes, size_t need /* the entry's own size query */, gs_stream_t stream) {
    TSDF_REQUIRE_VOLUME(name);
    TSDF_REQUIRE_FRAMES(name);
    GS_REQUIRE_WS(name, ws, ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const bool pose = g_poses != nullptr;
    const TsdfVol vol{nx, ny, nz, voxel_size, trunc, max_weight, origin};
    const int64_t nvox = tsdf_nvox(vol), HW = (int64_t)H * W;
    TsdfFrames fr = tsdf_frames(depth, nullptr, intrinsics, poses, L, H, W);
    TsdfBwdWs w;
    tsdf_bwd_layout(B, L, H, W, pose, nvox, g_color_out != nullptr, ws, &w);
    const bool fold = g_depth || g_rgb, color = g_color_out && (g_color_in || g_rgb);
    float *dst_t = g_tsdf_in ? g_tsdf_in : w.carry_t, *dst_c = color ? (g_color_in ? g_color_in : w.carry_c) : nullptr;
    const int lg = fold_lg(nvox);  // a pixel receives at most one term per voxel
    const int nblk = cdiv(nvox, TSDF_T);
    const dim3 grid(nblk, B);
    const int last = (L - 1) / TSDF_CHUNK * TSDF_CHUNK;
    auto second = !pose ? tsdf_bwd_k<true> : (fold ? tsdf_bwd_k<true, true, true> : tsdf_bwd_k<true, true, false>);
    for (int l0 = last; l0 >= 0; l0 -= TSDF_CHUNK) {  // the last chunk starts from the upstream adjoints, the others from the carried ones
        fr.l0 = l0;
        fr.Lc = std::min(TSDF_CHUNK, L - l0);
        const float *gt = l0 == last ? g_tsdf_out : dst_t, *gc = color ? (l0 == last ? g_color_out : dst_c) : nullptr;
        if (fold) {
            GS_HIP(hipMemsetAsync(ws, 0, w.fold_bytes, st), TsdfStage(name, "zero").text);
            hipLaunchKernelGGL(tsdf_bwd_k<false>, grid, dim3(TSDF_T), 0, st, vol, fr, weight_in, gt, gc, dst_t, dst_c, w.fold, lg);
        }
        hipLaunchKernelGGL(second, grid, dim3(TSDF_T), 0, st, vol, fr, weight_in, gt, gc, dst_t, dst_c, w.fold, lg, w.psum);
        GS_LAUNCH_CHECK(TsdfStage(name, "fold").text);
        if (fold)
            hipLaunchKernelGGL(tsdf_fold_finish_k, dim3(std::min(cdiv((int64_t)B * fr.Lc * HW, TSDF_T), 4096)), dim3(TSDF_T), 0, st, w.fold, lg,
                               B, L, l0, fr.Lc, HW, g_depth, g_rgb);
        if (pose)
            hipLaunchKernelGGL(tsdf_pose_finish_k, dim3(fr.Lc, B), dim3(TSDF_POSE_T), 0, st, (const float *)w.psum, nblk, poses, L, l0, fr.Lc,
                               g_poses);
        GS_LAUNCH_CHECK(TsdfStage(name, "finish").text);
    }
    return GS_OK;
}

size_t gs_tsdf_integrate_backward_ws_bytes(int B, int L, int H, int W) {
    if (B <= 0 || B > 65535 || L <= 0 || H <= 0 || W <= 0) return 0;
    return tsdf_bwd_layout(B, L, H, W, false, 0, false, nullptr, nullptr);
}

int gs_tsdf_integrate_backward(const float *depth, const float *intrinsics, const float *poses, int B, int L, int H, int W, int nx, int ny,
                               int nz, float voxel_size, const float *origin, float trunc, float max_weight, const float *weight_in,
                               const float *g_tsdf_out, const float *g_color_out, float *g_tsdf_in, float *g_color_in, float *g_depth,
                               float *g_rgb, void *ws, size_t ws_bytes, gs_stream_t stream) {
    GS_REQUIRE(depth && intrinsics && poses && origin && weight_in && g_tsdf_out && g_tsdf_in && g_depth,
               "gs_tsdf_integrate_backward: NULL argument");
    GS_REQUIRE((g_color_out != nullptr) == (g_color_in != nullptr) && (g_color_out != nullptr) == (g_rgb != nullptr),
               "gs_tsdf_integrate_backward: g_color_out, g_color_in and g_rgb go together");
    return tsdf_integrate_backward_run("gs_tsdf_integrate_backward", depth, intrinsics, poses, B, L, H, W, nx, ny, nz, voxel_size, origin,
                                       trunc, max_weight, weight_in, g_tsdf_out, g_color_out, g_tsdf_in, g_color_in, g_depth, g_rgb, nullptr,
                                       ws, ws_bytes, gs_tsdf_integrate_backward_ws_bytes(B, L, H, W), stream);
}

size_t gs_tsdf_integrate_backward_poses_ws_bytes(int B, int L, int H, int W, int nx, int ny, int nz, int has_color) {
    if (!tsdf_vol_ok(B, nx, ny, nz) || L <= 0 || H <= 0 || W <= 0) return 0;
    return tsdf_bwd_layout(B, L, H, W, true, (int64_t)nx * ny * nz, has_color != 0, nullptr, nullptr);
}

int gs_tsdf_integrate_backward_poses(const float *depth, const float *intrinsics, const float *poses, int B, int L, int H, int W, int nx,
                                     int ny, int nz, float voxel_size, const float *origin, float trunc, float max_weight,
                                     const float *weight_in, const float *g_tsdf_out, const float *g_color_out, float *g_tsdf_in,
                                     float *g_color_in, float *g_depth, float *g_rgb, float *g_poses, void *ws, size_t ws_bytes,
                                     gs_stream_t stream) {
    GS_REQUIRE(depth && intrinsics && poses && origin && weight_in && g_tsdf_out && g_poses, "gs_tsdf_integrate_backward_poses: NULL argument");
    GS_REQUIRE(g_color_out || (!g_color_in && !g_rgb), "gs_tsdf_integrate_backward_poses: g_color_in and g_rgb need g_color_out");
    return tsdf_integrate_backward_run("gs_tsdf_integrate_backward_poses", depth, intrinsics, poses, B, L, H, W, nx, ny, nz, voxel_size,
                                       origin, trunc, max_weight, weight_in, g_tsdf_out, g_color_out, g_tsdf_in, g_color_in, g_depth, g_rgb,
                                       g_poses, ws, ws_bytes,
                                       gs_tsdf_integrate_backward_poses_ws_bytes(B, L, H, W, nx, ny, nz, g_color_out != nullptr), stream);
}

size_t gs_tsdf_extract_ws_bytes(int B, int nx, int ny, int nz) {
    if (!tsdf_vol_ok(B, nx, ny, nz)) return 0;
    return tsdf_extract_layout(B, (int64_t)nx * ny * nz, nullptr, nullptr);
}

int gs_tsdf_extract(const float *tsdf, const float *weight, const float *color, int B, int nx, int ny, int nz, float voxel_size,
                    const float *origin, float min_weight, int cap, float *points, float *normals, float *colors, int32_t *edge,
                    int32_t *n_points, void *ws, size_t ws_bytes, gs_stream_t stream) {
    GS_REQUIRE(tsdf && weight && origin && n_points, "gs_tsdf_extract: NULL argument");
    GS_REQUIRE(cap >= 0 && (cap == 0 || (points && normals && edge)), "gs_tsdf_extract: cap = %d rows need points, normals and edge", cap);
    TSDF_REQUIRE_VOLUME("gs_tsdf_extract");
    GS_REQUIRE(min_weight == min_weight, "gs_tsdf_extract: min_weight must be a number");
    const size_t need = gs_tsdf_extract_ws_bytes(B, nx, ny, nz);
    GS_REQUIRE_WS("gs_tsdf_extract", ws, ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const TsdfVol vol{nx, ny, nz, voxel_size, 0.0f, 0.0f, origin};
    TsdfExtractWs w;
    tsdf_extract_layout(B, tsdf_nvox(vol), ws, &w);
    hipLaunchKernelGGL(tsdf_count_k, dim3(w.nb, B), dim3(kCT), 0, st, vol, tsdf, weight, min_weight, w);
    hipLaunchKernelGGL(tsdf_scan_k, dim3(B), dim3(1024), 0, st, w, n_points);
    GS_LAUNCH_CHECK("gs_tsdf_extract/count");
    if (cap > 0) {
        hipLaunchKernelGGL(tsdf_write_k, dim3(w.nb, B), dim3(kCT), 0, st, vol, tsdf, weight, color, min_weight, w, cap, points, normals, colors,
                           edge);
        GS_LAUNCH_CHECK("gs_tsdf_extract/write");
    }
    return GS_OK;
}

int gs_tsdf_extract_backward(const float *tsdf, const float *color, int B, int nx, int ny, int nz, float voxel_size, const int32_t *edge,
                             const int32_t *n_points, int cap, const float *g_points, const float *g_colors, float *g_tsdf, float *g_color,
                             gs_stream_t stream) {
    GS_REQUIRE(tsdf && edge && n_points && g_tsdf, "gs_tsdf_extract_backward: NULL argument");
    GS_REQUIRE((g_color == nullptr) || color, "gs_tsdf_extract_backward: g_color needs color");
    GS_REQUIRE(cap > 0, "gs_tsdf_extract_backward: cap must be positive, got %d", cap);
    TSDF_REQUIRE_VOLUME("gs_tsdf_extract_backward");
    hipStream_t st = (hipStream_t)stream;
    const TsdfVol vol{nx, ny, nz, voxel_size, 0.0f, 0.0f, nullptr};
    const int64_t n = (int64_t)B * tsdf_nvox(vol);
    GS_HIP(hipMemsetAsync(g_tsdf, 0, sizeof(float) * n, st), "gs_tsdf_extract_backward/zero");
    if (g_color) GS_HIP(hipMemsetAsync(g_color, 0, sizeof(float) * 3 * n, st), "gs_tsdf_extract_backward/zero");
    for (int axis = 0; axis < 3; ++axis)
        for (int end = 0; end < 2; ++end)
            hipLaunchKernelGGL(tsdf_extract_bwd_k, dim3(cdiv(cap, TSDF_T), B), dim3(TSDF_T), 0, st, vol, tsdf, g_color ? color : nullptr, edge,
                               n_points, cap, g_points, g_color ? g_colors : nullptr, axis, end, g_tsdf, g_color);
    GS_LAUNCH_CHECK("gs_tsdf_extract_backward");
    return GS_OK;
}

// the arguments a cast and its reverse pass share; kmax: the bound of a thread's loop
#define TSDF_REQUIRE_CAST(name)                                                                                                                \
    GS_REQUIRE(L > 0 && L <= 65535 && height > 0 && width > 0 && (int64_t)height * width <= INT32_MAX, "%s: bad frames L=%d H=%d W=%d", name, L, \
               height, width);                                                                                                                 \
    GS_REQUIRE(stride >= 1, "%s: stride must be at least 1, got %d", name, stride);                                                            \
    const int Ho = (int)(((int64_t)height + stride - 1) / stride), Wo = (int)(((int64_t)width + stride - 1) / stride);                         \
    GS_REQUIRE((int64_t)cdiv(Ho, 16) * cdiv(Wo, 16) <= TSDF_CAST_TILES, "%s: %d x %d output pixels need more than 2^22 tiles of 16 x 16", name, \
               Ho, Wo);                                                                                                                        \
    GS_REQUIRE(tsdf_pos(step), "%s: step must be finite and positive, got %g", name, (double)step);                                            \
    GS_REQUIRE(min_weight == min_weight, "%s: min_weight must be a number", name);                                                             \
    const double span = ((double)nx + ny + nz) * (double)voxel_size / (double)step;                                                            \
    GS_REQUIRE(span <= 1048576.0, "%s: (nx + ny + nz) voxel_size / step = %g exceeds 2^20 samples per ray", name, span)

int gs_tsdf_raycast(const float *tsdf, const float *weight, const float *color, int B, int nx, int ny, int nz, float voxel_size,
                    const float *origin, const float *intrinsics, const float *poses, int L, int height, int width, int stride, float step,
                    float near, float far, float min_weight, float *depth, float *normal, float *rgb, int32_t *k_end, gs_stream_t stream) {
    GS_REQUIRE(tsdf && weight && origin && intrinsics && poses && depth && normal && k_end, "gs_tsdf_raycast: NULL argument");
    GS_REQUIRE((color != nullptr) == (rgb != nullptr), "gs_tsdf_raycast: color and rgb go together");
    TSDF_REQUIRE_VOLUME("gs_tsdf_raycast");
    TSDF_REQUIRE_CAST("gs_tsdf_raycast");
    GS_REQUIRE(near >= 0.0f && far == far, "gs_tsdf_raycast: near must be a number >= 0 and far a number, got %g and %g", (double)near,
               (double)far);
    const TsdfVol vol{nx, ny, nz, voxel_size, 0.0f, 0.0f, origin};
    const TsdfCast cast{intrinsics, poses, L, Ho, Wo, stride, (int)span + 1040, step, near, far, min_weight};
    const dim3 grid(cdiv(Ho, 16) * cdiv(Wo, 16), L, B);
    hipLaunchKernelGGL(color ? tsdf_raycast_k<true> : tsdf_raycast_k<false>, grid, dim3(TSDF_T), 0, (hipStream_t)stream, vol, cast, tsdf,
                       weight, color, depth, normal, rgb, k_end);
    GS_LAUNCH_CHECK("gs_tsdf_raycast");
    return GS_OK;
}

// The reverse pass of a cast behind both entries (their NULL rules come first).  g_poses == NULL: the second pass is
// tsdf_raycast_bwd_k<ACC>, without the pose sums and their finish; g_tsdf == NULL (the pose entry allows it): no fold.
static int tsdf_raycast_backward_run(const char *name, const float *tsdf, const float *weight, const float *color, int B, int nx, int ny,
                                     int nz, float voxel_size, const float *origin, const float *intrinsics, const float *poses, int L,
                                     int height, int width, int stride, float step, float min_weight, const int32_t *k_end,
                                     const float *g_depth, const float *g_rgb, float *g_tsdf /* may be NULL */, float *g_color,
                                     float *g_poses /* may be NULL */, void *ws, size_t ws_bytes, size_t need /* the entry's own size query */,
                                     gs_stream_t stream) {
    TSDF_REQUIRE_VOLUME(name);
    TSDF_REQUIRE_CAST(name);
    GS_REQUIRE_WS(name, ws, ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const TsdfVol vol{nx, ny, nz, voxel_size, 0.0f, 0.0f, origin};
    const TsdfCast cast{intrinsics, poses, L, Ho, Wo, stride, 0, step, 0.0f, 0.0f, min_weight};
    const int tiles = cdiv(Ho, 16) * cdiv(Wo, 16);
    TsdfCastBwdWs w;
    tsdf_cast_bwd_layout(B, tsdf_nvox(vol), color ? 4 : 1, g_poses != nullptr, L, tiles, ws, &w);
    const int lg = fold_lg(2 * (int64_t)L * Ho * Wo);  // a voxel receives at most two terms per pixel of its batch element
    const int64_t total = (int64_t)B * tsdf_nvox(vol);
    const dim3 grid(tiles, L, B);
    if (g_tsdf) {
        GS_HIP(hipMemsetAsync(ws, 0, w.fold_bytes, st), TsdfStage(name, "zero").text);
        hipLaunchKernelGGL(tsdf_raycast_bwd_k<false>, grid, dim3(TSDF_T), 0, st, vol, cast, tsdf, weight, color, k_end, g_depth, g_rgb, w.fold, lg);
    }
    auto second = !g_poses ? tsdf_raycast_bwd_k<true> : (g_tsdf ? tsdf_raycast_bwd_k<true, true, true> : tsdf_raycast_bwd_k<true, true, false>);
    hipLaunchKernelGGL(second, grid, dim3(TSDF_T), 0, st, vol, cast, tsdf, weight, color, k_end, g_depth, g_rgb, w.fold, lg, w.psum);
    GS_LAUNCH_CHECK(TsdfStage(name, "fold").text);
    if (g_tsdf)
        hipLaunchKernelGGL(tsdf_cast_finish_k, dim3(std::min(cdiv(total, TSDF_T), 65536)), dim3(TSDF_T), 0, st, w.fold, lg, total, g_tsdf, g_color);
    if (g_poses) hipLaunchKernelGGL(tsdf_cast_pose_finish_k, dim3(L, B), dim3(TSDF_POSE_T), 0, st, (const float *)w.psum, tiles, g_poses);
    GS_LAUNCH_CHECK(TsdfStage(name, "finish").text);
    return GS_OK;
}

size_t gs_tsdf_raycast_backward_ws_bytes(int B, int nx, int ny, int nz, int has_color) {
    if (!tsdf_vol_ok(B, nx, ny, nz)) return 0;
    return tsdf_cast_bwd_layout(B, (int64_t)nx * ny * nz, has_color ? 4 : 1, false, 0, 0, nullptr, nullptr);
}

int gs_tsdf_raycast_backward(const float *tsdf, const float *weight, const float *color, int B, int nx, int ny, int nz, float voxel_size,
                             const float *origin, const float *intrinsics, const float *poses, int L, int height, int width, int stride,
                             float step, float min_weight, const int32_t *k_end, const float *g_depth, const float *g_rgb, float *g_tsdf,
                             float *g_color, void *ws, size_t ws_bytes, gs_stream_t stream) {
    GS_REQUIRE(tsdf && weight && origin && intrinsics && poses && k_end && g_tsdf, "gs_tsdf_raycast_backward: NULL argument");
    GS_REQUIRE((color != nullptr) == (g_color != nullptr) && (!g_rgb || color), "gs_tsdf_raycast_backward: color and g_color go together, g_rgb needs them");
    return tsdf_raycast_backward_run("gs_tsdf_raycast_backward", tsdf, weight, color, B, nx, ny, nz, voxel_size, origin, intrinsics, poses, L,
                                     height, width, stride, step, min_weight, k_end, g_depth, g_rgb, g_tsdf, g_color, nullptr, ws, ws_bytes,
                                     gs_tsdf_raycast_backward_ws_bytes(B, nx, ny, nz, color != nullptr), stream);
}

size_t gs_tsdf_raycast_backward_poses_ws_bytes(int B, int nx, int ny, int nz, int has_color, int L, int height, int width, int stride) {
    if (!tsdf_vol_ok(B, nx, ny, nz) || L <= 0 || L > 65535 || height <= 0 || width <= 0 || stride < 1) return 0;
    const int Ho = (int)(((int64_t)height + stride - 1) / stride), Wo = (int)(((int64_t)width + stride - 1) / stride);
    if ((int64_t)cdiv(Ho, 16) * cdiv(Wo, 16) > TSDF_CAST_TILES) return 0;
    return tsdf_cast_bwd_layout(B, (int64_t)nx * ny * nz, has_color ? 4 : 1, true, L, cdiv(Ho, 16) * cdiv(Wo, 16), nullptr, nullptr);
}

int gs_tsdf_raycast_backward_poses(const float *tsdf, const float *weight, const float *color, int B, int nx, int ny, int nz,
                                   float voxel_size, const float *origin, const float *intrinsics, const float *poses, int L, int height,
                                   int width, int stride, float step, float min_weight, const int32_t *k_end, const float *g_depth,
                                   const float *g_rgb, float *g_tsdf, float *g_color, float *g_poses, void *ws, size_t ws_bytes,
                                   gs_stream_t stream) {
    GS_REQUIRE(tsdf && weight && origin && intrinsics && poses && k_end && g_poses, "gs_tsdf_raycast_backward_poses: NULL argument");
    GS_REQUIRE((!g_color || (color && g_tsdf)) && (!g_rgb || color),
               "gs_tsdf_raycast_backward_poses: g_color needs color and g_tsdf, g_rgb needs color");
    return tsdf_raycast_backward_run("gs_tsdf_raycast_backward_poses", tsdf, weight, color, B, nx, ny, nz, voxel_size, origin, intrinsics,
                                     poses, L, height, width, stride, step, min_weight, k_end, g_depth, g_rgb, g_tsdf, g_color, g_poses, ws,
                                     ws_bytes, gs_tsdf_raycast_backward_poses_ws_bytes(B, nx, ny, nz, color != nullptr, L, height, width, stride),
                                     stream);
}

}  // extern "C"
