// libgradslam_hip -- map metrics (M): the two-sided nearest-neighbour statistics behind gs.metrics (chamfer distance,
// accuracy / completeness, precision / recall / F-score, Hausdorff distance) and their reverse pass.
//
// For a batch of cloud pairs a (B, Na_max, 3), b (B, Nb_max, 3) with device counts, gs_chamfer runs the exact 1-NN search of
// the ICP (knn_tile, gs_icp_assoc.hpp: bit-identical to brute force, the lowest index wins ties) in both directions and
// returns the packed keys of every row plus four sums per (batch element, direction), carried in fp64:
//   sum d2 | sum d (d = sqrt(d2), correctly rounded in fp32) | #(d2 < tau2) | max d2.
//
//   B  Bucketing (reorder != 0).  knn_tile prunes with the boxes of 16 CONSECUTIVE scan rows, which helps only when row
//      order is spatial order.  Each cloud is therefore scanned in the order of a uniform cell grid over its bounding box:
//        cham_bbox_k     bounding box of the valid rows (integer atomic max on order-preserving bit patterns: exact)
//        cham_hist_k     cell of every row (cham_grid: the rule), histogram
//        cham_scan_k     exclusive scan of the histogram, one block per (cloud, batch element)
//        cham_scatter_k  scan / scan_orig: rows in cell order (inside a cell in arrival order: the search's result does not
//                        depend on the scan order, its keys carry (distance bits, original row))
//      then cham_boxes_k boxes the scan order.  With reorder == 0 the boxes are built over the rows as they come and
//      scan == tgt, scan_orig == NULL: the path of gs_knn1.
//   D  cham_dir_k: one 64-row source tile per block (grid: tiles x batch x direction), knn_tile with a sampled seed, and an
//      epilogue that writes the keys and the block's partial sums.  cham_finish_k adds the partials in block order.  No
//      float atomics anywhere in the forward: the statistics are the same bits from run to run.
//   R  cham_bwd_k: the reverse pass (cham_contrib, gs_metrics.hpp), direct part stored, scattered part with float atomics;
//      the deterministic scatter lives in gs_metrics_det.hpp.
// Launch counts do not depend on the counts nor (the deterministic fold apart) on B; nothing synchronises the host.
#include <stddef.h>

#include "gs_cellgrid.hpp"
#include "gs_metrics.hpp"

namespace gs {

constexpr int CHAM_G_MAX = 64;  // cells per axis at most: 2^18 cells, a histogram one block scans in ~0.1 ms
constexpr int CHAM_PER_CELL = 16;  // = CHUNK: a surface sampled by n points fills ~g^2 cells of a g^3 grid
constexpr int CHAM_T = 256;
constexpr int CHAM_PART = 4;  // doubles per partial: sum d2, sum d, count, max d2

// cells along the longest axis of a cloud of n points: the smallest g with 16 g^2 >= n, at most CHAM_G_MAX
__host__ __device__ static inline int cham_g(int n) {
    int g = 1;
    while (g < CHAM_G_MAX && (int64_t)CHAM_PER_CELL * g * g < n) ++g;
    return g;
}
__host__ __device__ static inline int cham_nbox(int cap) { return (cap + CHUNK - 1) / CHUNK; }  // boxes per batch element
static inline int cham_cells_cap(int cap) { const int g = cham_g(cap); return g * g * g; }

// The cell grid of one cloud (gs_cellgrid.hpp) with chamfer's rule for the cells per axis, g = cham_g(n).
using ChamGrid = CellGrid;
__device__ __forceinline__ ChamGrid cham_grid(const uint32_t *__restrict__ acc /* max x y z | ~min x y z */, int n) {
    return cell_grid(acc, n, cham_g(n));
}
__device__ __forceinline__ int cham_cell(const ChamGrid &G, const f3 p) { return cell_of(G, p); }

// ------------------------------------------------------------------ workspace
struct ChamWs {
    float *scan[2];      // per side: (B, cap, 3) rows in cell order
    int32_t *orig[2];    // per side: (B, cap) original row of each scan slot
    int32_t *cell[2];    // per side: (B, cap) cell of each row
    float *boxes[2];     // per side: (B, ceil(cap / CHUNK), 6)
    uint32_t *bacc;      // (2, B, 8) bounding-box accumulators            } zeroed together
    int32_t *hist[2];    // per side: (B, cells_cap + 1)                   }
    double *part[2];     // per direction: (B, ceil(cap / 64), CHAM_PART)
    int hist_stride[2], nblk[2];
    size_t zero_bytes;
};
static size_t cham_layout(int B, int cap0, int cap1, void *ws, ChamWs *out) {
    Carve c{(char *)ws};
    ChamWs scratch, &r = out ? *out : scratch;
    const int cap[2] = {cap0, cap1};
    for (int s = 0; s < 2; ++s) {
        r.scan[s] = c.take<float>((size_t)B * cap[s] * 12);
        r.orig[s] = c.take<int32_t>((size_t)B * cap[s] * 4);
        r.cell[s] = c.take<int32_t>((size_t)B * cap[s] * 4);
        r.boxes[s] = c.take<float>((size_t)B * cham_nbox(cap[s]) * 6 * 4);
    }
    const size_t z0 = c.off;
    r.bacc = c.take<uint32_t>((size_t)2 * B * 8 * 4);
    for (int s = 0; s < 2; ++s) {
        r.hist_stride[s] = cham_cells_cap(cap[s]) + 1;
        r.hist[s] = c.take<int32_t>((size_t)B * r.hist_stride[s] * 4);
    }
    r.zero_bytes = c.off - z0;
    for (int d = 0; d < 2; ++d) {
        r.nblk[d] = cdiv(cap[d], 64);
        r.part[d] = c.take<double>((size_t)B * r.nblk[d] * CHAM_PART * 8);
    }
    return c.off;
}

// ------------------------------------------------------------------ B: bucketing.  grid (x: rows, y: batch element, z: side)
__global__ __launch_bounds__(CHAM_T) void cham_bbox_k(ChamIn in, uint32_t *__restrict__ bacc) {
    const int s = blockIdx.z, b = blockIdx.y, n = cham_count(in, s, b);
    if ((int)(blockIdx.x * CHAM_T) >= n) return;
    cell_bbox(in.pts[s] + (int64_t)b * in.cap[s] * 3, n, [&] { return bacc + ((int64_t)s * gridDim.y + b) * 8; }, CHAM_T);
}

__global__ __launch_bounds__(CHAM_T) void cham_hist_k(ChamIn in, ChamWs w) {
    const int s = blockIdx.z, b = blockIdx.y, n = cham_count(in, s, b);
    if ((int)(blockIdx.x * CHAM_T) >= n) return;
    const ChamGrid G = cham_grid(w.bacc + ((int64_t)s * gridDim.y + b) * 8, n);
    const float *pts = in.pts[s] + (int64_t)b * in.cap[s] * 3;
    int32_t *cell = w.cell[s] + (int64_t)b * in.cap[s];
    int32_t *hist = w.hist[s] + (int64_t)b * w.hist_stride[s];
    for (int i = blockIdx.x * CHAM_T + threadIdx.x; i < n; i += gridDim.x * CHAM_T) {
        const int c = cham_cell(G, ld3(pts, i));
        cell[i] = c;
        atomicAdd(hist + c, 1);
    }
}

// grid (x: batch element, y: side), 1024 threads: every wave scans one contiguous stretch of the cells, 64 at a time
__global__ __launch_bounds__(1024) void cham_scan_k(ChamIn in, ChamWs w) {
    __shared__ int wtot[16];
    const int s = blockIdx.y, b = blockIdx.x, n = cham_count(in, s, b);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ncells = min(cham_grid(w.bacc + ((int64_t)s * gridDim.x + b) * 8, n).ncells, w.hist_stride[s] - 1);
    cell_hist_scan(w.hist[s] + (int64_t)b * w.hist_stride[s], ncells, wtot, lane, wave);
}

__global__ __launch_bounds__(CHAM_T) void cham_scatter_k(ChamIn in, ChamWs w) {
    const int s = blockIdx.z, b = blockIdx.y, n = cham_count(in, s, b);
    if ((int)(blockIdx.x * CHAM_T) >= n) return;
    const float *pts = in.pts[s] + (int64_t)b * in.cap[s] * 3;
    const int32_t *cell = w.cell[s] + (int64_t)b * in.cap[s];
    int32_t *hist = w.hist[s] + (int64_t)b * w.hist_stride[s];
    float *scan = w.scan[s] + (int64_t)b * in.cap[s] * 3;
    int32_t *orig = w.orig[s] + (int64_t)b * in.cap[s];
    for (int i = blockIdx.x * CHAM_T + threadIdx.x; i < n; i += gridDim.x * CHAM_T) {
        const int slot = atomicAdd(hist + cell[i], 1);  // the cell's cursor: starts at the cell's first slot
        if ((unsigned)slot >= (unsigned)n) continue;    // (cannot happen: the cursors partition [0, n))
        st3(scan, slot, ld3(pts, i));
        orig[slot] = i;
    }
}

// boxes of CHUNK consecutive scan rows (tgt_boxes_k, batched): one wave covers 64 rows
__global__ __launch_bounds__(64) void cham_boxes_k(ChamIn in, ChamWs w, int reorder) {
    const int s = blockIdx.z, b = blockIdx.y, n = cham_count(in, s, b);
    const int j = blockIdx.x * 64 + threadIdx.x;
    if ((int)(blockIdx.x * 64) >= n) return;
    const float *pts = reorder ? w.scan[s] + (int64_t)b * in.cap[s] * 3 : in.pts[s] + (int64_t)b * in.cap[s] * 3;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (j < n) {
        const f3 p = ld3(pts, j);
        lo[0] = hi[0] = p.x; lo[1] = hi[1] = p.y; lo[2] = hi[2] = p.z;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int off = CHUNK / 2; off > 0; off >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], off, kWave));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off, kWave));
        }
    }
    if ((threadIdx.x % CHUNK) == 0 && j < n) {
        float *bx = w.boxes[s] + ((int64_t)b * cham_nbox(in.cap[s]) + j / CHUNK) * 6;
        bx[0] = lo[0]; bx[1] = lo[1]; bx[2] = lo[2]; bx[3] = hi[0]; bx[4] = hi[1]; bx[5] = hi[2];
    }
}

// ------------------------------------------------------------------ D: search + statistics.  grid (x: tiles, y: batch, z: direction)
__global__ __launch_bounds__(KNN_BT) void cham_dir_k(ChamIn in, ChamWs w, int reorder, float tau2,
                                                     unsigned long long *__restrict__ keys_ab,
                                                     unsigned long long *__restrict__ keys_ba) {
    __shared__ KnnShared sh;
    const int d = blockIdx.z, t = 1 - d, b = blockIdx.y;
    const int ns = cham_count(in, d, b), nt = cham_count(in, t, b);
    const int tile0 = blockIdx.x * 64;
    if (tile0 >= ns) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = tile0 + lane;
    const bool ok = i < ns;
    const float *src = in.pts[d] + (int64_t)b * in.cap[d] * 3;
    const float *tgt = in.pts[t] + (int64_t)b * in.cap[t] * 3;
    const f3 s = ok ? ld3(src, i) : f3{0.0f, 0.0f, 0.0f};
    unsigned long long key = KEY_NONE;
    if (nt > 0) {  // block-uniform
        const float *scan = reorder ? w.scan[t] + (int64_t)b * in.cap[t] * 3 : tgt;
        const int32_t *orig = reorder ? w.orig[t] + (int64_t)b * in.cap[t] : nullptr;
        const float *boxes = w.boxes[t] + (int64_t)b * cham_nbox(in.cap[t]) * 6;
        key = knn_tile<KNN_NW>(sh, s, ok, -1, tgt, scan, orig, boxes, nullptr, nt);
    }
    if (wave != 0) return;
    if (ok) (d ? keys_ba : keys_ab)[(int64_t)b * in.cap[d] + i] = key;
    const bool have = ok && key != KEY_NONE;
    const float d2 = have ? bitsf((uint32_t)(key >> 32)) : 0.0f;
    double s2 = (double)d2, s1 = (double)sqrtf(d2);  // correctly rounded (-fno-fast-math); __fsqrt_rn is the native 1-ulp instruction here
    int cnt = (have && d2 < tau2) ? 1 : 0;
    float mx = d2;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s2 += __shfl_xor(s2, off, kWave);
        s1 += __shfl_xor(s1, off, kWave);
        cnt += __shfl_xor(cnt, off, kWave);
        mx = fmaxf(mx, __shfl_xor(mx, off, kWave));
    }
    if (lane == 0) {
        double *p = w.part[d] + ((int64_t)b * w.nblk[d] + blockIdx.x) * CHAM_PART;
        p[0] = s2; p[1] = s1; p[2] = (double)cnt; p[3] = (double)mx;
    }
}

// grid (x: batch element, y: direction): the partials of the blocks that ran, added in block order
__global__ __launch_bounds__(CHAM_T) void cham_finish_k(ChamIn in, ChamWs w, double *__restrict__ stats) {
    __shared__ double red[CHAM_T][CHAM_PART];
    const int d = blockIdx.y, b = blockIdx.x;
    const int nb = (cham_count(in, d, b) + 63) / 64;
    const double *p = w.part[d] + (int64_t)b * w.nblk[d] * CHAM_PART;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int k = threadIdx.x; k < nb; k += CHAM_T) {
        a0 += p[CHAM_PART * k]; a1 += p[CHAM_PART * k + 1]; a2 += p[CHAM_PART * k + 2];
        a3 = fmax(a3, p[CHAM_PART * k + 3]);
    }
    red[threadIdx.x][0] = a0; red[threadIdx.x][1] = a1; red[threadIdx.x][2] = a2; red[threadIdx.x][3] = a3;
    __syncthreads();
    for (int h = CHAM_T / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            red[threadIdx.x][0] += red[threadIdx.x + h][0];
            red[threadIdx.x][1] += red[threadIdx.x + h][1];
            red[threadIdx.x][2] += red[threadIdx.x + h][2];
            red[threadIdx.x][3] = fmax(red[threadIdx.x][3], red[threadIdx.x + h][3]);
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < CHAM_PART) stats[((int64_t)b * 2 + d) * CHAM_PART + threadIdx.x] = red[0][threadIdx.x];
}

// ------------------------------------------------------------------ R: reverse pass.  grid (x: source rows, y: batch, z: direction)
// MODE 0: g_src[i] = v (zeros without a neighbour)   1: g_tgt[j] -= v with float atomics   2: g_src[i] += v
template <int MODE>
__global__ __launch_bounds__(CHAM_T) void cham_bwd_k(ChamIn in, const unsigned long long *__restrict__ keys_ab,
                                                     const unsigned long long *__restrict__ keys_ba, const float *__restrict__ g2,
                                                     const float *__restrict__ g1, float *__restrict__ g_a, float *__restrict__ g_b) {
    const int d = blockIdx.z, b = blockIdx.y;
    const int ns = cham_count(in, d, b);
    const unsigned long long *keys = d ? keys_ba : keys_ab;
    float *g_src = (d ? g_b : g_a) + (int64_t)b * in.cap[d] * 3;
    float *g_tgt = (d ? g_a : g_b) + (int64_t)b * in.cap[1 - d] * 3;
    for (int i = blockIdx.x * CHAM_T + threadIdx.x; i < ns; i += gridDim.x * CHAM_T) {
        f3 v;
        int j;
        const bool have = cham_contrib(in, keys, g2, g1, d, b, i, v, j);
        if (MODE == 0) st3(g_src, i, v);
        if (MODE == 1 && have) {
            atomicAdd(g_tgt + 3 * (int64_t)j, -v.x);
            atomicAdd(g_tgt + 3 * (int64_t)j + 1, -v.y);
            atomicAdd(g_tgt + 3 * (int64_t)j + 2, -v.z);
        }
        if (MODE == 2 && have) {
            const f3 g = ld3(g_src, i);
            st3(g_src, i, f3{g.x + v.x, g.y + v.y, g.z + v.z});
        }
    }
}

static inline bool cham_shape_ok(int B, int cap0, int cap1) { return B > 0 && B <= 65535 && cap0 > 0 && cap1 > 0; }

}  // namespace gs

using namespace gs;

extern "C" {

size_t gs_chamfer_ws_bytes(int B, int Na_max, int Nb_max) {
    if (B <= 0 || Na_max <= 0 || Nb_max <= 0) return 0;
    return cham_layout(B, Na_max, Nb_max, nullptr, nullptr);
}

int gs_chamfer(const float *a, const int32_t *a_counts, int Na_max, const float *b, const int32_t *b_counts, int Nb_max, int B,
               float tau2, int reorder, double *stats, uint64_t *keys_ab, uint64_t *keys_ba, void *ws, size_t ws_bytes,
               gs_stream_t stream) {
    GS_REQUIRE(a && a_counts && b && b_counts && stats && keys_ab && keys_ba, "gs_chamfer: NULL argument");
    GS_REQUIRE(cham_shape_ok(B, Na_max, Nb_max), "gs_chamfer: bad shape B=%d Na_max=%d Nb_max=%d", B, Na_max, Nb_max);
    GS_REQUIRE_WS("gs_chamfer", ws, ws_bytes, gs_chamfer_ws_bytes(B, Na_max, Nb_max));
    hipStream_t st = (hipStream_t)stream;
    ChamWs w;
    cham_layout(B, Na_max, Nb_max, ws, &w);
    const ChamIn in{{a, b}, {a_counts, b_counts}, {Na_max, Nb_max}};
    const int capm = std::max(Na_max, Nb_max);
    if (reorder) {
        const dim3 rows(std::min(cdiv(capm, CHAM_T), 1024), B, 2);
        GS_HIP(hipMemsetAsync(w.bacc, 0, w.zero_bytes, st), "gs_chamfer/zero");
        hipLaunchKernelGGL(cham_bbox_k, rows, dim3(CHAM_T), 0, st, in, w.bacc);
        hipLaunchKernelGGL(cham_hist_k, rows, dim3(CHAM_T), 0, st, in, w);
        hipLaunchKernelGGL(cham_scan_k, dim3(B, 2), dim3(1024), 0, st, in, w);
        hipLaunchKernelGGL(cham_scatter_k, rows, dim3(CHAM_T), 0, st, in, w);
        GS_LAUNCH_CHECK("gs_chamfer/bucket");
    }
    hipLaunchKernelGGL(cham_boxes_k, dim3(cdiv(capm, 64), B, 2), dim3(64), 0, st, in, w, reorder);
    GS_LAUNCH_CHECK("gs_chamfer/boxes");
    hipLaunchKernelGGL(cham_dir_k, dim3(cdiv(capm, 64), B, 2), dim3(KNN_BT), 0, st, in, w, reorder, tau2, (unsigned long long *)keys_ab,
                       (unsigned long long *)keys_ba);
    GS_LAUNCH_CHECK("gs_chamfer/search");
    hipLaunchKernelGGL(cham_finish_k, dim3(B, 2), dim3(CHAM_T), 0, st, in, w, stats);
    GS_LAUNCH_CHECK("gs_chamfer/finish");
    return GS_OK;
}

size_t gs_chamfer_backward_det_ws_bytes(int B, int Na_max, int Nb_max) {
    if (B <= 0 || Na_max <= 0 || Nb_max <= 0) return 0;
    return chamfer_det_ws_bytes(B, Na_max, Nb_max);
}

static int chamfer_backward_entry(const char *name, bool det, const float *a, const int32_t *a_counts, int Na_max, const float *b,
                                  const int32_t *b_counts, int Nb_max, int B, const uint64_t *keys_ab, const uint64_t *keys_ba,
                                  const float *g2, const float *g1, float *g_a, float *g_b, void *ws, size_t ws_bytes,
                                  gs_stream_t stream) {
    GS_REQUIRE(a && a_counts && b && b_counts && keys_ab && keys_ba && g2 && g1 && g_a && g_b, "%s: NULL argument", name);
    GS_REQUIRE(cham_shape_ok(B, Na_max, Nb_max), "%s: bad shape B=%d Na_max=%d Nb_max=%d", name, B, Na_max, Nb_max);
    if (det) GS_REQUIRE_WS(name, ws, ws_bytes, gs_chamfer_backward_det_ws_bytes(B, Na_max, Nb_max));
    hipStream_t st = (hipStream_t)stream;
    const ChamIn in{{a, b}, {a_counts, b_counts}, {Na_max, Nb_max}};
    const unsigned long long *kab = (const unsigned long long *)keys_ab, *kba = (const unsigned long long *)keys_ba;
    const dim3 grid(rows_grid(std::max(Na_max, Nb_max), CHAM_T, 2048), B, 2);
    if (det) {  // the fold overwrites the rows below the counts with the scattered part; the direct part is added to it
        const int rc = chamfer_det_scatter(in, B, kab, kba, g2, g1, g_a, g_b, ws, st, name);
        if (rc != GS_OK) return rc;
        hipLaunchKernelGGL(cham_bwd_k<2>, grid, dim3(CHAM_T), 0, st, in, kab, kba, g2, g1, g_a, g_b);
    } else {
        hipLaunchKernelGGL(cham_bwd_k<0>, grid, dim3(CHAM_T), 0, st, in, kab, kba, g2, g1, g_a, g_b);
        hipLaunchKernelGGL(cham_bwd_k<1>, grid, dim3(CHAM_T), 0, st, in, kab, kba, g2, g1, g_a, g_b);
    }
    GS_LAUNCH_CHECK(name);
    return GS_OK;
}

size_t gs_chamfer_backward_ws_bytes(int B, int Na_max, int Nb_max) {
    (void)B; (void)Na_max; (void)Nb_max;
    return 0;
}

int gs_chamfer_backward(const float *a, const int32_t *a_counts, int Na_max, const float *b, const int32_t *b_counts, int Nb_max,
                        int B, const uint64_t *keys_ab, const uint64_t *keys_ba, const float *g2, const float *g1, float *g_a,
                        float *g_b, void *ws, size_t ws_bytes, gs_stream_t stream) {
    return chamfer_backward_entry("gs_chamfer_backward", false, a, a_counts, Na_max, b, b_counts, Nb_max, B, keys_ab, keys_ba, g2, g1,
                                  g_a, g_b, ws, ws_bytes, stream);
}

int gs_chamfer_backward_det(const float *a, const int32_t *a_counts, int Na_max, const float *b, const int32_t *b_counts, int Nb_max,
                            int B, const uint64_t *keys_ab, const uint64_t *keys_ba, const float *g2, const float *g1, float *g_a,
                            float *g_b, void *ws, size_t ws_bytes, gs_stream_t stream) {
    return chamfer_backward_entry("gs_chamfer_backward_det", true, a, a_counts, Na_max, b, b_counts, Nb_max, B, keys_ab, keys_ba, g2,
                                  g1, g_a, g_b, ws, ws_bytes, stream);
}

}  // extern "C"
