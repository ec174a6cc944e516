// libgradslam_hip -- neighbours (N): the exact K nearest neighbours of every row of a cloud in another (or the same) cloud, the
// adjoint of their distances, and normals from the neighbourhoods' covariances.
//
// gs_knn: for source row i < src_counts[b], slot k holds the k-th smallest of {(d2(i, j), j) : j < tgt_counts[b]} in
// lexicographic order, packed with pack_key; d2 = dist2 of gs_icp_assoc.hpp (the bits of gs_knn1).  Everything else KEY_NONE.
//
//   B  Bucketing.  ONE grid per batch element, over the TARGETS' bounding box (gs_cellgrid.hpp, g = nb_g: the rule); both
//      clouds are bucketed in it (a source outside the box clamps to a border cell: only the order of the work depends on it).
//        nb_bbox_k     bounding box of the targets (integer atomic max on order-preserving bit patterns: exact)
//        nb_hist_k     cell of every row, histogram per side; for the targets also, per axis and cell layer, the smallest and
//                      largest coordinate in the layer (integer atomic max on ord_bits / ~ord_bits: exact)
//        nb_scan_k     exclusive scan of both histograms; suffix-min / prefix-max of the layers' extremes (nb "faces")
//        nb_scatter_k  targets in cell order as (x, y, z, original row) in one 16-byte word; sources: the row of every slot
//   S  nb_search_k: one thread per query, queries in the SOURCES' cell order.  The running top K lives in LDS as sorted packed
//      keys; a candidate is inserted only when its key is below the current K-th.  The examined region is a box of cells
//      around the query's cell.  After examining every target in the box, each face with targets beyond it bounds every
//      unexamined target from below: gap = fl(c - q_a) with c the smallest coordinate beyond (fl(q_a - c), c the largest, on the
//      low side); bound = fl(gap * gap) if gap > 0 else 0.  Rounding is monotone and the other two squares are >= 0, so
//      bound <= d2 holds exactly: no epsilon.  The search stops when it holds K keys and the K-th d2 is STRICTLY below every
//      face's bound (a target at equal distance may have a lower row), or when no face has a target beyond it.  Otherwise the
//      faces whose bound is not above the K-th distance grow by one layer and only the new cells are examined.
//      The result is a property of the key set alone: it does not depend on g, on either cloud's row order or on arrival order.
//   R  gs_knn_backward: g_src in fp32 in slot order; g_tgt by the exact fold of gs_fixed128.hpp (the rule is stated there).
//   E  gs_knn_normals: fp64 covariance of the neighbours, cyclic Jacobi, the eigenvector of the smallest eigenvalue.
// No float atomic, no allocation, no host synchronisation; launch counts do not depend on the counts, B or K.
#include <stddef.h>

#include <algorithm>

#include "gs_cellgrid.hpp"
#include "gs_fixed128.hpp"
#include "gs_icp_assoc.hpp"

namespace gs {

constexpr int NB_G_MAX = 128;  // cells per axis at most: 2^21 cells, a histogram one block scans in under a millisecond
constexpr int NB_T = 256;
constexpr int NB_KMAX = 32;
constexpr int NB_FACE = NB_G_MAX + 1;  // entries per axis of a face table
constexpr int NB_SWEEPS = 8;           // cyclic Jacobi sweeps of a 3x3 in fp64: convergence is quadratic, 4-5 suffice

static int g_knn_grid_cap = 0;  // gs_set_knn_grid: 0 = the rule, otherwise the cells per axis are capped (test knob)

// K is bucketed for the LDS of the search and for the grid rule
__host__ __device__ static inline int nb_kbucket(int K) { return K <= 8 ? 8 : (K <= 16 ? 16 : 32); }

// THE RULE.  Cells along the longest axis for n targets: the smallest g with kbucket(K) g^2 >= n, at most NB_G_MAX (and at
// most g_cap when that is set).  A surface sampled by n points fills about 2 g^2 cells of the g^3, so an occupied cell holds
// about K / 2 targets and the first ring (up to 9 occupied cells) a few K: the search rarely needs a second ring.
// No result depends on it.
__host__ __device__ static inline int nb_g(int n, int K, int g_cap) {
    const int per = nb_kbucket(K), gm = (g_cap > 0 && g_cap < NB_G_MAX) ? g_cap : NB_G_MAX;
    int g = 1;
    while (g < gm && (int64_t)per * g * g < n) ++g;
    return g;
}
static inline int nb_cells_cap(int cap, int K) { const int g = nb_g(cap, K, 0); return g * g * g; }

struct NbIn {
    const float *pts[2];    // side 0 = sources (B, cap[0], 3), side 1 = targets (B, cap[1], 3)
    const int32_t *cnt[2];  // (B,) device counts
    int cap[2];
    int K, g_cap;
};
__device__ __forceinline__ int nb_count(const NbIn &in, int side, int b) { return min(max(in.cnt[side][b], 0), in.cap[side]); }
__device__ __forceinline__ CellGrid nb_grid(const NbIn &in, const uint32_t *__restrict__ bacc, int b) {
    const int nt = nb_count(in, 1, b);
    return cell_grid(bacc + (int64_t)b * 8, nt, nb_g(nt, in.K, in.g_cap));
}

// ------------------------------------------------------------------ workspace of gs_knn
struct NbWs {
    float4 *scan;      // (B, cap1) targets in cell order: x, y, z, bits of the original row
    int32_t *orig0;    // (B, cap0) the source row of every slot of the sources' cell order
    int32_t *cell[2];  // per side: (B, cap) cell of each row
    float *face;       // (B, 2, 3, NB_FACE): [0] suffix-min over layers >= L at [L]; [1] prefix-max over layers <= L at [L + 1]
    uint32_t *bacc;    // (B, 8) bounding-box accumulators                                        } zeroed together
    uint32_t *lay;     // (B, 2, 3, NB_G_MAX): [0] ~ord_bits(min), [1] ord_bits(max); 0 = empty   }
    int32_t *hist[2];  // per side: (B, hist_stride)                                              }
    int hist_stride;
    size_t zero_bytes;
};
static size_t nb_layout(int B, int cap0, int cap1, int K, void *ws, NbWs *out) {
    Carve c{(char *)ws};
    NbWs scratch, &r = out ? *out : scratch;
    r.scan = c.take<float4>((size_t)B * cap1 * 16);
    r.orig0 = c.take<int32_t>((size_t)B * cap0 * 4);
    r.cell[0] = c.take<int32_t>((size_t)B * cap0 * 4);
    r.cell[1] = c.take<int32_t>((size_t)B * cap1 * 4);
    r.face = c.take<float>((size_t)B * 2 * 3 * NB_FACE * 4);
    const size_t z0 = c.off;
    r.bacc = c.take<uint32_t>((size_t)B * 8 * 4);
    r.lay = c.take<uint32_t>((size_t)B * 2 * 3 * NB_G_MAX * 4);
    r.hist_stride = nb_cells_cap(cap1, K);
    for (int s = 0; s < 2; ++s) r.hist[s] = c.take<int32_t>((size_t)B * r.hist_stride * 4);
    r.zero_bytes = c.off - z0;
    return c.off;
}

// ------------------------------------------------------------------ B: bucketing
// grid (x: rows, y: batch element): the targets' bounding box
__global__ __launch_bounds__(NB_T) void nb_bbox_k(NbIn in, uint32_t *__restrict__ bacc) {
    const int b = blockIdx.y, n = nb_count(in, 1, b);
    if ((int)(blockIdx.x * NB_T) >= n) return;
    cell_bbox(in.pts[1] + (int64_t)b * in.cap[1] * 3, n, [&] { return bacc + (int64_t)b * 8; }, NB_T);
}

// an integer atomic maximum that most callers skip: the plain read may be stale, which only costs an atomic
__device__ __forceinline__ void nb_raise(uint32_t *p, uint32_t v) {
    if (v > *(volatile uint32_t *)p) atomicMax(p, v);
}

// grid (x: rows, y: batch element, z: side)
__global__ __launch_bounds__(NB_T) void nb_hist_k(NbIn in, NbWs w) {
    const int s = blockIdx.z, b = blockIdx.y, n = nb_count(in, s, b);
    if ((int)(blockIdx.x * NB_T) >= n) return;
    const CellGrid G = nb_grid(in, w.bacc, b);
    const float *pts = in.pts[s] + (int64_t)b * in.cap[s] * 3;
    int32_t *cell = w.cell[s] + (int64_t)b * in.cap[s];
    int32_t *hist = w.hist[s] + (int64_t)b * w.hist_stride;
    uint32_t *lay = w.lay + (int64_t)b * 2 * 3 * NB_G_MAX;
    for (int i = blockIdx.x * NB_T + threadIdx.x; i < n; i += gridDim.x * NB_T) {
        const f3 p = ld3(pts, i);
        int cx, cy, cz;
        cell_xyz(G, p, cx, cy, cz);
        const int c = min((cz * G.g[1] + cy) * G.g[0] + cx, w.hist_stride - 1);  // (< ncells <= hist_stride: nb_g is monotone in n)
        cell[i] = c;
        atomicAdd(hist + c, 1);
        if (s == 1) {  // cx, cy, cz < g <= NB_G_MAX
            const uint32_t ox = ord_bits(p.x), oy = ord_bits(p.y), oz = ord_bits(p.z);
            nb_raise(lay + 0 * NB_G_MAX + cx, ~ox); nb_raise(lay + 3 * NB_G_MAX + cx, ox);
            nb_raise(lay + 1 * NB_G_MAX + cy, ~oy); nb_raise(lay + 4 * NB_G_MAX + cy, oy);
            nb_raise(lay + 2 * NB_G_MAX + cz, ~oz); nb_raise(lay + 5 * NB_G_MAX + cz, oz);
        }
    }
}

// grid (x: batch element, y: side), 1024 threads: every wave scans one contiguous stretch of the cells, 64 at a time.  The
// block of side 1 also turns the layers' extremes into the face tables (three threads, one per axis, g <= 128 steps each).
__global__ __launch_bounds__(1024) void nb_scan_k(NbIn in, NbWs w) {
    __shared__ int wtot[16];
    const int s = blockIdx.y, b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const CellGrid G = nb_grid(in, w.bacc, b);
    if (s == 1 && threadIdx.x < 3) {
        const int a = threadIdx.x, ga = min(a == 0 ? G.g[0] : (a == 1 ? G.g[1] : G.g[2]), NB_G_MAX);
        const uint32_t *lmin = w.lay + ((int64_t)b * 2 * 3 + a) * NB_G_MAX, *lmax = lmin + 3 * NB_G_MAX;
        float *suf = w.face + ((int64_t)b * 2 * 3 + a) * NB_FACE, *pre = suf + 3 * NB_FACE;
        float run = INFINITY;
        suf[ga] = run;
        for (int L = ga - 1; L >= 0; --L) {
            if (lmin[L]) run = fminf(run, ord_float(~lmin[L]));
            suf[L] = run;
        }
        run = -INFINITY;
        pre[0] = run;
        for (int L = 0; L < ga; ++L) {
            if (lmax[L]) run = fmaxf(run, ord_float(lmax[L]));
            pre[L + 1] = run;
        }
    }
    const int ncells = min(G.ncells, w.hist_stride);
    cell_hist_scan(w.hist[s] + (int64_t)b * w.hist_stride, ncells, wtot, lane, wave);
}

// grid (x: rows, y: batch element, z: side).  Every cell's cursor starts at the cell's first slot and ends at its end, which
// is what the search reads: cell c holds the slots [c ? hist[c - 1] : 0, hist[c]).  Inside a cell the rows stand in arrival
// order: the search's result does not depend on it, its keys carry (distance bits, original row).
__global__ __launch_bounds__(NB_T) void nb_scatter_k(NbIn in, NbWs w) {
    const int s = blockIdx.z, b = blockIdx.y, n = nb_count(in, s, b);
    if ((int)(blockIdx.x * NB_T) >= n) return;
    const float *pts = in.pts[s] + (int64_t)b * in.cap[s] * 3;
    const int32_t *cell = w.cell[s] + (int64_t)b * in.cap[s];
    int32_t *hist = w.hist[s] + (int64_t)b * w.hist_stride;
    for (int i = blockIdx.x * NB_T + threadIdx.x; i < n; i += gridDim.x * NB_T) {
        const int slot = atomicAdd(hist + cell[i], 1);
        if ((unsigned)slot >= (unsigned)n) continue;  // (cannot happen: the cursors partition [0, n))
        if (s == 1) {
            const f3 p = ld3(pts, i);
            w.scan[(int64_t)b * in.cap[1] + slot] = make_float4(p.x, p.y, p.z, __int_as_float(i));
        } else {
            w.orig0[(int64_t)b * in.cap[0] + slot] = i;
        }
    }
}

// ------------------------------------------------------------------ S: search.  grid (x: query slots, y: batch element)
__device__ __forceinline__ float nb_bound(float gap) { return gap > 0.0f ? gap * gap : 0.0f; }
__device__ __forceinline__ int nb_sel(int a, int x, int y, int z) { return a == 0 ? x : (a == 1 ? y : z); }

// every target of the cells [x0, x1] x [y0, y1] x [z0, z1]: cells consecutive in x are consecutive slots, one range per (y, z)
__device__ __forceinline__ void nb_examine(const float4 *__restrict__ scan, const int32_t *__restrict__ hist, int nt, int gx, int gy,
                                           int x0, int x1, int y0, int y1, int z0, int z1, const f3 s, int K,
                                           unsigned long long *top /* this thread's column: stride NB_T */, unsigned long long &kth) {
    for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y) {
            const int c0 = (z * gy + y) * gx + x0, c1 = c0 + (x1 - x0);
            const int j0 = c0 > 0 ? max(hist[c0 - 1], 0) : 0, j1 = min(hist[c1], nt);
            for (int j = j0; j < j1; ++j) {
                const float4 t = scan[j];
                const unsigned long long key = pack_key(dist2(s, t.x, t.y, t.z), __float_as_int(t.w));
                if (key >= kth) continue;
                int p = K - 1;
                while (p > 0) {
                    const unsigned long long prev = top[(p - 1) * NB_T];
                    if (prev <= key) break;
                    top[p * NB_T] = prev;
                    --p;
                }
                top[p * NB_T] = key;
                kth = top[(K - 1) * NB_T];
            }
        }
}

template <int KB>
__global__ __launch_bounds__(NB_T) void nb_search_k(NbIn in, NbWs w, unsigned long long *__restrict__ keys) {
    __shared__ unsigned long long top_s[KB * NB_T];
    __shared__ float suf_s[3][NB_FACE], pre_s[3][NB_FACE];
    const int b = blockIdx.y, K = in.K;
    const int ns = nb_count(in, 0, b), nt = nb_count(in, 1, b);
    const CellGrid G = nb_grid(in, w.bacc, b);
    const int gx = G.g[0], gy = G.g[1], gz = G.g[2];
    {
        const float *face = w.face + (int64_t)b * 2 * 3 * NB_FACE;
        for (int t = threadIdx.x; t < 3 * NB_FACE; t += NB_T) {
            const int a = t / NB_FACE, L = t - a * NB_FACE;
            const bool in_grid = L <= nb_sel(a, gx, gy, gz);  // nb_scan_k wrote [0, g_a]
            suf_s[a][L] = in_grid ? face[t] : INFINITY;
            pre_s[a][L] = in_grid ? face[3 * NB_FACE + t] : -INFINITY;
        }
    }
    __syncthreads();
    const int q = blockIdx.x * NB_T + threadIdx.x;
    if (q >= in.cap[0]) return;
    if (q >= ns) {  // the slots [0, ns) are a permutation of the rows [0, ns): row q >= ns is nobody's
        unsigned long long *o = keys + ((int64_t)b * in.cap[0] + q) * K;
        for (int k = 0; k < K; ++k) o[k] = KEY_NONE;
        return;
    }
    const int i = min(max(w.orig0[(int64_t)b * in.cap[0] + q], 0), ns - 1);
    const f3 s = ld3(in.pts[0], (int64_t)b * in.cap[0] + i);
    unsigned long long *top = top_s + threadIdx.x;
    for (int k = 0; k < K; ++k) top[k * NB_T] = KEY_NONE;
    unsigned long long kth = KEY_NONE;  // the K-th key; KEY_NONE until K keys are held
    const float4 *scan = w.scan + (int64_t)b * in.cap[1];
    const int32_t *hist = w.hist[1] + (int64_t)b * w.hist_stride;

    int lx, ly, lz;
    cell_xyz(G, s, lx, ly, lz);
    int hx = lx, hy = ly, hz = lz;
    nb_examine(scan, hist, nt, gx, gy, lx, hx, ly, hy, lz, hz, s, K, top, kth);
    for (;;) {
        // the faces' bounds: [2a] low side of axis a, [2a + 1] high side; +inf where no target lies beyond the face
        float bnd[6];
        bnd[0] = lx > 0 ? nb_bound(s.x - pre_s[0][lx]) : INFINITY;
        bnd[1] = hx < gx - 1 ? nb_bound(suf_s[0][hx + 1] - s.x) : INFINITY;
        bnd[2] = ly > 0 ? nb_bound(s.y - pre_s[1][ly]) : INFINITY;
        bnd[3] = hy < gy - 1 ? nb_bound(suf_s[1][hy + 1] - s.y) : INFINITY;
        bnd[4] = lz > 0 ? nb_bound(s.z - pre_s[2][lz]) : INFINITY;
        bnd[5] = hz < gz - 1 ? nb_bound(suf_s[2][hz + 1] - s.z) : INFINITY;
        const float minb = fminf(fminf(fminf(bnd[0], bnd[1]), fminf(bnd[2], bnd[3])), fminf(bnd[4], bnd[5]));
        if (!(minb < INFINITY)) break;  // nothing beyond any face
        const bool full = kth != KEY_NONE;
        const float d2k = bitsf((uint32_t)(kth >> 32));
        if (full && d2k < minb) break;
        // grow, one face after the other (each slab spans the box as grown so far, so corners are covered once)
#pragma unroll
        for (int f = 0; f < 6; ++f) {
            if (!(bnd[f] < INFINITY) || (full && d2k < bnd[f])) continue;  // (the face of minb always grows: progress)
            int x0 = lx, x1 = hx, y0 = ly, y1 = hy, z0 = lz, z1 = hz;
            if (f == 0) x0 = x1 = --lx;
            if (f == 1) x0 = x1 = ++hx;
            if (f == 2) y0 = y1 = --ly;
            if (f == 3) y0 = y1 = ++hy;
            if (f == 4) z0 = z1 = --lz;
            if (f == 5) z0 = z1 = ++hz;
            nb_examine(scan, hist, nt, gx, gy, x0, x1, y0, y1, z0, z1, s, K, top, kth);
        }
    }
    unsigned long long *o = keys + ((int64_t)b * in.cap[0] + i) * K;
    for (int k = 0; k < K; ++k) o[k] = top[k * NB_T];
}

// ------------------------------------------------------------------ R: reverse pass
struct NbBwd {
    NbIn in;
    const unsigned long long *keys;  // (B, cap0, K)
    const float *g_d2;               // (B, cap0, K)
    float *g_src, *g_tgt;            // (B, cap0, 3), (B, cap1, 3)
    Fold fold;                       // (B cap1) x 3: the sums of g_tgt (gs_fixed128.hpp), zeroed as one piece
    int lg;
};
static size_t nb_bwd_layout(int B, int cap1, void *ws, NbBwd *out) {
    Carve c{(char *)ws};
    const Fold f = fold_carve(c, (size_t)B * cap1, 3, true);  // sums | flags | maximum
    if (out) out->fold = f;
    return c.off;
}

// The term of slot (i, k): with j its neighbour, c = 2 g_d2[i, k], delta = s_i - t_j, v = c delta, all fp32.  False (v = 0)
// for KEY_NONE or an index outside the target's count.
__device__ __forceinline__ bool nb_term(const NbBwd &a, int b, int nt, int i, int k, f3 &v, int &j) {
    v = f3{0.0f, 0.0f, 0.0f};
    j = -1;
    const int64_t e = ((int64_t)b * a.in.cap[0] + i) * a.in.K + k;
    const unsigned long long key = a.keys[e];
    if (key == KEY_NONE) return false;
    const uint32_t jj = (uint32_t)(key & 0xffffffffu);
    if (jj >= (uint32_t)nt) return false;
    const f3 s = ld3(a.in.pts[0], (int64_t)b * a.in.cap[0] + i), t = ld3(a.in.pts[1], (int64_t)b * a.in.cap[1] + jj);
    const float c = 2.0f * a.g_d2[e];
    v = f3{c * (s.x - t.x), c * (s.y - t.y), c * (s.z - t.z)};
    j = (int)jj;
    return true;
}

// grid (x: source rows, y: batch element): g_src (every row written) and the largest finite |v|
__global__ __launch_bounds__(NB_T) void nb_bwd_src_k(NbBwd a) {
    const int b = blockIdx.y, ns = nb_count(a.in, 0, b), nt = nb_count(a.in, 1, b);
    float *g_src = a.g_src + (int64_t)b * a.in.cap[0] * 3;
    uint32_t mx = 0;
    for (int i0 = blockIdx.x * NB_T; i0 < a.in.cap[0]; i0 += gridDim.x * NB_T) {
        const int i = i0 + threadIdx.x;
        if (i >= a.in.cap[0]) continue;
        f3 g{0.0f, 0.0f, 0.0f};
        if (i < ns)
            for (int k = 0; k < a.in.K; ++k) {
                f3 v;
                int j;
                if (!nb_term(a, b, nt, i, k, v, j)) continue;
                g = f3{g.x + v.x, g.y + v.y, g.z + v.z};
                mx = fold_max(fold_max(fold_max(mx, v.x), v.y), v.z);
            }
        st3(g_src, i, g);
    }
    fold_max_commit(a.fold.maxbits, mx);
}

// grid (x: slots (i, k), y: batch element): -v of every slot into its target's 128-bit sums
__global__ __launch_bounds__(NB_T) void nb_bwd_acc_k(NbBwd a) {
    const int b = blockIdx.y, ns = nb_count(a.in, 0, b), nt = nb_count(a.in, 1, b), K = a.in.K;
    const int E = det_scale(*a.fold.maxbits, a.lg);
    const int64_t total = (int64_t)ns * K;
    for (int64_t e = (int64_t)blockIdx.x * NB_T + threadIdx.x; e < total; e += (int64_t)gridDim.x * NB_T) {
        const int i = (int)(e / K), k = (int)(e - (int64_t)i * K);
        f3 v;
        int j;
        if (!nb_term(a, b, nt, i, k, v, j)) continue;
        const int64_t row = (int64_t)b * a.in.cap[1] + j;
        fold_add(a.fold, row, 0, -v.x, E);
        fold_add(a.fold, row, 1, -v.y, E);
        fold_add(a.fold, row, 2, -v.z, E);
    }
}

// grid (x: elements of g_tgt, y: batch element): every element of g_tgt is written
__global__ __launch_bounds__(NB_T) void nb_bwd_finish_k(NbBwd a) {
    const int b = blockIdx.y, nt = nb_count(a.in, 1, b);
    const int E = det_scale(*a.fold.maxbits, a.lg);
    const int64_t total = (int64_t)a.in.cap[1] * 3, base = (int64_t)b * total;
    for (int64_t t = (int64_t)blockIdx.x * NB_T + threadIdx.x; t < total; t += (int64_t)gridDim.x * NB_T) {
        const int j = (int)(t / 3), c = (int)(t - (int64_t)j * 3);
        float r = 0.0f;
        if (j < nt) r = fold_result(a.fold, (int64_t)b * a.in.cap[1] + j, c, E);
        a.g_tgt[base + t] = r;
    }
}

// ------------------------------------------------------------------ E: normals.  grid (x: source rows, y: batch element)
// One Jacobi rotation of the symmetric 3x3 (diagonal app, aqq; the rotated pair's entry apq; the third index's entries apr,
// aqr) and of the eigenvector columns vp, vq.  Everything stays in named registers: no indexed array, no scratch.
__device__ __forceinline__ void nb_jacobi(double &app, double &aqq, double &apq, double &apr, double &aqr, double &vp0, double &vp1,
                                          double &vp2, double &vq0, double &vq1, double &vq2) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));  // (an infinite theta: t = 0)
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double pr = c * apr - s * aqr, qr = s * apr + c * aqr;
    apr = pr; aqr = qr;
    const double p0 = c * vp0 - s * vq0, q0 = s * vp0 + c * vq0;
    const double p1 = c * vp1 - s * vq1, q1 = s * vp1 + c * vq1;
    const double p2 = c * vp2 - s * vq2, q2 = s * vp2 + c * vq2;
    vp0 = p0; vq0 = q0; vp1 = p1; vq1 = q1; vp2 = p2; vq2 = q2;
}

__global__ __launch_bounds__(NB_T) void nb_normals_k(NbIn in, const unsigned long long *__restrict__ keys, int mode,
                                                     const float *__restrict__ orient, float *__restrict__ normals,
                                                     float *__restrict__ variation) {
    const int b = blockIdx.y, K = in.K;
    const int ns = nb_count(in, 0, b), nt = nb_count(in, 1, b);
    const float *tgt = in.pts[1] + (int64_t)b * in.cap[1] * 3;
    for (int i = blockIdx.x * NB_T + threadIdx.x; i < in.cap[0]; i += gridDim.x * NB_T) {
        const int64_t row = (int64_t)b * in.cap[0] + i;
        f3 n{0.0f, 0.0f, 0.0f};
        float var = 0.0f;
        if (i < ns) {
            const unsigned long long *kr = keys + row * K;
            int m = 0;
            double sx = 0.0, sy = 0.0, sz = 0.0;
            for (int k = 0; k < K; ++k) {
                const unsigned long long key = kr[k];
                const uint32_t j = (uint32_t)(key & 0xffffffffu);
                if (key == KEY_NONE || j >= (uint32_t)nt) continue;
                const f3 t = ld3(tgt, j);
                sx += (double)t.x; sy += (double)t.y; sz += (double)t.z;
                ++m;
            }
            if (m >= 3) {
                const double inv = 1.0 / (double)m, mx = sx * inv, my = sy * inv, mz = sz * inv;
                double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
                for (int k = 0; k < K; ++k) {
                    const unsigned long long key = kr[k];
                    const uint32_t j = (uint32_t)(key & 0xffffffffu);
                    if (key == KEY_NONE || j >= (uint32_t)nt) continue;
                    const f3 t = ld3(tgt, j);
                    const double dx = (double)t.x - mx, dy = (double)t.y - my, dz = (double)t.z - mz;
                    a00 += dx * dx; a01 += dx * dy; a02 += dx * dz; a11 += dy * dy; a12 += dy * dz; a22 += dz * dz;
                }
                a00 *= inv; a01 *= inv; a02 *= inv; a11 *= inv; a12 *= inv; a22 *= inv;
                double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;  // vRC: row R of column C
                for (int sweep = 0; sweep < NB_SWEEPS; ++sweep) {
                    nb_jacobi(a00, a11, a01, a02, a12, v00, v10, v20, v01, v11, v21);  // (p, q, r) = (0, 1, 2)
                    nb_jacobi(a00, a22, a02, a01, a12, v00, v10, v20, v02, v12, v22);  // (0, 2, 1)
                    nb_jacobi(a11, a22, a12, a01, a02, v01, v11, v21, v02, v12, v22);  // (1, 2, 0)
                }
                // the smallest eigenvalue (the lowest column wins a tie) and its column
                // (blended with exact 0 / 1 weights: a select chain over nine registers becomes an indexed stack array)
                const bool is2 = a22 < fmin(a00, a11), is1 = !is2 && a11 < a00;
                const double w0 = (is1 || is2) ? 0.0 : 1.0, w1 = is1 ? 1.0 : 0.0, w2 = is2 ? 1.0 : 0.0;
                const double l0 = (w0 * a00 + w1 * a11) + w2 * a22;
                double nx = (w0 * v00 + w1 * v01) + w2 * v02, ny = (w0 * v10 + w1 * v11) + w2 * v12,
                       nz = (w0 * v20 + w1 * v21) + w2 * v22;
                const double len = sqrt((nx * nx + ny * ny) + nz * nz);
                if (len > 0.0) { nx /= len; ny /= len; nz /= len; }
                double dot = 0.0;
                if (mode == 1) {
                    const f3 p = ld3(in.pts[0], row), view = ld3(orient, b);
                    dot = (nx * ((double)view.x - (double)p.x) + ny * ((double)view.y - (double)p.y)) + nz * ((double)view.z - (double)p.z);
                } else if (mode == 2) {
                    const f3 r = ld3(orient, row);
                    dot = (nx * (double)r.x + ny * (double)r.y) + nz * (double)r.z;
                }
                if (dot < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
                n = f3{(float)nx, (float)ny, (float)nz};
                const double tr = (a00 + a11) + a22;
                var = tr > 0.0 ? (float)(l0 / tr) : 0.0f;
            }
        }
        st3(normals, row, n);
        if (variation) variation[row] = var;
    }
}

static inline bool nb_shape_ok(int B, int cap0, int cap1, int K) {
    return B > 0 && B <= 65535 && cap0 > 0 && cap1 > 0 && K >= 1 && K <= NB_KMAX;
}

}  // namespace gs

using namespace gs;

extern "C" {

void gs_set_knn_grid(int g_max) { g_knn_grid_cap = g_max > 0 ? g_max : 0; }

size_t gs_knn_ws_bytes(int B, int Ns_max, int Nt_max, int K) {
    if (!nb_shape_ok(B, Ns_max, Nt_max, K)) return 0;
    return nb_layout(B, Ns_max, Nt_max, K, nullptr, nullptr);
}

int gs_knn(const float *src, const int32_t *src_counts, int Ns_max, const float *tgt, const int32_t *tgt_counts, int Nt_max, int B,
           int K, uint64_t *keys, void *ws, size_t ws_bytes, gs_stream_t stream) {
    GS_REQUIRE(src && src_counts && tgt && tgt_counts && keys, "gs_knn: NULL argument");
    GS_REQUIRE(nb_shape_ok(B, Ns_max, Nt_max, K), "gs_knn: bad shape B=%d Ns_max=%d Nt_max=%d K=%d (1 <= K <= 32)", B, Ns_max, Nt_max, K);
    GS_REQUIRE_WS("gs_knn", ws, ws_bytes, gs_knn_ws_bytes(B, Ns_max, Nt_max, K));
    hipStream_t st = (hipStream_t)stream;
    NbWs w;
    nb_layout(B, Ns_max, Nt_max, K, ws, &w);
    const NbIn in{{src, tgt}, {src_counts, tgt_counts}, {Ns_max, Nt_max}, K, g_knn_grid_cap};
    const int capm = std::max(Ns_max, Nt_max);
    const dim3 rows(std::min(cdiv(capm, NB_T), 1024), B, 2);
    GS_HIP(hipMemsetAsync(w.bacc, 0, w.zero_bytes, st), "gs_knn/zero");
    hipLaunchKernelGGL(nb_bbox_k, dim3(std::min(cdiv(Nt_max, NB_T), 1024), B), dim3(NB_T), 0, st, in, w.bacc);
    hipLaunchKernelGGL(nb_hist_k, rows, dim3(NB_T), 0, st, in, w);
    hipLaunchKernelGGL(nb_scan_k, dim3(B, 2), dim3(1024), 0, st, in, w);
    hipLaunchKernelGGL(nb_scatter_k, rows, dim3(NB_T), 0, st, in, w);
    GS_LAUNCH_CHECK("gs_knn/bucket");
    const dim3 grid(cdiv(Ns_max, NB_T), B);
    unsigned long long *out = (unsigned long long *)keys;
    switch (nb_kbucket(K)) {
        case 8: hipLaunchKernelGGL(nb_search_k<8>, grid, dim3(NB_T), 0, st, in, w, out); break;
        case 16: hipLaunchKernelGGL(nb_search_k<16>, grid, dim3(NB_T), 0, st, in, w, out); break;
        default: hipLaunchKernelGGL(nb_search_k<32>, grid, dim3(NB_T), 0, st, in, w, out); break;
    }
    GS_LAUNCH_CHECK("gs_knn/search");
    return GS_OK;
}

size_t gs_knn_backward_ws_bytes(int B, int Ns_max, int Nt_max, int K) {
    if (!nb_shape_ok(B, Ns_max, Nt_max, K)) return 0;
    return nb_bwd_layout(B, Nt_max, nullptr, nullptr);
}

int gs_knn_backward(const float *src, const int32_t *src_counts, int Ns_max, const float *tgt, const int32_t *tgt_counts, int Nt_max,
                    int B, int K, const uint64_t *keys, const float *g_d2, float *g_src, float *g_tgt, void *ws, size_t ws_bytes,
                    gs_stream_t stream) {
    GS_REQUIRE(src && src_counts && tgt && tgt_counts && keys && g_d2 && g_src && g_tgt, "gs_knn_backward: NULL argument");
    GS_REQUIRE(nb_shape_ok(B, Ns_max, Nt_max, K), "gs_knn_backward: bad shape B=%d Ns_max=%d Nt_max=%d K=%d (1 <= K <= 32)", B, Ns_max,
               Nt_max, K);
    GS_REQUIRE(g_src != g_tgt, "gs_knn_backward: g_src and g_tgt must be distinct buffers");
    GS_REQUIRE_WS("gs_knn_backward", ws, ws_bytes, gs_knn_backward_ws_bytes(B, Ns_max, Nt_max, K));
    hipStream_t st = (hipStream_t)stream;
    NbBwd a;
    const size_t bytes = nb_bwd_layout(B, Nt_max, ws, &a);
    a.in = NbIn{{src, tgt}, {src_counts, tgt_counts}, {Ns_max, Nt_max}, K, 0};
    a.keys = (const unsigned long long *)keys;
    a.g_d2 = g_d2;
    a.g_src = g_src;
    a.g_tgt = g_tgt;
    a.lg = fold_lg((int64_t)Ns_max * K);  // no target row receives more terms
    GS_HIP(hipMemsetAsync(ws, 0, bytes, st), "gs_knn_backward/zero");
    hipLaunchKernelGGL(nb_bwd_src_k, dim3(rows_grid(Ns_max, NB_T, 4096), B), dim3(NB_T), 0, st, a);
    hipLaunchKernelGGL(nb_bwd_acc_k, dim3(rows_grid((int64_t)Ns_max * K, NB_T, 4096), B), dim3(NB_T), 0, st, a);
    GS_LAUNCH_CHECK("gs_knn_backward/fold");
    hipLaunchKernelGGL(nb_bwd_finish_k, dim3(rows_grid((int64_t)Nt_max * 3, NB_T, 4096), B), dim3(NB_T), 0, st, a);
    GS_LAUNCH_CHECK("gs_knn_backward/finish");
    return GS_OK;
}

int gs_knn_normals(const float *src, const int32_t *src_counts, int Ns_max, const float *tgt, const int32_t *tgt_counts, int Nt_max,
                   int B, int K, const uint64_t *keys, int mode, const float *orient, float *normals, float *variation,
                   gs_stream_t stream) {
    GS_REQUIRE(src && src_counts && tgt && tgt_counts && keys && normals, "gs_knn_normals: NULL argument");
    GS_REQUIRE(nb_shape_ok(B, Ns_max, Nt_max, K), "gs_knn_normals: bad shape B=%d Ns_max=%d Nt_max=%d K=%d (1 <= K <= 32)", B, Ns_max,
               Nt_max, K);
    GS_REQUIRE(mode >= 0 && mode <= 2, "gs_knn_normals: bad orientation mode %d", mode);
    GS_REQUIRE(mode == 0 || orient, "gs_knn_normals: orientation mode %d needs its viewpoint / reference normals", mode);
    const NbIn in{{src, tgt}, {src_counts, tgt_counts}, {Ns_max, Nt_max}, K, 0};
    hipLaunchKernelGGL(nb_normals_k, dim3(rows_grid(Ns_max, NB_T, 4096), B), dim3(NB_T), 0, (hipStream_t)stream, in,
                       (const unsigned long long *)keys, mode, orient, normals, variation);
    GS_LAUNCH_CHECK("gs_knn_normals");
    return GS_OK;
}

}  // extern "C"
