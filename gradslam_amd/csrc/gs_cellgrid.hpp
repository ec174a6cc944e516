// gs_cellgrid.hpp -- the uniform cell grid over a cloud's bounding box that buckets arbitrary clouds: device functions only, no
// kernels, stated once for the translation units that bucket (metrics.hip: chamfer's scan order; neighbors.hip: the K-NN ring
// search).  How many cells per axis a cloud gets is the caller's rule (cham_g, nb_g), and so are the histogram's and the
// scatter's payload; the grid, the bounding box (cell_bbox) and the histogram's scan (cell_hist_scan) are here.
#pragma once
#include "gs_common.hpp"

namespace gs {

// order-preserving float -> uint32 (all finite values and the infinities) and back
__device__ __forceinline__ uint32_t ord_bits(float f) {
    const uint32_t u = __float_as_uint(f);
    return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}
__device__ __forceinline__ float ord_float(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o); }

// The cell grid of one cloud: cubic cells of side h = (longest extent) / g; an axis of extent e gets floor(e / h) + 1 cells, at
// most g (a flat or degenerate axis: one).  No extent at all (one point, all points equal, no point): one cell.  Every value is
// clamped, so a non-finite coordinate lands in some cell and never outside the table.
struct CellGrid {
    float lo[3], inv_h;
    int g[3], ncells;
};
__device__ __forceinline__ CellGrid cell_grid(const uint32_t *__restrict__ acc /* max x y z | ~min x y z */, int n, int g) {
    CellGrid G;
    G.lo[0] = G.lo[1] = G.lo[2] = 0.0f;
    G.inv_h = 0.0f;
    G.g[0] = G.g[1] = G.g[2] = 1;
    G.ncells = 1;
    if (n <= 0) return G;
    float ext[3], emax = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        G.lo[a] = ord_float(~acc[3 + a]);
        ext[a] = ord_float(acc[a]) - G.lo[a];
        emax = fmaxf(emax, ext[a]);
    }
    if (!(emax > 0.0f) || !(emax < INFINITY)) return G;
    G.inv_h = (float)g / emax;
#pragma unroll
    for (int a = 0; a < 3; ++a) G.g[a] = min((int)fminf(ext[a] * G.inv_h, (float)(g - 1)), g - 1) + 1;
    G.ncells = G.g[0] * G.g[1] * G.g[2];
    return G;
}
// the cell of a point per axis (its layer on that axis), and as one index (x fastest)
__device__ __forceinline__ void cell_xyz(const CellGrid &G, const f3 p, int &cx, int &cy, int &cz) {
    cx = min(max((int)((p.x - G.lo[0]) * G.inv_h), 0), G.g[0] - 1);
    cy = min(max((int)((p.y - G.lo[1]) * G.inv_h), 0), G.g[1] - 1);
    cz = min(max((int)((p.z - G.lo[2]) * G.inv_h), 0), G.g[2] - 1);
}
__device__ __forceinline__ int cell_of(const CellGrid &G, const f3 p) {
    int cx, cy, cz;
    cell_xyz(G, p, cx, cy, cz);
    return (cz * G.g[1] + cy) * G.g[0] + cx;
}

// The bounding box of the rows [0, n) of one cloud, by the blocks of T threads along grid.x, into the cloud's accumulator
// (max x y z | ~min x y z, zeroed by the caller): integer atomic max on order-preserving bit patterns, exact.  acc_of() gives
// the accumulator: asked for after the rows, where the kernels took its address, so that their code stays what it was.
template <class AccOf>
__device__ __forceinline__ void cell_bbox(const float *pts, int n, AccOf acc_of, int T) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * T + threadIdx.x; i < n; i += gridDim.x * T) {
        const f3 p = ld3(pts, i);
        lo[0] = fminf(lo[0], p.x); lo[1] = fminf(lo[1], p.y); lo[2] = fminf(lo[2], p.z);
        hi[0] = fmaxf(hi[0], p.x); hi[1] = fmaxf(hi[1], p.y); hi[2] = fmaxf(hi[2], p.z);
    }
    uint32_t *acc = acc_of();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float l = wave_min_f(lo[a]), h = wave_max_f(hi[a]);
        if ((threadIdx.x & 63) == 0 && l <= h) {  // (a wave without rows: +inf > -inf)
            atomicMax(acc + a, ord_bits(h));
            atomicMax(acc + 3 + a, ~ord_bits(l));
        }
    }
}

// The exclusive scan of hist[0 .. ncells) in place by one block of 1024 threads: every wave scans one contiguous stretch of the
// cells, 64 at a time; wtot: 16 ints of LDS; lane, wave: threadIdx.x & 63, threadIdx.x >> 6, taken at the kernel's top, where
// the kernels computed them, so that their code stays what it was.
__device__ __forceinline__ void cell_hist_scan(int32_t *hist, int ncells, int *wtot, int lane, int wave) {
    const int seg = ((ncells + 15) / 16 + 63) & ~63;
    const int c0 = min(wave * seg, ncells), c1 = min(c0 + seg, ncells);
    int run = 0;
    for (int c = c0; c < c1; c += 64) {
        const int idx = c + lane;
        const int v = idx < c1 ? hist[idx] : 0;
        int inc = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(inc, off, kWave);
            if (lane >= off) inc += t;
        }
        if (idx < c1) hist[idx] = run + inc - v;
        run += __shfl(inc, 63, kWave);
    }
    if (lane == 0) wtot[wave] = run;
    __syncthreads();
    int base = 0;
    for (int k = 0; k < wave; ++k) base += wtot[k];
    if (base)
        for (int c = c0 + lane; c < c1; c += 64) hist[c] += base;
}

}  // namespace gs
