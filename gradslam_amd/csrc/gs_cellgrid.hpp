// gs_cellgrid.hpp -- the uniform cell grid over a cloud's bounding box that buckets arbitrary clouds: device functions only, no
// kernels, stated once for the translation units that bucket (metrics.hip: chamfer's scan order; neighbors.hip: the K-NN ring
// search).  How many cells per axis a cloud gets is the caller's rule (cham_g, nb_g); everything else is here.
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

}  // namespace gs
