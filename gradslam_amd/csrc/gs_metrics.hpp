// gs_metrics.hpp -- what the two translation units of the map metrics share (metrics.hip: bucketing, search, statistics and
// the default reverse pass; gs_metrics_det.hpp inside icp.hip: the deterministic scatter, because gs_detfold.hpp defines
// kernels and so belongs to one translation unit only).
//
// Clouds come as the renderer takes them: side 0 = a (B, cap[0], 3), side 1 = b (B, cap[1], 3), fp32, padded, with
// (B,) int32 device counts.  Direction d searches the rows of side d (sources) in side 1 - d (targets): 0 is a -> b.
#pragma once
#include <algorithm>

#include "gs_icp_assoc.hpp"

namespace gs {

struct ChamIn {
    const float *pts[2];
    const int32_t *cnt[2];
    int cap[2];
};
__device__ __forceinline__ int cham_count(const ChamIn &in, int side, int b) { return min(max(in.cnt[side][b], 0), in.cap[side]); }

// Reverse pass of one source row: with j its nearest target (the key's index), delta = s_i - t_j, d = sqrt(d2) from the key's
// bits, c = 2 g2 + (d > 0 ? g1 / d : 0):  v = c delta is the source's adjoint, -v goes to target row j.  False (and v = 0)
// for KEY_NONE or an index outside the target's count.  g2 / g1: (B, 2) adjoints of sum d2 / sum d per direction.
__device__ __forceinline__ bool cham_contrib(const ChamIn &in, const unsigned long long *__restrict__ keys, const float *__restrict__ g2,
                                             const float *__restrict__ g1, int d, int b, int i, f3 &v, int &j) {
    v = f3{0.0f, 0.0f, 0.0f};
    j = -1;
    const unsigned long long key = keys[(int64_t)b * in.cap[d] + i];
    if (key == KEY_NONE) return false;
    const uint32_t jj = (uint32_t)(key & 0xffffffffu);
    if (jj >= (uint32_t)cham_count(in, 1 - d, b)) return false;
    const f3 s = ld3(in.pts[d], (int64_t)b * in.cap[d] + i), t = ld3(in.pts[1 - d], (int64_t)b * in.cap[1 - d] + jj);
    const float dd = sqrtf(bitsf((uint32_t)(key >> 32)));
    const float c = 2.0f * g2[2 * b + d] + (dd > 0.0f ? g1[2 * b + d] / dd : 0.0f);
    v = f3{c * (s.x - t.x), c * (s.y - t.y), c * (s.z - t.z)};
    j = (int)jj;
    return true;
}

// the deterministic scatter (gs_metrics_det.hpp): -v of every source folded into its target's row of g_pts[1 - d] in exact
// fixed point (gs_detfold.hpp); rows below the target's count are overwritten, the others untouched
size_t chamfer_det_ws_bytes(int B, int cap0, int cap1);
int chamfer_det_scatter(const ChamIn &in, int B, const unsigned long long *keys_ab, const unsigned long long *keys_ba, const float *g2,
                        const float *g1, float *g_a, float *g_b, void *ws, hipStream_t st, const char *name);

}  // namespace gs
