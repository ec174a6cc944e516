// gs_metrics_det.hpp -- the deterministic scatter of the chamfer reverse pass (torch.use_deterministic_algorithms).  Included
// by icp.hip, last: gs_detfold.hpp's kernels exist in that translation unit only, and a kernel defined after all the others
// leaves theirs as they were.  One launch stores -c delta of every source row as a contribution row (normal part zero), then
// det_fold_run adds each (batch element, direction)'s rows into the target cloud's adjoint: four launches per fold, Q = 1.
#pragma once
#include "gs_detfold.hpp"
#include "gs_metrics.hpp"

namespace gs {

// grid (x: source rows, y: batch element, z: direction)
__global__ __launch_bounds__(256) void cham_bwd_rows_k(ChamIn in, const unsigned long long *__restrict__ keys_ab,
                                                       const unsigned long long *__restrict__ keys_ba, const float *__restrict__ g2,
                                                       const float *__restrict__ g1, float *__restrict__ rows_ab,
                                                       float *__restrict__ rows_ba) {
    const int d = blockIdx.z, b = blockIdx.y;
    const int ns = cham_count(in, d, b);
    const unsigned long long *keys = d ? keys_ba : keys_ab;
    float *rows = (d ? rows_ba : rows_ab) + (int64_t)b * in.cap[d] * DET_ROW;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += gridDim.x * blockDim.x) {
        f3 v;
        int j;
        if (cham_contrib(in, keys, g2, g1, d, b, i, v, j)) det_store_row(rows, i, f3{-v.x, -v.y, -v.z}, f3{0.0f, 0.0f, 0.0f}, j);
        else det_store_none(rows, i);
    }
}

struct ChamDetWs {
    float *rows[2];  // per direction: (B, cap[d], DET_ROW)
    Fold fold;       // one fold's workspace (max(cap) x DET_NCH), reused by the folds in stream order
};
static size_t cham_det_layout(int B, int cap0, int cap1, void *ws, ChamDetWs *out) {
    Carve c{(char *)ws};
    ChamDetWs scratch, &r = out ? *out : scratch;
    const size_t capm = (size_t)std::max(cap0, cap1);
    r.rows[0] = c.take<float>((size_t)B * cap0 * DET_ROW * 4);
    r.rows[1] = c.take<float>((size_t)B * cap1 * DET_ROW * 4);
    r.fold = fold_carve(c, capm, DET_NCH);
    return c.off;
}

size_t chamfer_det_ws_bytes(int B, int cap0, int cap1) { return cham_det_layout(B, cap0, cap1, nullptr, nullptr); }

int chamfer_det_scatter(const ChamIn &in, int B, const unsigned long long *keys_ab, const unsigned long long *keys_ba, const float *g2,
                        const float *g1, float *g_a, float *g_b, void *ws, hipStream_t st, const char *name) {
    ChamDetWs w;
    cham_det_layout(B, in.cap[0], in.cap[1], ws, &w);
    hipLaunchKernelGGL(cham_bwd_rows_k, dim3(rows_grid(std::max(in.cap[0], in.cap[1]), 256, 2048), B, 2), dim3(256), 0, st, in, keys_ab, keys_ba, g2, g1,
                       w.rows[0], w.rows[1]);
    GS_LAUNCH_CHECK(name);
    float *g_pts[2] = {g_a, g_b};
    for (int b = 0; b < B; ++b)
        for (int d = 0; d < 2; ++d) {
            const int t = 1 - d;
            const DetWs dw{w.rows[d] + (int64_t)b * in.cap[d] * DET_ROW, w.fold};
            const int rc = det_fold_run(dw, 1, in.cap[d], in.cnt[d] + b, in.cnt[t] + b, in.cap[t], g_pts[t] + (int64_t)b * in.cap[t] * 3,
                                        nullptr, st, name);
            if (rc != GS_OK) return rc;
        }
    return GS_OK;
}

}  // namespace gs
