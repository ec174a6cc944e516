// gs_detfold.hpp -- the deterministic fold of the scattered target / normal adjoints (torch.use_deterministic_algorithms).
//
// The default reverse passes add d_bar / n_bar of every source i into row j = NN(i) of g_tgt / g_nrm with float atomics, in
// arrival order.  The DET variants store each contribution instead -- one row of DET_ROW words per (launch q, source i):
// d_bar (3) | n_bar (3) | j (int bits, -1 = no contribution) | pad -- and fold the rows into the targets afterwards in four
// launches, however many reverse launches wrote rows: det_clear_k, det_max_k, det_acc_k, det_finish_k.  The fold is the exact
// one of gs_fixed128.hpp (the rule, its scale and its flags are stated there), over cap_t rows of DET_NCH sums.
#pragma once
#include "gs_common.hpp"
#include "gs_fixed128.hpp"

namespace gs {

constexpr int DET_ROW = 8;  // words per stored contribution

__device__ __forceinline__ void det_store_row(float *__restrict__ rows, int64_t i, const f3 dt, const f3 dn, int j) {
    int4 *p = reinterpret_cast<int4 *>(rows + DET_ROW * i);
    p[0] = make_int4(__float_as_int(dt.x), __float_as_int(dt.y), __float_as_int(dt.z), __float_as_int(dn.x));
    p[1] = make_int4(__float_as_int(dn.y), __float_as_int(dn.z), j, 0);
}
__device__ __forceinline__ void det_store_none(float *__restrict__ rows, int64_t i) {
    reinterpret_cast<int *>(rows)[DET_ROW * i + 6] = -1;
}

constexpr int DET_NCH = 6;  // sums per target: d_bar (3) | n_bar (3)

struct DetWs {
    float *rows;  // Q x cap_s x DET_ROW
    Fold fold;    // cap_t x DET_NCH
};
static inline size_t det_ws_layout(int Q, int cap_s, int cap_t, void *ws, DetWs *out) {
    Carve c{(char *)ws};
    DetWs scratch, &r = out ? *out : scratch;
    r.rows = c.take<float>((size_t)Q * cap_s * DET_ROW * 4);
    r.fold = fold_carve(c, (size_t)cap_t, DET_NCH);
    return c.off;
}

// zeroes the rows below the device count only (a memset cannot)
__global__ void det_clear_k(uint32_t *__restrict__ maxbits, uint32_t *__restrict__ flags, unsigned long long *__restrict__ acc,
                            const int32_t *__restrict__ d_nt, int cap_t) {
    const int nt = min(*d_nt, cap_t);
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (int i = tid; i < 12 * nt; i += stride) acc[i] = 0ull;
    for (int i = tid; i < nt; i += stride) flags[i] = 0u;
    if (tid == 0) *maxbits = 0u;
}

// grid (x: sources, y: launch q)
__global__ __launch_bounds__(256) void det_max_k(const float *__restrict__ rows, int cap_s, const int32_t *__restrict__ d_ns, Fold f) {
    const int ns = min(*d_ns, cap_s);
    const int4 *R = reinterpret_cast<const int4 *>(rows + (size_t)blockIdx.y * cap_s * DET_ROW);
    uint32_t m = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += gridDim.x * blockDim.x) {
        const int4 a = R[2 * i], b = R[2 * i + 1];
        if (b.z < 0) continue;
        const int w[DET_NCH] = {a.x, a.y, a.z, a.w, b.x, b.y};
#pragma unroll
        for (int c = 0; c < DET_NCH; ++c) m = fold_max(m, __int_as_float(w[c]));
    }
    fold_max_commit(f.maxbits, m);
}

__global__ __launch_bounds__(256) void det_acc_k(const float *__restrict__ rows, int cap_s, const int32_t *__restrict__ d_ns,
                                                 const int32_t *__restrict__ d_nt, int cap_t, int lg, Fold f) {
    const int ns = min(*d_ns, cap_s), nt = min(*d_nt, cap_t);
    const int E = det_scale(*f.maxbits, lg);
    const int4 *R = reinterpret_cast<const int4 *>(rows + (size_t)blockIdx.y * cap_s * DET_ROW);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += gridDim.x * blockDim.x) {
        const int4 a = R[2 * i], b = R[2 * i + 1];
        const int j = b.z;
        if (j < 0 || j >= nt) continue;
        const int w[DET_NCH] = {a.x, a.y, a.z, a.w, b.x, b.y};
#pragma unroll
        for (int c = 0; c < DET_NCH; ++c) fold_add(f, j, c, __int_as_float(w[c]), E);
    }
}

// rows < min(nt, cap_t) of g_tgt / g_nrm (either may be NULL) are written, nothing else
__global__ void det_finish_k(Fold f, int lg, const int32_t *__restrict__ d_nt, int cap_t, float *__restrict__ g_tgt,
                             float *__restrict__ g_nrm) {
    const int nt = min(*d_nt, cap_t);
    const int E = det_scale(*f.maxbits, lg);
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < DET_NCH * nt; t += gridDim.x * blockDim.x) {
        const int row = t / DET_NCH, c = t - DET_NCH * row;
        float *out = c < 3 ? g_tgt : g_nrm;
        if (!out) continue;
        out[3 * (int64_t)row + (c % 3)] = fold_result(f, row, c, E);
    }
}

// the four fold launches over Q launches' rows (cap_s rows each, the first *d_ns of them written); a target receives at most
// Q cap_s contributions
static inline int det_fold_run(const DetWs &w, int Q, int cap_s, const int32_t *d_ns, const int32_t *d_nt, int cap_t, float *g_tgt,
                               float *g_nrm, hipStream_t st, const char *name) {
    const int lg = fold_lg((int64_t)Q * cap_s);
    const Fold &f = w.fold;
    hipLaunchKernelGGL(det_clear_k, dim3(min(cdiv((int64_t)12 * cap_t, 256), 1024)), dim3(256), 0, st, f.maxbits, f.flags, f.acc, d_nt, cap_t);
    const dim3 grid(min(cdiv(cap_s, 256), 256), Q);
    hipLaunchKernelGGL(det_max_k, grid, dim3(256), 0, st, (const float *)w.rows, cap_s, d_ns, f);
    hipLaunchKernelGGL(det_acc_k, grid, dim3(256), 0, st, (const float *)w.rows, cap_s, d_ns, d_nt, cap_t, lg, f);
    hipLaunchKernelGGL(det_finish_k, dim3(min(cdiv((int64_t)DET_NCH * cap_t, 256), 1024)), dim3(256), 0, st, f, lg, d_nt, cap_t, g_tgt, g_nrm);
    GS_LAUNCH_CHECK(name);
    return GS_OK;
}

}  // namespace gs
