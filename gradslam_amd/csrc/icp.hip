// icp.hip -- exact 1-NN association (K), linearise + 6x6 reduce (J), the O(1) solve / SE(3)
// exponential / LM control (X), and whole ICP / gradICP loops that never leave the device.
//
// One translation unit; the device code lives in role headers, each with its part of the design at its top:
//   gs_icp_assoc.hpp   K  keys, row algebra, the tile search (chunk boxes, grid windows) up to knn_tile
//   gs_icp_reduce.hpp  J  the rp_* partial-row reduction, expand44 (a block's row: gs_rowsum.hpp)
//   gs_icp_step.hpp    X  IcpState, LoopBufs, solve6*, se3_exp_dev, GradParams, tape records, step_wave0
//   gs_icp_loop.hpp       LoopConst, the camera proof, knn1_loop_k, icp_init_state_k, icp_prepare_k, copy_best_last_k
//   gs_icp_bwd.hpp        the reverse pass: BwdState ... bwd_finish_k, bwd_ws_layout
//   gs_icp.hpp            what slam.hip calls here
// This file: the stand-alone kernels behind gs_knn1* / gs_icp_linearize* / gs_icp_rows / gs_transform_points, icp_step_k, launch
// geometry, profiling, the knobs, the workspace and tape layouts, icp_run, icp_backward_run and the C entry points.
#include <stddef.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

#include "gs_detfold.hpp"
#include "gs_icp.hpp"
#include "gs_icp_reduce.hpp"
#include "gs_rowsum.hpp"

namespace gs {

// ------------------------------------------------------------------ K: brute force (verifier / tiny inputs)
__global__ __launch_bounds__(KNN_T) void knn1_brute_k(const float *__restrict__ src, const int32_t *__restrict__ d_ns,
                                                      const float *__restrict__ tgt, const int32_t *__restrict__ d_nt,
                                                      int nsplit, unsigned long long *__restrict__ best) {
    const int ns = *d_ns, nt = *d_nt;
    const int i = blockIdx.x * KNN_T + threadIdx.x;
    if (blockIdx.x * KNN_T >= ns) return;
    const int chunk = (nt + nsplit - 1) / nsplit;
    const int j0 = blockIdx.y * chunk, j1 = min(nt, j0 + chunk);
    const bool ok = i < ns;
    const f3 s = ok ? ld3(src, i) : f3{0.0f, 0.0f, 0.0f};
    float bd = INFINITY;
    int bi = 0;
    for (int j = j0; j < j1; ++j) {  // wave-uniform j: tgt[j] lives in SGPRs
        const float d = dist2(s, tgt[3 * j], tgt[3 * j + 1], tgt[3 * j + 2]);
        if (d < bd) { bd = d; bi = j; }  // strict: lowest index wins
    }
    if (ok && bd < INFINITY) atomicMin(best + i, pack_key(bd, bi));
}

// ------------------------------------------------------------------ K: AABB-pruned exact search
// boxes: per chunk 6 floats (lo.xyz, hi.xyz).  One wave covers 64 target points = 64/CHUNK chunks
// (segmented butterfly inside each CHUNK-lane group).
__global__ __launch_bounds__(64) void tgt_boxes_k(const float *__restrict__ tgt, const int32_t *__restrict__ d_nt,
                                                  float *__restrict__ boxes) {
    const int nt = *d_nt;
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (blockIdx.x * 64 >= nt) return;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (j < nt) {
        const f3 p = ld3(tgt, j);
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
    if ((threadIdx.x % CHUNK) == 0 && j < nt) {
        float *b = boxes + 6 * (int64_t)(j / CHUNK);
        b[0] = lo[0]; b[1] = lo[1]; b[2] = lo[2]; b[3] = hi[0]; b[4] = hi[1]; b[5] = hi[2];
    }
}

// Stand-alone pruned search (gs_knn1): no transform, sampled seed pass.
__global__ __launch_bounds__(KNN_BT) void knn1_box_k(const float *__restrict__ src, const int32_t *__restrict__ d_ns,
                                                     const float *__restrict__ tgt, const float *__restrict__ boxes,
                                                     const int32_t *__restrict__ d_nt, unsigned long long *__restrict__ best) {
    __shared__ KnnShared sh;
    const int ns = *d_ns, nt = *d_nt;
    const int tile0 = blockIdx.x * 64;
    if (tile0 >= ns) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = tile0 + lane;
    const bool ok = i < ns;
    const f3 s = ok ? ld3(src, i) : f3{0.0f, 0.0f, 0.0f};
    if (nt <= 0) {
        if (ok && wave == 0) best[i] = KEY_NONE;
        return;
    }
    const unsigned long long key = knn_tile<KNN_NW>(sh, s, ok, -1, tgt, tgt, nullptr, boxes, nullptr, nt);
    if (ok && wave == 0) best[i] = key;
}

__global__ void knn_unpack_k(const unsigned long long *__restrict__ best, const int32_t *__restrict__ d_ns,
                             float *__restrict__ dist2_out, int64_t *__restrict__ idx) {
    const int ns = *d_ns;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += gridDim.x * blockDim.x) {
        const unsigned long long k = best[i];
        if (dist2_out) dist2_out[i] = bitsf((uint32_t)(k >> 32));
        if (idx) idx[i] = (int64_t)(uint32_t)(k & 0xffffffffu);
    }
}

__global__ void fill_u64_k(unsigned long long *__restrict__ p, int n, unsigned long long v) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = v;
}

// ------------------------------------------------------------------ J: stand-alone kernels
__global__ __launch_bounds__(LIN_T) void linearize_k(const float *__restrict__ src, const int32_t *__restrict__ d_ns,
                                                     const float *__restrict__ tgt, const float *__restrict__ nrm,
                                                     const unsigned long long *__restrict__ best, float thresh,
                                                     float *__restrict__ partials /* gridDim.x x NACC */) {
    const int ns = *d_ns;
    float acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0f;
    for (int i = blockIdx.x * LIN_T + threadIdx.x; i < ns; i += gridDim.x * LIN_T) {
        const Row r = make_row(src, tgt, nrm, best, i, ns, thresh);
        if (r.valid) accumulate_row(r, acc);
    }
    block_row<NACC, LIN_T / kWave>(acc, [&](unsigned n) { return &partials[blockIdx.x * NACC + n]; });
}

__global__ __launch_bounds__(1024) void finalize44_k(const float *__restrict__ partials, int nblocks, float *__restrict__ out44) {
    __shared__ float acc[NACC];
    reduce_partials(partials, nblocks, acc);
    if (threadIdx.x == 0) expand44(acc, out44);
}

__global__ void icp_rows_k(const float *__restrict__ src, const int32_t *__restrict__ d_ns, const float *__restrict__ tgt,
                           const float *__restrict__ nrm, const unsigned long long *__restrict__ best, float thresh,
                           float *__restrict__ A, float *__restrict__ bvec, uint8_t *__restrict__ keep) {
    const int ns = *d_ns;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += gridDim.x * blockDim.x) {
        const Row r = make_row(src, tgt, nrm, best, i, ns, thresh);
        keep[i] = r.valid ? 1 : 0;
#pragma unroll
        for (int u = 0; u < 6; ++u) A[6 * (int64_t)i + u] = r.valid ? r.a[u] : 0.0f;
        bvec[i] = r.valid ? r.b : 0.0f;
    }
}

// adjoint of linearize.  DET: g_tgt = contribution rows (gs_detfold.hpp), g_nrm unused
template <bool DET>
__global__ void linearize_bwd_k(const float *__restrict__ src, const int32_t *__restrict__ d_ns,
                                const float *__restrict__ tgt, const float *__restrict__ nrm,
                                const unsigned long long *__restrict__ best, float thresh,
                                const float *__restrict__ gout /*43: Hbar36 | gbar6 | ebar*/, float *__restrict__ g_src,
                                float *__restrict__ g_tgt, float *__restrict__ g_nrm) {
    const int ns = *d_ns;
    __shared__ float G[43];
    if (threadIdx.x < 43) G[threadIdx.x] = gout[threadIdx.x];
    __syncthreads();
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += gridDim.x * blockDim.x) {
        const Row r = make_row(src, tgt, nrm, best, i, ns, thresh);
        if (!r.valid) {
            if (g_src) st3(g_src, i, f3{0, 0, 0});
            if (DET && g_tgt) det_store_none(g_tgt, i);
            continue;
        }
        const uint32_t j = (uint32_t)(best[i] & 0xffffffffu);
        const f3 s = ld3(src, i), d = ld3(tgt, j), n = ld3(nrm, j);
        float ab[6];
#pragma unroll
        for (int u = 0; u < 6; ++u) {
            float v = G[36 + u] * r.b;
#pragma unroll
            for (int w = 0; w < 6; ++w) v += (G[6 * u + w] + G[6 * w + u]) * r.a[w];
            ab[u] = v;
        }
        float bb = 2.0f * G[42] * r.b;
#pragma unroll
        for (int u = 0; u < 6; ++u) bb += G[36 + u] * r.a[u];
        // a = [n ; s x n]
        const f3 an{ab[0], ab[1], ab[2]}, ac{ab[3], ab[4], ab[5]};
        // c = s x n: s_bar = n x c_bar ; n_bar += c_bar x s
        f3 sb{n.y * ac.z - n.z * ac.y, n.z * ac.x - n.x * ac.z, n.x * ac.y - n.y * ac.x};
        f3 nb{an.x + (ac.y * s.z - ac.z * s.y), an.y + (ac.z * s.x - ac.x * s.z), an.z + (ac.x * s.y - ac.y * s.x)};
        // b = n.(d - s)
        sb.x -= bb * n.x; sb.y -= bb * n.y; sb.z -= bb * n.z;
        nb.x += bb * (d.x - s.x); nb.y += bb * (d.y - s.y); nb.z += bb * (d.z - s.z);
        if (g_src) st3(g_src, i, sb);
        if constexpr (DET) {
            if (g_tgt) det_store_row(g_tgt, i, f3{bb * n.x, bb * n.y, bb * n.z}, nb, (int)j);
            continue;
        }
        if (g_tgt) {
            atomicAdd(g_tgt + 3 * (int64_t)j, bb * n.x);
            atomicAdd(g_tgt + 3 * (int64_t)j + 1, bb * n.y);
            atomicAdd(g_tgt + 3 * (int64_t)j + 2, bb * n.z);
        }
        if (g_nrm) {
            atomicAdd(g_nrm + 3 * (int64_t)j, nb.x);
            atomicAdd(g_nrm + 3 * (int64_t)j + 1, nb.y);
            atomicAdd(g_nrm + 3 * (int64_t)j + 2, nb.z);
        }
    }
}

__global__ void transform_k(const float *__restrict__ pts, const int32_t *__restrict__ d_n, const float *__restrict__ T,
                            float *__restrict__ out) {
    const int n = *d_n;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) st3(out, i, xform(T, ld3(pts, i)));
}

}  // namespace gs

// The loops' kernels are included here, after the stand-alone ones, not at the top: the compiler emits kernels in the
// order of their definitions, so moving these includes changes the code object (same kernels, other order).
#include "gs_icp_loop.hpp"
#include "gs_icp_bwd.hpp"

namespace gs {

// ------------------------------------------------------------------ launch geometry
static inline int knn_nsplit_brute(int max_ns, int max_nt) {
    const int tiles = cdiv(max_ns, KNN_T);
    int ns = cdiv(2048, tiles);
    const int cap = cdiv(max_nt, 64);
    if (ns > cap) ns = cap;
    if (ns < 1) ns = 1;
    if (ns > 4096) ns = 4096;
    return ns;
}
static inline int lin_blocks(int max_ns) {
    int nb = cdiv(max_ns, LIN_T);
    if (nb > LIN_MAXB) nb = LIN_MAXB;
    if (nb < 1) nb = 1;
    return nb;
}
static inline size_t boxes_bytes(int max_nt) { return (size_t)cdiv(max_nt > 0 ? max_nt : 1, CHUNK) * 6 * 4; }

// ------------------------------------------------------------------ optional per-kernel timing
// bench.py asks for the average duration of the two hot kernels of the loop, measured with HIP events
// on the stream they are launched on.  Off by default (no events, no overhead).
struct Prof {
    bool on = false;
    std::vector<hipEvent_t> ev[2][2];  // [tag][start|stop]
    size_t used[2] = {0, 0};
    double total_ms[2] = {0.0, 0.0};
    long count[2] = {0, 0};
};
static Prof g_prof;
static inline void prof_mark(int tag, int which, hipStream_t st) {
    if (!g_prof.on) return;
    auto &v = g_prof.ev[tag][which];
    const size_t i = g_prof.used[tag];
    if (i >= v.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        v.push_back(e);
    }
    (void)hipEventRecord(v[i], st);
    if (which == 1) g_prof.used[tag] = i + 1;
}

bool profiling_enabled() { return g_prof.on; }

static int g_grid_mode = getenv("GS_GRID_MODE") ? atoi(getenv("GS_GRID_MODE")) : 1;  // gs_set_grid_search (environment: measurements)
static int g_tile_points = 0;  // gs_set_tile_points (0 = automatic)
static int g_loop_waves = 0;   // gs_set_loop_waves (0 = automatic)

// Source points per block of the loops' association kernel (knn1_loop_k): 64 -- lane = point.  Round 2 cut a dense
// target's cloud into 38-point tiles (every CU two equal tiles: the chunk-box search there was VALU-issue bound and a
// launch lasted as long as its doubled-up CUs); with the grid search's geometric proof the launch is latency-bound at every
// density and the tile size no longer matters (200 frames, MI355X: 1 864 / 1 842 / 1 838 frames/s for 64 / the round-2 rule /
// 38, profiles/r03d), so the rule is gone and with it the surplus blocks it launched while a map grew dense.  The
// setting remains for tests (gs_set_tile_points): the tile size fixes the order of the 29-term sums, so results of
// different settings agree to rounding, nearest neighbours exactly.
constexpr int TILE_MIN = 32;
static inline int loop_tile_points() {
    static const int env = getenv("GS_TILE_POINTS") ? atoi(getenv("GS_TILE_POINTS")) : 0;
    const int forced = g_tile_points ? g_tile_points : env;
    return (forced >= TILE_MIN && forced <= 64) ? forced : 64;
}
// Waves per block of the loops' association kernel.  Results do not depend on it (see knn1_loop_k), so the host chooses
// freely: eight where the grid search runs -- two such blocks on a CU are the sixteen waves one block used to be, and the
// launch lasts as long as the CUs that host two ("eight-wave blocks") -- sixteen for the chunk-box
// search, which is VALU-bound, and for a target whose CAPACITY exceeds LOOP_WAVES_DENSE slots per grid pixel: a long
// sequence's arena, where the 200-frame forward measured 2 % slower with eight (capacity 218 per pixel; the c2 step,
// capacity 27, is where eight gain).  gs_set_loop_waves / GS_LOOP_WAVES (8 or 16) force one for A/B runs and tests.
constexpr int LOOP_WAVES_DENSE = 64;
static inline int loop_waves(bool grid_search, int max_nt, int cells) {
    static const int env = getenv("GS_LOOP_WAVES") ? atoi(getenv("GS_LOOP_WAVES")) : 0;
    const int forced = g_loop_waves ? g_loop_waves : env;
    if (forced == 8 || forced == 16) return forced;
    return (grid_search && (int64_t)max_nt <= (int64_t)LOOP_WAVES_DENSE * cells) ? 8 : 16;
}
int icp_config_stamp() { return g_grid_mode | (g_tile_points << 4) | (g_loop_waves << 12); }  // part of slam.hip's graph-cache key
static inline int loop_blocks_max(int max_ns) { return cdiv(max_ns, TILE_MIN); }  // workspace: whatever the tile size
// rows of a partial-sum buffer: the association kernel's prologue reads rows 0 .. 32 RP_LOADS - 1 without testing them against
// the launch's row count (icp_prepare_k zeroes the rows the loop's launches do not write), four bytes at a time up to twelve
// bytes past a row's end: one spare row
static inline int partial_rows_alloc(int max_ns) { return std::max(loop_blocks_max(max_ns), 32 * RP_LOADS) + 1; }

struct IcpWs {
    IcpState *S[2];      // double-buffered across launches (see knn1_loop_k)
    LoopBufs B;
    float *partials[2];
    float *boxes, *sboxes;  // chunk boxes, and one box per SUPER chunks
    LoopConst *lc;       // the loop's constants (knn1_loop_k reads them from here, not from its arguments)
    int32_t *cells;      // grid search: (2, max_ns) ds-grid pixel of every point an association wrote, by launch parity
};
// n equal pieces in a row, as LoopBufs wants its slots: the first one's address, *stride = a piece's size in elements
template <class T>
static inline T *take_slots(Carve &c, int n, size_t bytes, int64_t *stride) {
    const size_t o = c.off;
    T *first = c.take<T>(bytes);
    *stride = (int64_t)((c.off - o) / sizeof(T));
    for (int k = 1; k < n; ++k) c.take(bytes);
    return first;
}
static inline size_t icp_ws_layout(int max_ns, int max_nt, void *ws, IcpWs *out) {
    Carve c{(char *)ws};
    IcpWs scratch, &w = out ? *out : scratch;
    const size_t part_b = (size_t)partial_rows_alloc(max_ns) * NACC * 4;
    w.S[0] = c.take<IcpState>(sizeof(IcpState)); w.S[1] = c.take<IcpState>(sizeof(IcpState));
    w.B.pts = take_slots<float>(c, 2, (size_t)max_ns * 12, &w.B.pts_stride);
    w.B.best = take_slots<unsigned long long>(c, 2, (size_t)max_ns * 8, &w.B.best_stride);
    w.partials[0] = c.take<float>(part_b); w.partials[1] = c.take<float>(part_b);
    w.boxes = c.take<float>(boxes_bytes(max_nt));
    w.sboxes = c.take<float>((size_t)cdiv(max_nt > 0 ? max_nt : 1, 1024) * 6 * 4);
    w.lc = c.take<LoopConst>(sizeof(LoopConst));
    w.cells = c.take<int32_t>((size_t)max_ns * 12);  // cells by launch parity (2 planes) | the loop's copy of hints.src_pix
    return c.off;
}

// ------------------------------------------------------------------ tape (autograd)
// [records: (steps + 1) x REC_WORDS floats][cloud slots][nearest-neighbour slots]; one slot per association
// launch, one record per step launch.  LM: numiters + 1 of each; gradLM: 2 numiters of each.
struct Tape {
    float *rec;
    LoopBufs B;
    int nslots;
};
static inline int tape_launches(bool grad, int numiters) { return grad ? 2 * numiters : numiters + 1; }
static inline size_t tape_layout(bool grad, int max_ns, int numiters, void *tape, Tape *out) {
    Carve c{(char *)tape};
    Tape scratch, &t = out ? *out : scratch;
    t.nslots = tape_launches(grad, numiters > 0 ? numiters : 1);
    t.rec = c.take<float>((size_t)(t.nslots + 1) * REC_WORDS * 4);
    t.B.pts = take_slots<float>(c, t.nslots, (size_t)max_ns * 12, &t.B.pts_stride);
    t.B.best = take_slots<unsigned long long>(c, t.nslots, (size_t)max_ns * 8, &t.B.best_stride);
    return c.off;
}

// GradParams of a gradLM loop from the caller's lambda_max / B / B2 / nu, and what the plain LM loops pass in their place
static inline GradParams make_grad_params(float lambda_max, float B, float B2, float nu) {
    return GradParams{(float)(1.0 / (double)lambda_max), (float)((double)lambda_max - 1.0 / (double)lambda_max), B, B2,
                      (float)(1.0 / (double)nu)};
}
static inline GradParams lm_grad_params() { return GradParams{0.5f, 1.5f, 1.0f, 1.0f, 0.005f}; }

// X as a launch of its own (a loop's last step): step_wave0 on an LDS copy of the state.  grid 1, 1024 threads
__global__ __launch_bounds__(1024) void icp_step_k(IcpState *__restrict__ Sg, const float *__restrict__ partials, int nblocks,
                                                  int mode, GradParams gp, float *__restrict__ trace /* or NULL */,
                                                  float *__restrict__ out_T, int look_slot,
                                                  float *__restrict__ rec /* this step's tape record or NULL */, int solve,
                                                  const float *__restrict__ compose_right, float *__restrict__ compose_out) {
    __shared__ float acc[NACC];
    __shared__ double lu_sm[42];
    __shared__ IcpState st;  // work on an LDS copy: ~200 dependent accesses at LDS, not HBM, latency
    constexpr int kWords = sizeof(IcpState) / 4;
#ifdef GS_DIAG_STAMPS
    if (g_diag && threadIdx.x == 0) g_diag[0] = wall_clock64();
#endif
    if (threadIdx.x < kWords) reinterpret_cast<int *>(&st)[threadIdx.x] = reinterpret_cast<const int *>(Sg)[threadIdx.x];
    reduce_partials(partials, nblocks, acc);  // ends with a barrier: st and acc are visible
    // (from the global copy: wave 0 is about to change the LDS one)
    if (rec && threadIdx.x < kWords) reinterpret_cast<int *>(rec)[REC_STATE + threadIdx.x] = reinterpret_cast<const int *>(Sg)[threadIdx.x];
#ifdef GS_DIAG_STAMPS
    if (g_diag && threadIdx.x == 0) g_diag[1] = wall_clock64();
#endif
    if (threadIdx.x < 64) step_wave0(&st, acc, mode, gp, trace, out_T, look_slot, rec, lu_sm, solve != 0);
#ifdef GS_DIAG_STAMPS
    if (g_diag && threadIdx.x == 0) g_diag[2] = wall_clock64();
#endif
    __syncthreads();
    if (threadIdx.x < kWords) {
        const int v = reinterpret_cast<const int *>(&st)[threadIdx.x];
        reinterpret_cast<int *>(Sg)[threadIdx.x] = v;
        if (rec) reinterpret_cast<int *>(rec)[REC_WORDS + REC_STATE + threadIdx.x] = v;  // head of the next record = state after
    }
    if (compose_out && threadIdx.x == 0) compose44(st.T, compose_right, compose_out);  // e.g. T . previous pose
}

static int icp_run(bool grad, const float *src, const int32_t *d_ns, int max_ns, const float *tgt, const float *nrm,
                   const int32_t *d_nt, int max_nt, const float *init_T, int numiters, float damp, float thresh,
                   GradParams gp, const gs_icp_hints *hints_in, float *out_T, uint64_t *best_last, float *trace, void *ws,
                   size_t ws_bytes, hipStream_t st, const char *name, void *tape = nullptr, size_t tape_bytes = 0,
                   const float *compose_right = nullptr, float *compose_out = nullptr) {
    gs_icp_hints hints{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, 0};
    if (hints_in) hints = *hints_in;
    GS_REQUIRE(!hints.scan_points || hints.scan_orig, "%s: hints.scan_points needs hints.scan_orig", name);
    GS_REQUIRE(src && d_ns && tgt && nrm && d_nt && out_T, "%s: NULL argument", name);  // init_T NULL = identity
    GS_REQUIRE(max_ns > 0 && max_nt > 0 && numiters >= 0, "%s: bad sizes max_ns=%d max_nt=%d numiters=%d", name, max_ns, max_nt, numiters);
    IcpWs w;
    GS_REQUIRE_WS(name, ws, ws_bytes, icp_ws_layout(max_ns, max_nt, ws, &w));
    if (numiters == 0) {
        if (init_T) {
            GS_HIP(hipMemcpyAsync(out_T, init_T, 64, hipMemcpyDeviceToDevice, st), name);
        } else {
            hipLaunchKernelGGL(icp_init_state_k, dim3(1), dim3(64), 0, st, w.S[0], init_T, damp);
            GS_HIP(hipMemcpyAsync(out_T, w.S[0], 64, hipMemcpyDeviceToDevice, st), name);  // IcpState starts with T
        }
        return GS_OK;
    }
    Tape tp{nullptr, {}, 0};
    if (tape) {
        GS_REQUIRE_TAPE(name, tape, tape_bytes, tape_layout(grad, max_ns, numiters, tape, &tp), GS_ERR_WORKSPACE_TOO_SMALL);
        w.B = tp.B;  // the tape is the loop's working storage
    }
    int n_assoc = 0, n_step = 0;
    const int tile_points = loop_tile_points();
    const dim3 kgrid(cdiv(max_ns, tile_points));
    const int lb = (int)kgrid.x;  // one partial row per tile, written by the association kernel
    const int fb = min(cdiv(max_ns, 256), 256);

    static const int cert_off = getenv("GS_CERT_OFF") != nullptr;
    // all hints and the camera given: grid search with its geometric proof (knn1_loop_k<true>), at every density;
    // GS_NO_GRID_SEARCH=1 / gs_set_grid_search(0) keep the chunk-box search for every association (same results; for
    // A/B measurements and tests)
    static const bool grid_off = getenv("GS_NO_GRID_SEARCH") != nullptr;
    const bool grid_search = !grid_off && g_grid_mode != 0 && hints.scan_points && hints.scan_orig && hints.src_pix && hints.pix_start &&
                             hints.cam_pose && hints.cam_K && hints.ds > 0 && hints.grid_w > 0 && hints.grid_h > 0;
    LoopConst lc{src, tgt, nrm, w.boxes, w.sboxes, d_ns, d_nt, trace, out_T, hints, gp, thresh, 0, 0, cert_off, tile_points,
                 grid_search ? 1 : 0, CamK{}, 0, w.cells, max_ns};
    hipLaunchKernelGGL(icp_prepare_k, dim3(cdiv(max_nt, SUPER * CHUNK)), dim3(SUPER * CHUNK), 0, st, w.S[0], init_T, damp,
                       hints.scan_points ? hints.scan_points : tgt, d_nt, w.boxes, w.sboxes, lc, w.lc, w.partials[0], w.partials[1], lb,
                       std::max(lb, 32 * RP_LOADS));
    GS_LAUNCH_CHECK(name);
    // The loop as a sequence  A S A S ... A S  (A = association + linearise launch, S = O(1) step on A's sums).
    // Every S but the last runs in the prologue of the A that follows it; state and partial sums alternate
    // between two buffers from launch to launch.
    int cur = 0;            // buffer the next launch READS its state / the previous sums from
    int pending = -1;       // step waiting to be folded into the next association
    int pending_slot = -1;  // slot the association before that step wrote (tape mode)
    // Folding pays while the association's blocks all run at once (latency-bound regime: the step's ~4 us ride in
    // every block instead of a ~4.5 us launch).  With more tiles than the chip holds (2 x 1024-thread blocks per CU)
    // the kernel is throughput-bound and 4 us of redundant work in EVERY block costs more than one small launch:
    // then each step is a launch of its own again (measured at 78 k source points: 1225 blocks).
    const bool fold = (int)kgrid.x <= 2 * 256;
    auto assoc = [&](int first) {
        if (!fold && pending >= 0) {  // stand-alone step, state updated in place
            hipLaunchKernelGGL(icp_step_k, dim3(1), dim3(1024), 0, st, w.S[cur], w.partials[cur], lb, pending, gp, trace, out_T,
                               pending_slot, tape ? tp.rec + (size_t)n_step * REC_WORDS : nullptr, 1, (const float *)nullptr,
                               (float *)nullptr);
            ++n_step;
            pending = -1;
        }
        const int nxt = pending >= 0 ? 1 - cur : cur;  // a folded step publishes the new state to the other buffer
        prof_mark(0, 0, st);
        float *rec_p = (tape && pending >= 0) ? tp.rec + (size_t)n_step * REC_WORDS : nullptr;
        const int nw = loop_waves(grid_search, max_nt, hints.grid_w * hints.grid_h);
        auto launch_nw = [&](auto kernel, int waves) {
            hipLaunchKernelGGL(kernel, kgrid, dim3(waves * 64), 0, st, (const LoopConst *)w.lc, (const IcpState *)w.S[cur], (const float *)w.partials[cur],
                               (const int32_t *)(w.cells + 2 * (size_t)max_ns), (const int32_t *)(w.cells + (size_t)(1 - (n_assoc & 1)) * max_ns),
                               max_ns, tile_points, first | ((n_assoc & 1) << 1), pending, pending_slot, lb, w.S[nxt], rec_p,
                               tape ? n_assoc : -1, w.B, w.partials[nxt], src);
        };
        auto launch = [&](auto k16, auto k8) {
            if (nw == 16) launch_nw(k16, 16); else launch_nw(k8, 8);
        };
        if (grid_search && lb <= 32 * RP_FEW) launch(knn1_loop_k<true, RP_FEW, 16>, knn1_loop_k<true, RP_FEW, 8>);
        else if (grid_search) launch(knn1_loop_k<true, RP_LOADS, 16>, knn1_loop_k<true, RP_LOADS, 8>);
        else launch(knn1_loop_k<false, RP_LOADS, 16>, knn1_loop_k<false, RP_LOADS, 8>);
        prof_mark(0, 1, st);
        if (pending >= 0) ++n_step;
        cur = nxt;
        pending = -1;
        ++n_assoc;
    };
    auto step = [&](int mode) {  // deferred: folded into the next association, or launched by finish()
        pending = mode;
        pending_slot = tape ? n_assoc - 1 : -1;
    };
    auto finish = [&]() {  // the loop's last step has no association behind it
        hipLaunchKernelGGL(icp_step_k, dim3(1), dim3(1024), 0, st, w.S[cur], w.partials[cur], lb, pending, gp, trace, out_T,
                           pending_slot, tape ? tp.rec + (size_t)n_step * REC_WORDS : nullptr, 0, compose_right, compose_out);
        ++n_step;
        pending = -1;
    };
    // NB with a folded step the sums it reduces are those of the launch before: partials[cur] at that time.
    // assoc() above passes w.partials[cur] (read) and w.partials[nxt] (write); without a pending step nothing is
    // read and cur == nxt is harmless.
    assoc(1);
    step(STEP_ADOPT);
    if (!grad) {
        // numiters + 1 associations instead of the reference's 2 x numiters: an accepted look-ahead
        // IS the next iteration's first linearisation, a rejected one leaves it unchanged.
        for (int it = 0; it < numiters; ++it) {
            assoc(0);
            step(STEP_LM);
        }
    } else {
        for (int it = 0; it < numiters; ++it) {
            assoc(0);            // look-ahead: pts[p_cur] . exp(xi)
            step(STEP_GRAD_B);   // dT = exp(sigma xi); look-ahead discarded
            if (it + 1 < numiters) {
                assoc(0);        // new current cloud: pts[p_cur] . exp(sigma xi)
                step(STEP_ADOPT);
            }
        }
    }
    finish();
    GS_LAUNCH_CHECK(name);
    if (best_last) {
        hipLaunchKernelGGL(copy_best_last_k, dim3(fb), dim3(256), 0, st, w.S[cur], w.B, d_ns, (unsigned long long *)best_last);
        GS_LAUNCH_CHECK(name);
    }
    return GS_OK;
}

// det: the target / normal adjoints by the deterministic fold (gs_detfold.hpp) -- reverse launch q (q = numiters - 1 - k for LM;
// 2 (numiters - 1 - k) and + 1 for gradLM's look / lin pair) stores its contributions in its own rows, the fold adds them up
static inline int bwd_launches(bool grad, int numiters) { return grad ? 2 * numiters : numiters; }
// the reverse pass's workspace and, behind it in det mode, the fold's: each taken as one piece and handed to its own layout
struct BwdDetWs {
    BwdWs bwd;
    DetWs det;
};
static inline size_t bwd_det_layout(bool det, bool grad, int max_ns, int max_nt, int numiters, void *ws, BwdDetWs *out) {
    Carve c{(char *)ws};
    BwdDetWs scratch, &w = out ? *out : scratch;
    bwd_ws_layout(max_ns, c.take(bwd_ws_layout(max_ns, nullptr, nullptr)), &w.bwd);
    w.det = DetWs{};
    if (det) {
        const int Q = bwd_launches(grad, numiters > 0 ? numiters : 1);
        det_ws_layout(Q, max_ns, max_nt, c.take(det_ws_layout(Q, max_ns, max_nt, nullptr, nullptr)), &w.det);
    }
    return c.off;
}

static int icp_backward_run(bool grad, const float *src, const int32_t *d_ns, int max_ns, const float *tgt, const float *nrm,
                            const int32_t *d_nt, int max_nt, const float *init_T, int numiters, float thresh, GradParams gp, const void *tape,
                            size_t tape_bytes, const float *grad_T, float *g_src, float *g_tgt, float *g_nrm, float *g_init_T,
                            void *ws, size_t ws_bytes, hipStream_t st, bool det = false) {
    const char *name = det ? "gs_icp_backward_det" : "gs_icp_backward";
    GS_REQUIRE(src && d_ns && tgt && nrm && d_nt && init_T && tape && grad_T && g_src && g_init_T, "%s: NULL argument", name);
    GS_REQUIRE(max_ns > 0 && max_nt > 0 && numiters >= 0, "%s: bad sizes", name);
    GS_REQUIRE(!det || bwd_launches(grad, numiters) <= 65535, "%s: too many iterations for the deterministic fold", name);
    BwdDetWs both;
    GS_REQUIRE_WS(name, ws, ws_bytes, bwd_det_layout(det, grad, max_ns, max_nt, numiters, ws, &both));
    Tape tp;
    GS_REQUIRE_TAPE(name, tape, tape_bytes, tape_layout(grad, max_ns, numiters, (void *)tape, &tp), GS_ERR_INVALID_ARG);
    const BwdWs &w = both.bwd;
    const DetWs &dw = both.det;
    const bool fold = det && (g_tgt || g_nrm);
    // what the walk's kernels scatter into: the outputs (float atomics) or, DET, launch q's contribution rows
    auto rows_of = [&](int q) { return fold ? dw.rows + (size_t)q * max_ns * DET_ROW : nullptr; };
    float *walk_nrm = det ? nullptr : g_nrm;
    const int nb = min(cdiv(max_ns, BWD_T), BWD_MAXB);
    int cur = 0;  // buffer the next launch READS its state / the previous sums from
    hipLaunchKernelGGL(bwd_begin_k, dim3(min(cdiv(3 * max(max_nt, max_ns), 256), 1024)), dim3(256), 0, st, w.S[0], grad_T, w.gP, 3 * max_ns,
                       w.partials[0], nb * 12, det ? nullptr : g_tgt, walk_nrm, d_nt, max_nt);
    for (int k = numiters - 1, q = 0; k >= 0; --k) {
        if (!grad) {
            const float *rec = tp.rec + (size_t)(1 + k) * REC_WORDS;
            float *gt = det ? rows_of(q++) : g_tgt;
            hipLaunchKernelGGL(det ? bwd_lin_k<true> : bwd_lin_k<false>, dim3(nb), dim3(BWD_T), 0, st, (const BwdState *)w.S[cur],
                               w.S[1 - cur], (int)FOLD_LM, rec, (const float *)w.partials[cur], nb, k, 1, tp.B, src, d_ns, tgt, nrm, thresh,
                               w.gP, gt, walk_nrm, w.partials[1 - cur]);
            cur = 1 - cur;
        } else {
            const float *rec = tp.rec + (size_t)(1 + 2 * k) * REC_WORDS;
            // slots of the gradLM loop are fixed: cloud k lives in slot 0 (k = 0) or 2k
            float *gt = det ? rows_of(q++) : g_tgt;
            hipLaunchKernelGGL(det ? bwd_look_k<true> : bwd_look_k<false>, dim3(nb), dim3(BWD_T), 0, st, (const BwdState *)w.S[cur],
                               w.S[1 - cur], rec, (const float *)w.partials[cur], nb, gp, k == 0 ? -1 : (k == 1 ? 0 : 2 * (k - 1)), tp.B, d_ns,
                               tgt, nrm, thresh, w.gP, gt, walk_nrm, w.partials[1 - cur]);
            cur = 1 - cur;
            gt = det ? rows_of(q++) : g_tgt;
            hipLaunchKernelGGL(det ? bwd_lin_k<true> : bwd_lin_k<false>, dim3(nb), dim3(BWD_T), 0, st, (const BwdState *)w.S[cur],
                               w.S[1 - cur], (int)FOLD_G2, rec, (const float *)w.partials[cur], nb, 0, 0, tp.B, src, d_ns, tgt, nrm, thresh,
                               w.gP, gt, walk_nrm, w.partials[1 - cur]);
            cur = 1 - cur;
        }
    }
    hipLaunchKernelGGL(bwd_finish_k, dim3(nb), dim3(BWD_T), 0, st, init_T, d_ns, (const float *)w.gP, g_src, (const BwdState *)w.S[cur],
                       (const float *)w.partials[cur], nb, g_init_T);
    GS_LAUNCH_CHECK(name);
    if (fold) return det_fold_run(dw, bwd_launches(grad, numiters), max_ns, d_ns, d_nt, max_nt, g_tgt, g_nrm, st, name);
    return GS_OK;
}

int icp_localize_run(int grad_lm, const float *src, const int32_t *d_ns, int max_ns, const float *tgt, const float *nrm,
                     const int32_t *d_nt, int max_nt, int numiters, float damp, float thresh, float lambda_max, float Bp,
                     float B2, float nu, const gs_icp_hints *hints, float *out_T, void *ws, size_t ws_bytes, hipStream_t st,
                     void *tape, size_t tape_bytes, const float *compose_right, float *compose_out) {
    const GradParams gp = grad_lm ? make_grad_params(lambda_max, Bp, B2, nu) : lm_grad_params();
    return icp_run(grad_lm != 0, src, d_ns, max_ns, tgt, nrm, d_nt, max_nt, nullptr, numiters, damp, thresh, gp, hints, out_T, nullptr,
                   nullptr, ws, ws_bytes, st, "gs_slam_localize/icp", tape, tape_bytes, compose_right, compose_out);
}

}  // namespace gs

using namespace gs;

extern "C" {

#ifdef GS_DIAG_STAMPS
int gs_diag_set_buffer(void *p) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_diag), &p, sizeof(p));
}
#endif

void gs_set_grid_search(int on) { g_grid_mode = on; }
void gs_set_tile_points(int n) { g_tile_points = n; }
int gs_set_loop_waves(int n) {
    if (n == 0 || n == 8 || n == 16) g_loop_waves = n;
    return g_loop_waves;
}
int gs_icp_launch_geometry(int max_ns, int have_hints, int *blocks, int *tile_points_dense, int *partial_rows) {
    GS_REQUIRE(max_ns > 0, "gs_icp_launch_geometry: max_ns must be positive");
    (void)have_hints;
    const int tp = loop_tile_points();
    if (blocks) *blocks = cdiv(max_ns, tp);
    if (tile_points_dense) *tile_points_dense = tp;
    if (partial_rows) *partial_rows = partial_rows_alloc(max_ns);
    return GS_OK;
}

int gs_loop_counts(unsigned int *out4, int reset) {
    GS_REQUIRE(out4, "gs_loop_counts: NULL argument");
    GS_HIP(hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_loop_counts), 16), "gs_loop_counts");  // synchronises with the device
    if (reset) {
        const unsigned int z[4] = {0, 0, 0, 0};
        GS_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_loop_counts), z, 16), "gs_loop_counts/reset");
    }
    return GS_OK;
}

int gs_window_counts(unsigned int *out4, int reset) {
    GS_REQUIRE(out4, "gs_window_counts: NULL argument");
    unsigned int stripes[WCOUNT_STRIPES][16];  // (4 KiB, local: the entry point holds no state of its own)
    GS_HIP(hipMemcpyFromSymbol(stripes, HIP_SYMBOL(g_window_counts), sizeof(stripes)), "gs_window_counts");  // synchronises with the device
    for (int k = 0; k < 4; ++k) {
        out4[k] = 0;
        for (int q = 0; q < WCOUNT_STRIPES; ++q) out4[k] += stripes[q][k];
    }
    if (reset) {
        for (int q = 0; q < WCOUNT_STRIPES; ++q)
            for (int k = 0; k < 16; ++k) stripes[q][k] = 0;
        GS_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_window_counts), stripes, sizeof(stripes)), "gs_window_counts/reset");
    }
    return GS_OK;
}

void gs_profile_enable(int on) {
    g_prof.on = on != 0;
    for (int t = 0; t < 2; ++t) { g_prof.used[t] = 0; g_prof.total_ms[t] = 0.0; g_prof.count[t] = 0; }
}

// Fold the events recorded so far into the totals (the caller must have synchronised the stream)
// and return, for tag 0 (association kernel) / 1 (linearise kernel), launches and total milliseconds.
int gs_profile_read(int tag, long *launches, double *total_ms) {
    GS_REQUIRE(tag == 0 || tag == 1, "gs_profile_read: tag must be 0 or 1");
    for (int t = 0; t < 2; ++t) {
        for (size_t i = 0; i < g_prof.used[t]; ++i) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, g_prof.ev[t][0][i], g_prof.ev[t][1][i]) == hipSuccess) {
                g_prof.total_ms[t] += ms;
                g_prof.count[t] += 1;
            }
        }
        g_prof.used[t] = 0;
    }
    if (launches) *launches = g_prof.count[tag];
    if (total_ms) *total_ms = g_prof.total_ms[tag];
    return GS_OK;
}

size_t gs_knn1_ws_bytes(int max_nt) { return one_piece_bytes(boxes_bytes(max_nt)); }

int gs_knn1(const float *src, const int32_t *d_ns, int max_ns, const float *tgt, const int32_t *d_nt, int max_nt,
            uint64_t *best, void *ws, size_t ws_bytes, gs_stream_t stream) {
    GS_REQUIRE(src && d_ns && tgt && d_nt && best, "gs_knn1: NULL argument");
    GS_REQUIRE(max_ns >= 0 && max_nt >= 0, "gs_knn1: negative size");
    if (max_ns == 0) return GS_OK;
    hipStream_t st = (hipStream_t)stream;
    if (max_nt == 0) {
        hipLaunchKernelGGL(fill_u64_k, dim3(min(cdiv(max_ns, 256), 1024)), dim3(256), 0, st, (unsigned long long *)best, max_ns, KEY_NONE);
        GS_LAUNCH_CHECK("gs_knn1/fill");
        return GS_OK;
    }
    GS_REQUIRE_WS("gs_knn1", ws, ws_bytes, gs_knn1_ws_bytes(max_nt));
    hipLaunchKernelGGL(tgt_boxes_k, dim3(cdiv(max_nt, 64)), dim3(64), 0, st, tgt, d_nt, (float *)ws);
    GS_LAUNCH_CHECK("gs_knn1/boxes");
    hipLaunchKernelGGL(knn1_box_k, dim3(cdiv(max_ns, 64)), dim3(KNN_BT), 0, st, src, d_ns, tgt, (const float *)ws, d_nt,
                       (unsigned long long *)best);
    GS_LAUNCH_CHECK("gs_knn1");
    return GS_OK;
}

int gs_knn1_bruteforce(const float *src, const int32_t *d_ns, int max_ns, const float *tgt, const int32_t *d_nt,
                       int max_nt, uint64_t *best, gs_stream_t stream) {
    GS_REQUIRE(src && d_ns && tgt && d_nt && best, "gs_knn1_bruteforce: NULL argument");
    GS_REQUIRE(max_ns >= 0 && max_nt >= 0, "gs_knn1_bruteforce: negative size");
    if (max_ns == 0) return GS_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(fill_u64_k, dim3(min(cdiv(max_ns, 256), 1024)), dim3(256), 0, st, (unsigned long long *)best, max_ns, KEY_NONE);
    GS_LAUNCH_CHECK("gs_knn1_bruteforce/fill");
    if (max_nt == 0) return GS_OK;
    const int nsplit = knn_nsplit_brute(max_ns, max_nt);
    hipLaunchKernelGGL(knn1_brute_k, dim3(cdiv(max_ns, KNN_T), nsplit), dim3(KNN_T), 0, st, src, d_ns, tgt, d_nt, nsplit,
                       (unsigned long long *)best);
    GS_LAUNCH_CHECK("gs_knn1_bruteforce");
    return GS_OK;
}

int gs_knn1_unpack(const uint64_t *best, const int32_t *d_ns, int max_ns, float *dist2, int64_t *idx, gs_stream_t stream) {
    GS_REQUIRE(best && d_ns && max_ns >= 0, "gs_knn1_unpack: bad arguments");
    if (max_ns == 0) return GS_OK;
    hipLaunchKernelGGL(knn_unpack_k, dim3(min(cdiv(max_ns, 256), 1024)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned long long *)best, d_ns, dist2, idx);
    GS_LAUNCH_CHECK("gs_knn1_unpack");
    return GS_OK;
}

size_t gs_icp_linearize_ws_bytes(int max_ns) { (void)max_ns; return one_piece_bytes((size_t)LIN_MAXB * NACC * 4); }

int gs_icp_linearize(const float *src, const int32_t *d_ns, int max_ns, const float *tgt, const float *tgt_normals,
                     const uint64_t *best, float dist_thresh, float *out44, void *ws, size_t ws_bytes,
                     gs_stream_t stream) {
    GS_REQUIRE(src && d_ns && tgt && tgt_normals && best && out44, "gs_icp_linearize: NULL argument");
    GS_REQUIRE(max_ns >= 0, "gs_icp_linearize: negative size");
    GS_REQUIRE_WS("gs_icp_linearize", ws, ws_bytes, gs_icp_linearize_ws_bytes(max_ns));
    hipStream_t st = (hipStream_t)stream;
    const int nb = lin_blocks(max_ns);  // capped at LIN_MAXB: large clouds grid-stride
    hipLaunchKernelGGL(linearize_k, dim3(nb), dim3(LIN_T), 0, st, src, d_ns, tgt, tgt_normals,
                       (const unsigned long long *)best, dist_thresh, (float *)ws);
    GS_LAUNCH_CHECK("gs_icp_linearize");
    hipLaunchKernelGGL(finalize44_k, dim3(1), dim3(1024), 0, st, (const float *)ws, nb, out44);
    GS_LAUNCH_CHECK("gs_icp_linearize/finalize");
    return GS_OK;
}

int gs_icp_rows(const float *src, const int32_t *d_ns, int max_ns, const float *tgt, const float *tgt_normals,
                const uint64_t *best, float dist_thresh, float *A, float *b, uint8_t *keep, gs_stream_t stream) {
    GS_REQUIRE(src && d_ns && tgt && tgt_normals && best && A && b && keep, "gs_icp_rows: NULL argument");
    if (max_ns <= 0) return GS_OK;
    hipLaunchKernelGGL(icp_rows_k, dim3(min(cdiv(max_ns, 256), 2048)), dim3(256), 0, (hipStream_t)stream, src, d_ns, tgt,
                       tgt_normals, (const unsigned long long *)best, dist_thresh, A, b, keep);
    GS_LAUNCH_CHECK("gs_icp_rows");
    return GS_OK;
}

int gs_icp_linearize_backward(const float *src, const int32_t *d_ns, int max_ns, const float *tgt,
                              const float *tgt_normals, const uint64_t *best, float dist_thresh, const float *g_out43,
                              float *g_src, float *g_tgt, float *g_normals, gs_stream_t stream) {
    GS_REQUIRE(src && d_ns && tgt && tgt_normals && best && g_out43, "gs_icp_linearize_backward: NULL argument");
    if (max_ns <= 0) return GS_OK;
    hipLaunchKernelGGL(linearize_bwd_k<false>, dim3(min(cdiv(max_ns, 256), 2048)), dim3(256), 0, (hipStream_t)stream, src, d_ns,
                       tgt, tgt_normals, (const unsigned long long *)best, dist_thresh, g_out43, g_src, g_tgt, g_normals);
    GS_LAUNCH_CHECK("gs_icp_linearize_backward");
    return GS_OK;
}

size_t gs_icp_linearize_backward_det_ws_bytes(int max_ns, int max_nt) {
    return det_ws_layout(1, max_ns > 0 ? max_ns : 1, max_nt > 0 ? max_nt : 1, nullptr, nullptr);
}

int gs_icp_linearize_backward_det(const float *src, const int32_t *d_ns, int max_ns, const float *tgt, const float *tgt_normals,
                                  const int32_t *d_nt, int max_nt, const uint64_t *best, float dist_thresh, const float *g_out43,
                                  float *g_src, float *g_tgt, float *g_normals, void *ws, size_t ws_bytes, gs_stream_t stream) {
    const char *name = "gs_icp_linearize_backward_det";
    GS_REQUIRE(src && d_ns && tgt && tgt_normals && d_nt && best && g_out43, "%s: NULL argument", name);
    if (max_ns <= 0) return GS_OK;
    GS_REQUIRE(max_nt > 0, "%s: bad sizes", name);
    DetWs dw;
    GS_REQUIRE_WS(name, ws, ws_bytes, det_ws_layout(1, max_ns, max_nt, ws, &dw));
    hipStream_t st = (hipStream_t)stream;
    const bool fold = g_tgt || g_normals;
    hipLaunchKernelGGL(linearize_bwd_k<true>, dim3(min(cdiv(max_ns, 256), 2048)), dim3(256), 0, st, src, d_ns, tgt, tgt_normals,
                       (const unsigned long long *)best, dist_thresh, g_out43, g_src, fold ? dw.rows : nullptr, nullptr);
    GS_LAUNCH_CHECK(name);
    if (fold) return det_fold_run(dw, 1, max_ns, d_ns, d_nt, max_nt, g_tgt, g_normals, st, name);
    return GS_OK;
}

int gs_transform_points(const float *pts, const int32_t *d_n, int max_n, const float *T, float *out, gs_stream_t stream) {
    GS_REQUIRE(pts && d_n && T && out && max_n >= 0, "gs_transform_points: bad arguments");
    if (max_n == 0) return GS_OK;
    hipLaunchKernelGGL(transform_k, dim3(min(cdiv(max_n, 256), 2048)), dim3(256), 0, (hipStream_t)stream, pts, d_n, T, out);
    GS_LAUNCH_CHECK("gs_transform_points");
    return GS_OK;
}

size_t gs_icp_ws_bytes(int max_ns, int max_nt) {
    return icp_ws_layout(max_ns > 0 ? max_ns : 1, max_nt > 0 ? max_nt : 1, nullptr, nullptr);
}

int gs_icp_point_to_plane(const float *src, const int32_t *d_ns, int max_ns, const float *tgt, const float *tgt_normals,
                          const int32_t *d_nt, int max_nt, const float *init_T, int numiters, float damp,
                          float dist_thresh, const gs_icp_hints *hints, float *out_T, uint64_t *best_last, float *trace,
                          void *ws, size_t ws_bytes, gs_stream_t stream) {
    return icp_run(false, src, d_ns, max_ns, tgt, tgt_normals, d_nt, max_nt, init_T, numiters, damp, dist_thresh,
                   lm_grad_params(), hints, out_T, best_last, trace, ws, ws_bytes, (hipStream_t)stream,
                   "gs_icp_point_to_plane");
}

int gs_icp_point_to_plane_grad(const float *src, const int32_t *d_ns, int max_ns, const float *tgt,
                               const float *tgt_normals, const int32_t *d_nt, int max_nt, const float *init_T,
                               int numiters, float damp, float dist_thresh, float lambda_max, float B, float B2, float nu,
                               const gs_icp_hints *hints, float *out_T, uint64_t *best_last, float *trace, void *ws,
                               size_t ws_bytes, gs_stream_t stream) {
    return icp_run(true, src, d_ns, max_ns, tgt, tgt_normals, d_nt, max_nt, init_T, numiters, damp, dist_thresh,
                   make_grad_params(lambda_max, B, B2, nu), hints, out_T, best_last, trace, ws, ws_bytes,
                   (hipStream_t)stream, "gs_icp_point_to_plane_grad");
}

size_t gs_icp_tape_bytes(int max_ns, int numiters, int grad_lm) {
    return tape_layout(grad_lm != 0, max_ns > 0 ? max_ns : 1, numiters, nullptr, nullptr);
}

int gs_icp_point_to_plane_taped(const float *src, const int32_t *d_ns, int max_ns, const float *tgt, const float *tgt_normals,
                                const int32_t *d_nt, int max_nt, const float *init_T, int numiters, float damp,
                                float dist_thresh, int grad_lm, float lambda_max, float B, float B2, float nu,
                                const gs_icp_hints *hints, float *out_T, uint64_t *best_last, void *tape, size_t tape_bytes,
                                void *ws, size_t ws_bytes, gs_stream_t stream) {
    GS_REQUIRE(tape, "gs_icp_point_to_plane_taped: NULL tape");
    return icp_run(grad_lm != 0, src, d_ns, max_ns, tgt, tgt_normals, d_nt, max_nt, init_T, numiters, damp, dist_thresh,
                   grad_lm ? make_grad_params(lambda_max, B, B2, nu) : lm_grad_params(), hints, out_T,
                   best_last, nullptr, ws, ws_bytes, (hipStream_t)stream, "gs_icp_point_to_plane_taped", tape, tape_bytes);
}

size_t gs_icp_backward_ws_bytes(int max_ns) { return bwd_det_layout(false, false, max_ns > 0 ? max_ns : 1, 1, 1, nullptr, nullptr); }

size_t gs_icp_backward_det_ws_bytes(int max_ns, int max_nt, int numiters, int grad_lm) {
    return bwd_det_layout(true, grad_lm != 0, max_ns > 0 ? max_ns : 1, max_nt > 0 ? max_nt : 1, numiters, nullptr, nullptr);
}

static int icp_backward_entry(bool det, const float *src, const int32_t *d_ns, int max_ns, const float *tgt, const float *tgt_normals,
                              const int32_t *d_nt, int max_nt, const float *init_T, int numiters, float dist_thresh, int grad_lm,
                              float lambda_max, float B, float B2, float nu, const void *tape, size_t tape_bytes,
                              const float *grad_T, float *grad_src, float *grad_tgt, float *grad_normals,
                              float *grad_init_T, void *ws, size_t ws_bytes, gs_stream_t stream) {
    if (numiters == 0) {  // T = init_T, nothing else depends on the inputs (no scatter: the same in both modes)
        GS_REQUIRE(grad_T && grad_src && grad_init_T && d_nt && max_ns > 0 && max_nt > 0, "gs_icp_point_to_plane_backward: bad arguments");
        hipStream_t st = (hipStream_t)stream;
        GS_HIP(hipMemsetAsync(grad_src, 0, (size_t)max_ns * 12, st), "gs_icp_point_to_plane_backward");
        if (grad_tgt || grad_normals)
            hipLaunchKernelGGL(zero_rows_k, dim3(min(cdiv(3 * max_nt, 256), 1024)), dim3(256), 0, st, grad_tgt, grad_normals, d_nt, max_nt);
        GS_HIP(hipMemcpyAsync(grad_init_T, grad_T, 64, hipMemcpyDeviceToDevice, st), "gs_icp_point_to_plane_backward");
        return GS_OK;
    }
    return icp_backward_run(grad_lm != 0, src, d_ns, max_ns, tgt, tgt_normals, d_nt, max_nt, init_T, numiters, dist_thresh,
                            grad_lm ? make_grad_params(lambda_max, B, B2, nu) : lm_grad_params(), tape,
                            tape_bytes, grad_T, grad_src, grad_tgt, grad_normals, grad_init_T, ws, ws_bytes, (hipStream_t)stream, det);
}

int gs_icp_point_to_plane_backward(const float *src, const int32_t *d_ns, int max_ns, const float *tgt, const float *tgt_normals,
                                   const int32_t *d_nt, int max_nt, const float *init_T, int numiters, float dist_thresh, int grad_lm,
                                   float lambda_max, float B, float B2, float nu, const void *tape, size_t tape_bytes,
                                   const float *grad_T, float *grad_src, float *grad_tgt, float *grad_normals,
                                   float *grad_init_T, void *ws, size_t ws_bytes, gs_stream_t stream) {
    return icp_backward_entry(false, src, d_ns, max_ns, tgt, tgt_normals, d_nt, max_nt, init_T, numiters, dist_thresh, grad_lm, lambda_max,
                              B, B2, nu, tape, tape_bytes, grad_T, grad_src, grad_tgt, grad_normals, grad_init_T, ws, ws_bytes, stream);
}

int gs_icp_point_to_plane_backward_det(const float *src, const int32_t *d_ns, int max_ns, const float *tgt, const float *tgt_normals,
                                       const int32_t *d_nt, int max_nt, const float *init_T, int numiters, float dist_thresh, int grad_lm,
                                       float lambda_max, float B, float B2, float nu, const void *tape, size_t tape_bytes,
                                       const float *grad_T, float *grad_src, float *grad_tgt, float *grad_normals,
                                       float *grad_init_T, void *ws, size_t ws_bytes, gs_stream_t stream) {
    return icp_backward_entry(true, src, d_ns, max_ns, tgt, tgt_normals, d_nt, max_nt, init_T, numiters, dist_thresh, grad_lm, lambda_max,
                              B, B2, nu, tape, tape_bytes, grad_T, grad_src, grad_tgt, grad_normals, grad_init_T, ws, ws_bytes, stream);
}

}  // extern "C"

// The map metrics' deterministic scatter shares gs_detfold.hpp's kernels with the reverse passes above; it comes last, so the
// kernels above are emitted as before.
#include "gs_metrics_det.hpp"
