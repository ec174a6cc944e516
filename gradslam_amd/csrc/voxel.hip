// libgradslam_hip -- voxel downsampling (V): one output row per occupied voxel, holding the exact sum or mean of its members.
//
//   A  gs_voxel_assign: which voxel every row belongs to.  A hash grid per batch element (open addressing, linear probing,
//      load <= 0.5), not a sort and not a dense grid:
//        vox_init_k     table := empty; voxel_count := 0, voxel_first := -1, n_dropped := 0, error word := 0
//        vox_insert_k   key of every row (vox_key: the rule); 64-bit atomicCAS claims the key's slot, atomicMin leaves the lowest
//                       member row in the slot's row word; the row's slot is kept (4 B per row) so that nothing probes twice
//        vox_count_k  } the stable compaction of gs_compact.hpp over the LEADERS (rows that are their slot's lowest member):
//       [vox_scan_k]  } leaders are numbered in row order, which is the order of first appearance; the leader's number goes to
//        vox_write_k  } voxel_of[leader], its row to voxel_first[number]; the total is n_voxels
//        vox_finish_k   every other row copies its leader's number; members are counted (one integer atomic per run of lanes
//                       that share a voxel)
//      The numbering is a property of the input alone: it depends on the lowest member row of every voxel, which atomicMin
//      finds whatever the arrival order, never on which slot a key landed in.
//   R  gs_voxel_reduce: the exact fold of gs_fixed128.hpp (the rule is stated there) over the members of every voxel:
//        (memset)       the fold's workspace := 0
//        vred_max_k     the max pass over the members
//        vred_acc_k     the accumulate pass, one lane per row: runs of lanes that share a voxel are summed in registers first
//                       (integer addition is associative: same bits) and the run's first lane adds the total
//        vred_finish_k  per (voxel, component): the fold's result, divided by float(count) in mean mode; rows beyond
//                       n_voxels := 0
//      gs_voxel_reduce_backward: one gather launch.
// Every probe loop is bounded by the table size; nothing spins, nothing is handed from one workgroup to another inside a launch,
// nothing synchronises the host.  Batch elements ride in grid.y, rows in grid.x.
#include <cmath>
#include <stddef.h>

#include <algorithm>

#include "gs_compact.hpp"
#include "gs_fixed128.hpp"
#include "gs_voxel.hpp"

namespace gs {

struct VoxIn {
    const float *pts;        // (B, N, 3)
    const int32_t *counts;   // (B,)
    int N;
    float v;
    f3 o;
};
__device__ __forceinline__ int vox_count(const int32_t *__restrict__ counts, int b, int N) { return min(max(counts[b], 0), N); }

// Runs of consecutive lanes with equal `m`: is this lane the first of its run, and which lane is the run's last.
__device__ __forceinline__ bool wave_run(int m, int lane, int &end, unsigned long long &heads) {
    const int prev = __shfl_up(m, 1, kWave);
    const bool head = lane == 0 || prev != m;
    heads = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    end = above ? lane + __ffsll((long long)above) - 1 : 63;
    return head;
}

// ------------------------------------------------------------------ A: assignment.  grid (x: rows / slots, y: batch element)
__global__ __launch_bounds__(VOX_T) void vox_init_k(VoxWs w, int N, int32_t *__restrict__ n_voxels, int32_t *__restrict__ n_dropped,
                                                    int32_t *__restrict__ voxel_count, int32_t *__restrict__ voxel_first) {
    const int b = blockIdx.y;
    const int64_t tid = (int64_t)blockIdx.x * VOX_T + threadIdx.x, stride = (int64_t)gridDim.x * VOX_T;
    unsigned long long *keys = w.keys + (int64_t)b * w.S;
    uint32_t *rows = w.rows + (int64_t)b * w.S;
    for (int64_t s = tid; s < w.S; s += stride) {
        keys[s] = VOX_EMPTY;
        rows[s] = 0xffffffffu;
    }
    for (int64_t i = tid; i < N; i += stride) {
        voxel_count[(int64_t)b * N + i] = 0;
        voxel_first[(int64_t)b * N + i] = -1;
    }
    if (tid == 0) {
        n_voxels[b] = 0;
        n_dropped[b] = 0;
        if (b == 0) *w.err = 0;
    }
}

__global__ __launch_bounds__(VOX_T) void vox_insert_k(VoxIn in, VoxWs w, int32_t *__restrict__ n_dropped) {
    const int b = blockIdx.y, N = in.N, n = vox_count(in.counts, b, N);
    const float *pts = in.pts + (int64_t)b * N * 3;
    unsigned long long *keys = w.keys + (int64_t)b * w.S;
    uint32_t *rows = w.rows + (int64_t)b * w.S;
    int32_t *slot = w.slot + (int64_t)b * N;
    const uint32_t mask = (uint32_t)(w.S - 1);
    for (int64_t i0 = (int64_t)blockIdx.x * VOX_T; i0 < N; i0 += (int64_t)gridDim.x * VOX_T) {  // (block-uniform trip count)
        const int64_t i = i0 + threadIdx.x;
        if (i0 >= n) {  // padding only
            if (i < N) slot[i] = -1;
            continue;
        }
        int s = -1;
        bool dropped = false;
        if (i < n) {
            unsigned long long key = 0;
            if (vox_key(ld3(pts, i), in.o, in.v, key)) {
                uint32_t h = vox_hash(key, mask);
                for (int64_t t = 0; t < w.S; ++t) {  // bounded: at load <= 0.5 a free slot or the key is met long before
                    unsigned long long cur = keys[h];  // (a key never changes once set: only a stale EMPTY can be read, and the CAS decides)
                    if (cur == VOX_EMPTY) cur = atomicCAS(keys + h, VOX_EMPTY, key);
                    if (cur == VOX_EMPTY || cur == key) {
                        s = (int)h;
                        break;
                    }
                    h = (h + 1) & mask;
                }
                if (s >= 0) atomicMin(rows + s, (uint32_t)i);
                else atomicExch(w.err, 1);
            } else {
                dropped = true;
                s = -2;
            }
        }
        if (i < N) slot[i] = s;
        const unsigned long long d = __ballot(dropped);
        if ((threadIdx.x & 63) == 0 && d) atomicAdd(n_dropped + b, __popcll(d));
    }
}

struct VoxLeader {  // the compaction's predicate: the row is the lowest member of its voxel
    const int32_t *slot;
    const uint32_t *rows;
    __device__ bool operator()(int64_t i) const {
        const int s = slot[i];
        return s >= 0 && rows[s] == (uint32_t)i;
    }
};
struct VoxNumber {  // the compaction's writer: leader i is voxel `pos`
    int32_t *voxel_of, *voxel_first;
    __device__ void operator()(int64_t i, int64_t pos) const {
        voxel_of[i] = (int32_t)pos;
        voxel_first[pos] = (int32_t)i;
    }
};

// grid (x: compaction blocks, y: batch element)
__global__ __launch_bounds__(kCT) void vox_count_k(VoxWs w, int N) {
    const int b = blockIdx.y;
    const VoxLeader pred{w.slot + (int64_t)b * N, w.rows + (int64_t)b * w.S};
    compact_count_body((int64_t)N, pred, w.bcount + (int64_t)b * w.nb, (unsigned char *)nullptr, (int)blockIdx.x, w.nb);
}

// grid (x: batch element), one block each: exclusive scan of the batch element's block counts; the total is n_voxels
__global__ __launch_bounds__(1024) void vox_scan_k(VoxWs w, int32_t *__restrict__ n_voxels) {
    const int b = blockIdx.x;
    compact_scan_body(w.bcount + (int64_t)b * w.nb, w.nb, w.boffset + (int64_t)b * w.nb, (int *)(n_voxels + b));
}

template <bool SelfScan>
__global__ __launch_bounds__(kCT) void vox_write_k(VoxWs w, int N, int32_t *__restrict__ voxel_of, int32_t *__restrict__ voxel_first,
                                                   int32_t *__restrict__ n_voxels) {
    const int b = blockIdx.y;
    const VoxLeader pred{w.slot + (int64_t)b * N, w.rows + (int64_t)b * w.S};
    const VoxNumber writer{voxel_of + (int64_t)b * N, voxel_first + (int64_t)b * N};
    const int *blocks = (SelfScan ? w.bcount : w.boffset) + (int64_t)b * w.nb;
    compact_write_body<VoxLeader, VoxNumber, SelfScan>((int64_t)N, pred, writer, blocks, SelfScan ? (int *)(n_voxels + b) : (int *)nullptr,
                                                       (const unsigned char *)nullptr, (int)blockIdx.x, w.nb);
}

// voxel_of of every row that is not a leader (leaders hold theirs since vox_write_k: this kernel reads leaders' entries only and
// writes the others' only), and the members per voxel.  A failed insertion (error word) is reported as n_voxels = -1.
__global__ __launch_bounds__(VOX_T) void vox_finish_k(VoxWs w, int N, int32_t *voxel_of, int32_t *__restrict__ voxel_count,
                                                      int32_t *__restrict__ n_voxels) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int32_t *slot = w.slot + (int64_t)b * N;
    const uint32_t *rows = w.rows + (int64_t)b * w.S;
    int32_t *vof = voxel_of + (int64_t)b * N;
    int32_t *cnt = voxel_count + (int64_t)b * N;
    if (blockIdx.x == 0 && threadIdx.x == 0 && *w.err) n_voxels[b] = -1;
    for (int64_t i0 = (int64_t)blockIdx.x * VOX_T; i0 < N; i0 += (int64_t)gridDim.x * VOX_T) {
        const int64_t i = i0 + threadIdx.x;
        int m = -1;
        if (i < N) {
            const int s = slot[i];
            if (s >= 0) {
                const uint32_t leader = rows[s];
                m = leader < (uint32_t)N ? vof[leader] : -1;
                if ((int64_t)leader != i) vof[i] = m;
            } else {
                vof[i] = -1;
            }
        }
        int end;
        unsigned long long heads;
        const bool head = wave_run(m, lane, end, heads);
        if (head && m >= 0 && m < N) atomicAdd(cnt + m, end - lane + 1);
    }
}

// ------------------------------------------------------------------ R: reduction.  grid (x: rows, y: batch element)
struct VredIn {
    const float *x;            // (B, N, C)
    const int32_t *counts;     // (B,)
    const int32_t *voxel_of;   // (B, N)
    const int32_t *n_voxels;   // (B,)
    const int32_t *voxel_count;  // (B, N)
    int N, C, M;               // M = M_max: rows of out / the accumulators per batch element
};
__device__ __forceinline__ int vred_nvox(const VredIn &in, int b) { return min(max(in.n_voxels[b], 0), in.M); }

__global__ __launch_bounds__(VOX_T) void vred_max_k(VredIn in, Fold f) {
    const int b = blockIdx.y, n = vox_count(in.counts, b, in.N), nv = vred_nvox(in, b);
    const float *x = in.x + (int64_t)b * in.N * in.C;
    const int32_t *vof = in.voxel_of + (int64_t)b * in.N;
    const int64_t total = (int64_t)n * in.C;
    uint32_t mx = 0;
    for (int64_t e = (int64_t)blockIdx.x * VOX_T + threadIdx.x; e < total; e += (int64_t)gridDim.x * VOX_T) {
        const uint32_t u = fold_max(mx, x[e]);
        if (u != mx && (uint32_t)vof[e / in.C] < (uint32_t)nv) mx = u;  // (the voxel is looked up for a new maximum only)
    }
    fold_max_commit(f.maxbits, mx);
}

// PREAGG: runs of lanes that share a voxel are summed in registers and the run's first lane adds the total
template <bool PREAGG>
__global__ __launch_bounds__(VOX_T) void vred_acc_k(VredIn in, Fold f, int lg) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, C = in.C;
    const int n = vox_count(in.counts, b, in.N), nv = vred_nvox(in, b);
    const int E = det_scale(*f.maxbits, lg);
    const uint32_t *x = reinterpret_cast<const uint32_t *>(in.x) + (int64_t)b * in.N * C;
    const int32_t *vof = in.voxel_of + (int64_t)b * in.N;
    const int64_t row0 = (int64_t)b * in.M;
    for (int64_t i0 = (int64_t)blockIdx.x * VOX_T; i0 < n; i0 += (int64_t)gridDim.x * VOX_T) {  // (block-uniform trip count)
        const int64_t i = i0 + threadIdx.x;
        int m = i < n ? vof[i] : -1;
        if ((uint32_t)m >= (uint32_t)nv) m = -1;
        int end = lane;
        unsigned long long heads = ~0ull;
        bool head = true;
        if (PREAGG) head = wave_run(m, lane, end, heads);
        const bool lone = heads == ~0ull;  // wave-uniform: every run is one lane long, nothing to add up
        for (int c = 0; c < C; ++c) {
            __int128 v = 0;
            if (m >= 0) {
                const uint32_t bits = x[i * C + c];
                if (fold_finite(f, row0 + m, c, bits)) v = det_to_fixed(bits, E);
            }
            unsigned long long lo = (unsigned long long)v, hi = (unsigned long long)(v >> 64);
            if (PREAGG && !lone) {
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {  // segmented sum: lane l ends with the sum of [l, end]
                    const unsigned long long olo = __shfl_down(lo, off, kWave), ohi = __shfl_down(hi, off, kWave);
                    if (lane + off <= end) {
                        const unsigned long long s = lo + olo;
                        hi += ohi + (s < lo ? 1ull : 0ull);
                        lo = s;
                    }
                }
            }
            if (head && m >= 0) fold_add_words(fold_sum(f, row0 + m, c), lo, hi);
        }
    }
}

// grid (x: elements of out, y: batch element): every element of out is written
__global__ __launch_bounds__(VOX_T) void vred_finish_k(VredIn in, Fold f, int lg, int mean, float *__restrict__ out) {
    const int b = blockIdx.y, C = in.C, nv = vred_nvox(in, b);
    const int E = det_scale(*f.maxbits, lg);
    const int32_t *cnt = in.voxel_count + (int64_t)b * in.N;
    float *o = out + (int64_t)b * in.M * C;
    const int64_t total = (int64_t)in.M * C, row0 = (int64_t)b * in.M;
    for (int64_t t = (int64_t)blockIdx.x * VOX_T + threadIdx.x; t < total; t += (int64_t)gridDim.x * VOX_T) {
        const int m = (int)(t / C), c = (int)(t - (int64_t)m * C);
        float r = 0.0f;
        if (m < nv) {
            r = fold_result(f, row0 + m, c, E);
            if (mean) r = r / (float)cnt[m];
        }
        o[t] = r;
    }
}

// grid (x: elements of g_x, y: batch element): every element of g_x is written
__global__ __launch_bounds__(VOX_T) void vred_bwd_k(const float *__restrict__ g_out, VredIn in, int mean, float *__restrict__ g_x) {
    const int b = blockIdx.y, C = in.C, n = vox_count(in.counts, b, in.N);
    const int32_t *vof = in.voxel_of + (int64_t)b * in.N;
    const int32_t *cnt = in.voxel_count + (int64_t)b * in.N;
    const float *go = g_out + (int64_t)b * in.M * C;
    float *gx = g_x + (int64_t)b * in.N * C;
    const int64_t total = (int64_t)in.N * C;
    for (int64_t t = (int64_t)blockIdx.x * VOX_T + threadIdx.x; t < total; t += (int64_t)gridDim.x * VOX_T) {
        const int64_t i = t / C;
        const int c = (int)(t - i * C);
        float r = 0.0f;
        if (i < n) {
            const int m = vof[i];
            if ((uint32_t)m < (uint32_t)in.M) {
                r = go[(int64_t)m * C + c];
                if (mean) r = r / (float)cnt[m];
            }
        }
        gx[t] = r;
    }
}

static inline bool vox_shape_ok(int B, int N_max) { return B > 0 && B <= 65535 && N_max > 0 && N_max <= VOX_NMAX; }
static inline bool vred_shape_ok(int B, int N_max, int C, int M_max) {
    return vox_shape_ok(B, N_max) && C >= 1 && C <= VOX_CMAX && M_max > 0 && M_max <= N_max;
}

}  // namespace gs

using namespace gs;

extern "C" {

size_t gs_voxel_assign_ws_bytes(int B, int N_max) {
    if (!vox_shape_ok(B, N_max)) return 0;
    return vox_assign_layout(B, N_max, nullptr, nullptr);
}

int gs_voxel_assign(const float *points, const int32_t *counts, int N_max, int B, float voxel_size, const float *origin,
                    int32_t *voxel_of, int32_t *n_voxels, int32_t *n_dropped, int32_t *voxel_count, int32_t *voxel_first, void *ws,
                    size_t ws_bytes, gs_stream_t stream) {
    GS_REQUIRE(points && counts && origin && voxel_of && n_voxels && n_dropped && voxel_count && voxel_first,
               "gs_voxel_assign: NULL argument");
    GS_REQUIRE(vox_shape_ok(B, N_max), "gs_voxel_assign: bad shape B=%d N_max=%d (N_max <= 2^29)", B, N_max);
    GS_REQUIRE(voxel_size > 0.0f && voxel_size < INFINITY, "gs_voxel_assign: voxel_size must be finite and positive, got %g",
               (double)voxel_size);
    GS_REQUIRE(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]), "gs_voxel_assign: origin must be finite");
    GS_REQUIRE_WS("gs_voxel_assign", ws, ws_bytes, gs_voxel_assign_ws_bytes(B, N_max));
    hipStream_t st = (hipStream_t)stream;
    VoxWs w;
    vox_assign_layout(B, N_max, ws, &w);
    const VoxIn in{points, counts, N_max, voxel_size, f3{origin[0], origin[1], origin[2]}};
    const dim3 rows(rows_grid(N_max, VOX_T, 4096), B);
    hipLaunchKernelGGL(vox_init_k, dim3(rows_grid(w.S, VOX_T, 4096), B), dim3(VOX_T), 0, st, w, N_max, n_voxels, n_dropped, voxel_count, voxel_first);
    hipLaunchKernelGGL(vox_insert_k, rows, dim3(VOX_T), 0, st, in, w, n_dropped);
    GS_LAUNCH_CHECK("gs_voxel_assign/insert");
    hipLaunchKernelGGL(vox_count_k, dim3(w.nb, B), dim3(kCT), 0, st, w, N_max);
    if (w.nb <= kSelfScanBlocks) {
        hipLaunchKernelGGL(vox_write_k<true>, dim3(w.nb, B), dim3(kCT), 0, st, w, N_max, voxel_of, voxel_first, n_voxels);
    } else {
        hipLaunchKernelGGL(vox_scan_k, dim3(B), dim3(1024), 0, st, w, n_voxels);
        hipLaunchKernelGGL((vox_write_k<false>), dim3(w.nb, B), dim3(kCT), 0, st, w, N_max, voxel_of, voxel_first, n_voxels);
    }
    GS_LAUNCH_CHECK("gs_voxel_assign/number");
    hipLaunchKernelGGL(vox_finish_k, rows, dim3(VOX_T), 0, st, w, N_max, voxel_of, voxel_count, n_voxels);
    GS_LAUNCH_CHECK("gs_voxel_assign/finish");
    return GS_OK;
}

size_t gs_voxel_reduce_ws_bytes(int B, int M_max, int C) {
    if (B <= 0 || B > 65535 || M_max <= 0 || M_max > VOX_NMAX || C < 1 || C > VOX_CMAX) return 0;
    return vox_reduce_layout(B, M_max, C, nullptr, nullptr);
}

int gs_voxel_reduce(const float *x, const int32_t *counts, int N_max, int C, int B, const int32_t *voxel_of, const int32_t *n_voxels,
                    const int32_t *voxel_count, int M_max, int mode, float *out, void *ws, size_t ws_bytes, gs_stream_t stream) {
    GS_REQUIRE(x && counts && voxel_of && n_voxels && voxel_count && out, "gs_voxel_reduce: NULL argument");
    GS_REQUIRE(vred_shape_ok(B, N_max, C, M_max), "gs_voxel_reduce: bad shape B=%d N_max=%d C=%d M_max=%d (1 <= C <= 64, M_max <= N_max)",
               B, N_max, C, M_max);
    GS_REQUIRE(mode >= 0 && mode <= 3, "gs_voxel_reduce: bad mode %d", mode);
    GS_REQUIRE_WS("gs_voxel_reduce", ws, ws_bytes, gs_voxel_reduce_ws_bytes(B, M_max, C));
    hipStream_t st = (hipStream_t)stream;
    Fold w;
    const size_t bytes = vox_reduce_layout(B, M_max, C, ws, &w);
    const VredIn in{x, counts, voxel_of, n_voxels, voxel_count, N_max, C, M_max};
    const int lg = fold_lg(N_max);  // no voxel has more members
    GS_HIP(hipMemsetAsync(ws, 0, bytes, st), "gs_voxel_reduce/zero");
    hipLaunchKernelGGL(vred_max_k, dim3(rows_grid((int64_t)N_max * C, VOX_T, 4096), B), dim3(VOX_T), 0, st, in, w);
    const dim3 rows(rows_grid(N_max, VOX_T, 4096), B);
    if (mode & GS_VOXEL_NO_PREAGG) hipLaunchKernelGGL(vred_acc_k<false>, rows, dim3(VOX_T), 0, st, in, w, lg);
    else hipLaunchKernelGGL(vred_acc_k<true>, rows, dim3(VOX_T), 0, st, in, w, lg);
    GS_LAUNCH_CHECK("gs_voxel_reduce/fold");
    hipLaunchKernelGGL(vred_finish_k, dim3(rows_grid((int64_t)M_max * C, VOX_T, 4096), B), dim3(VOX_T), 0, st, in, w, lg, mode & GS_VOXEL_MEAN, out);
    GS_LAUNCH_CHECK("gs_voxel_reduce/finish");
    return GS_OK;
}

int gs_voxel_reduce_backward(const float *g_out, const int32_t *counts, int N_max, int C, int B, const int32_t *voxel_of,
                             const int32_t *voxel_count, int M_max, int mode, float *g_x, gs_stream_t stream) {
    GS_REQUIRE(g_out && counts && voxel_of && voxel_count && g_x, "gs_voxel_reduce_backward: NULL argument");
    GS_REQUIRE(vred_shape_ok(B, N_max, C, M_max),
               "gs_voxel_reduce_backward: bad shape B=%d N_max=%d C=%d M_max=%d (1 <= C <= 64, M_max <= N_max)", B, N_max, C, M_max);
    GS_REQUIRE(mode >= 0 && mode <= 3, "gs_voxel_reduce_backward: bad mode %d", mode);
    const VredIn in{nullptr, counts, voxel_of, nullptr, voxel_count, N_max, C, M_max};
    hipLaunchKernelGGL(vred_bwd_k, dim3(rows_grid((int64_t)N_max * C, VOX_T, 4096), B), dim3(VOX_T), 0, (hipStream_t)stream, g_out, in,
                       mode & GS_VOXEL_MEAN, g_x);
    GS_LAUNCH_CHECK("gs_voxel_reduce_backward");
    return GS_OK;
}

}  // extern "C"
