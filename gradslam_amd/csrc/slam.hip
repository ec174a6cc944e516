// slam.hip -- whole-step drivers: chains of the kernels of this library with every data-dependent size
// kept on the device, so one C call enqueues a complete ICPSLAM._localize (reference
// slam/icpslam.py:238-247) without a single host round trip.
#include <algorithm>
#include <chrono>
#include <mutex>
#include <stdlib.h>
#include <vector>

#include "gs_common.hpp"
#include "gs_drivers.hpp"
#include "gs_icp.hpp"

namespace gs {

// ------------------------------------------------------------------ hipGraph cache for the ICP loops
// Every argument of the (grad)ICP loop launched by gs_slam_localize lives in the caller's workspace, so
// for a given workspace address and configuration the ~35 launches are the same bytes every frame:
// capture them once (on a private stream: the user's may be the legacy default stream, which cannot be
// captured) and replay the instantiated graph on the user's stream.  Replay costs one launch on the host
// instead of ~35, which is what keeps the step GPU-bound on slow hosts.  GS_NO_GRAPH=1 disables it.
struct GraphKey {
    void *ws;
    int B, capS, capT, numiters, use_grad;
    float damp, thresh, lmax, Bp, B2, nu;
    int icp_cfg;             // what else decides WHICH kernels a loop launches: gs_set_grid_search / gs_set_tile_points / gs_set_loop_waves
    int H, W, ds;            // the loop's constants hold the ds-grid's dimensions
    bool operator==(const GraphKey &o) const {
        return H == o.H && W == o.W && ds == o.ds && ws == o.ws && B == o.B && capS == o.capS && capT == o.capT && numiters == o.numiters && use_grad == o.use_grad &&
               damp == o.damp && thresh == o.thresh && lmax == o.lmax && Bp == o.Bp && B2 == o.B2 && nu == o.nu &&
               icp_cfg == o.icp_cfg;
    }
};
struct GraphEntry {
    GraphKey key;
    int device;
    hipGraphExec_t exec;
    unsigned long long last_use;
};
static std::mutex g_graph_mu;
static std::vector<GraphEntry> g_graphs;
static std::vector<GraphKey> g_seen_once;  // a configuration is captured the second time it shows up
static unsigned long long g_graph_clock = 0;
static int g_graph_mode = -1;  // -1: automatic, 0: off, 1: on
// Automatic mode.  With the step folded into the association a loop is 13 launches, and on a fast host
// launching them eagerly is as fast as replaying a graph (and lets the loop's last launch write the composed
// pose); on a slow host the ~2x lower host cost of a replay is what keeps the step GPU-bound.  So the library
// times its own eager enqueues (host clock around the loop's launches, minimum over the first calls -- the
// minimum, because a full queue makes a launch block) and turns graphs on only if a launch costs the host
// more than kSlowLaunchUs -- about where the ~24 launches of a step would take the host as long as they take
// the GPU (a fast host needs ~3 us per launch).  Capturing costs several milliseconds once, so a borderline
// host is better off eager.  GS_NO_GRAPH=1 / GS_GRAPH=1 in the environment, or gs_set_graph_mode, override.
constexpr double kSlowLaunchUs = 8.0;
static int g_auto_samples = 0;
static double g_auto_min_us = 1e30;
static int g_captures = 0, g_replays = 0;
static bool graphs_allowed() {
    static const bool env_off = getenv("GS_NO_GRAPH") != nullptr, env_on = getenv("GS_GRAPH") != nullptr;
    if (profiling_enabled()) return false;
    if (g_graph_mode >= 0) return g_graph_mode != 0;
    if (env_off) return false;
    if (env_on) return true;
    return g_auto_samples >= 4 && g_auto_min_us > kSlowLaunchUs;
}

// The cache's one call.  Replays the graph of `key` on `st`; a key seen for the second time is captured first:
// enqueue(capture stream) on a private non-blocking stream.  *launched stays false where there is no graph to replay (first
// sighting, or a capture that failed: its error is cleared) -- the caller then launches eagerly.
template <class Enqueue>
static int graph_replay(const GraphKey &key, hipStream_t st, Enqueue &&enqueue, bool *launched) {
    std::lock_guard<std::mutex> lock(g_graph_mu);
    int device = 0;
    (void)hipGetDevice(&device);
    GraphEntry *hit = nullptr;
    for (auto &e : g_graphs)
        if (e.device == device && e.key == key) hit = &e;
    bool seen = false;
    if (!hit) {
        for (auto &k : g_seen_once) seen = seen || (k == key);
        if (!seen) {
            if (g_seen_once.size() >= 16) g_seen_once.erase(g_seen_once.begin());
            g_seen_once.push_back(key);
        }
    }
    if (!hit && seen) {
        hipStream_t cs = nullptr;
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        bool ok = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) == hipSuccess;
        ok = ok && hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (ok) {
            const int r = enqueue(cs);
            const hipError_t e = hipStreamEndCapture(cs, &graph);
            ok = (r == GS_OK) && e == hipSuccess && graph != nullptr;
        }
        ok = ok && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
        if (graph) (void)hipGraphDestroy(graph);
        if (cs) (void)hipStreamDestroy(cs);
        if (ok) {
            if (g_graphs.size() >= 8) {  // evict the least recently used
                size_t v = 0;
                for (size_t i = 1; i < g_graphs.size(); ++i)
                    if (g_graphs[i].last_use < g_graphs[v].last_use) v = i;
                (void)hipGraphExecDestroy(g_graphs[v].exec);
                g_graphs.erase(g_graphs.begin() + v);
            }
            g_graphs.push_back(GraphEntry{key, device, exec, 0});
            hit = &g_graphs.back();
            ++g_captures;
        } else {
            (void)hipGetLastError();
        }
    }
    if (hit) {
        hit->last_use = ++g_graph_clock;
        ++g_replays;
        GS_HIP(hipGraphLaunch(hit->exec, st), "gs_slam_localize/graph");
        *launched = true;
    }
    return GS_OK;
}

// Automatic mode's sample: enqueue() eagerly, and what one of its `launches` launches cost the host.
template <class Enqueue>
static int eager_timed(int launches, Enqueue &&enqueue) {
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = enqueue();
    if (rc) return rc;
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    std::lock_guard<std::mutex> lock(g_graph_mu);
    if (g_auto_samples < 64) {
        ++g_auto_samples;
        g_auto_min_us = std::min(g_auto_min_us, us / launches);
    }
    return GS_OK;
}

// out[b] = T[b] . P[b]   (compose44, gs_common.hpp)
__global__ void compose_k(const float *__restrict__ T, const float *__restrict__ P, int B, float *__restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    compose44(T + 16 * b, P + 16 * b, out + 16 * b);
}

__global__ void eye4_k(float *__restrict__ T, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 16 * B) T[i] = ((i % 16) % 5 == 0) ? 1.0f : 0.0f;
}

struct LocWs {
    float *src;        // (B, capS, 3)
    int32_t *src_pix;  // (B, capS) ds-grid pixel of every source point
    float *scan;       // (B, capT, 3) target points in pixel order
    int32_t *scan_orig;// (B, capT)
    int32_t *pix_start;// (B, capS + 1) first scan slot of every ds-grid pixel
    int32_t *ns;       // (B)
    int64_t *rows;     // (B*Nmax, 4)
    int32_t *nrows;    // (1)
    float *tgt, *tnrm; // (B, capT, 3)
    int32_t *nt;       // (B)
    float *T;          // (B, 16) ICP result; eye (B,16) follows
    float *eye;
    float *cam;        // (B, 32) previous pose | intrinsics: the bucketing camera at a workspace address (graph replay)
    void *sub;         // scratch shared by the sub-calls (they run one after the other on one stream)
    size_t sub_bytes;
};

// target capacity: the map size rounded up to a power of two, so that the workspace layout (and with it the
// captured graph of the ICP loops) stays the same while a map grows frame by frame
static inline int target_cap(int Nmax) {
    int c = 1024;
    while (c < Nmax && c < (1 << 30)) c <<= 1;
    return c;
}

static size_t loc_layout(int B, int H, int W, int ds, int Nmax, void *ws, LocWs *out) {
    const int capS = cdiv(H, ds) * cdiv(W, ds), capT = target_cap(Nmax);
    Carve c{(char *)ws};
    LocWs scratch, &w = out ? *out : scratch;
    w.src = c.take<float>((size_t)B * capS * 12); w.ns = c.take<int32_t>((size_t)B * 4);
    w.src_pix = c.take<int32_t>((size_t)B * capS * 4); w.scan = c.take<float>((size_t)B * capT * 12);
    w.scan_orig = c.take<int32_t>((size_t)B * capT * 4); w.pix_start = c.take<int32_t>((size_t)B * (capS + 1) * 4);
    // NB every size below depends on (B, H, W, ds, capT) only -- never on Nmax itself -- so that pointers baked
    // into a captured graph stay valid while the map grows inside one capacity bucket
    w.rows = c.take<int64_t>((size_t)B * capT * 32); w.nrows = c.take<int32_t>(4);
    w.tgt = c.take<float>((size_t)B * capT * 12); w.tnrm = c.take<float>((size_t)B * capT * 12); w.nt = c.take<int32_t>((size_t)B * 4);
    w.T = c.take<float>((size_t)B * 64); w.eye = c.take<float>((size_t)B * 64); w.cam = c.take<float>((size_t)B * 128);
    w.sub_bytes = std::max({gs_downsample_frame_ws_bytes(H, W, ds), gs_project_active_ws_bytes(B, Nmax), gs_gather_table_rows_ws_bytes(B),
                            gs_bucket_by_pixel_ws_bytes(B, H, W, ds), gs_icp_ws_bytes(capS, capT), project_target1_ws_bytes(H, W, ds, Nmax)});
    w.sub = c.take(w.sub_bytes);
    return c.off;
}

// gs_set_fused_setup: the fused front end (project.hip: project_front1) for one sequence; the environment's GS_FUSED_SETUP
// (measurements) sets the default
static int g_fused_setup = getenv("GS_FUSED_SETUP") ? atoi(getenv("GS_FUSED_SETUP")) : 1;
static inline bool fused_front(int B, int H, int W, int ds) {
    return g_fused_setup != 0 && B == 1 && (int64_t)cdiv(H, ds) * cdiv(W, ds) <= kBucketPixMax;  // project_front1's limit
}

// The front end of both localisation entry points: the live frame's ds-grid source cloud (src, src_pix, ns) and, from the map
// points that land on the ds-grid of the previous frame, the ICP target -- reference-order points, normals and count (nt), the
// map index of every slot (tgt_index, optional), and the same points in pixel order with the first scan slot of every ds-grid
// pixel (search hints only).  The destinations are the workspace's (gs_slam_localize) or the tape's (gs_slam_localize_taped).
// compute_maps: the frame's maps under the previous pose are computed too (gvertex is then gvertex_out), and the bucketing
// camera -- previous pose | intrinsics -- lands at cam_out.  Otherwise gvertex is the caller's and the map outputs are NULL.
// One sequence takes the fused form (gs_set_fused_setup; maps + counts, write, bucketing: three launches) or, switched off,
// the 4-launch form behind the maps kernel, on whose first two launches the frame's ds-grid source cloud rides (two launches
// of ~5 us less on the step's chain); a batch takes the separate entry points.
static int enqueue_front(const float *depth, const float *gvertex, const float *intrinsics, const float *prev_poses, int B, int H, int W,
                         int ds, const float *map_points, const float *map_normals, const int32_t *map_counts, int Nmax, const LocWs &w,
                         float *src, int32_t *src_pix, int32_t *ns, int32_t *nt, int32_t *tgt_index, bool compute_maps, float *vertex,
                         float *normal, float *gvertex_out, float *gnormal, float *cam_out, hipStream_t st) {
    const int capS = cdiv(H, ds) * cdiv(W, ds), capT = target_cap(Nmax);
    const DsJob frame{depth, gvertex, src, src_pix, ns};
    int rc;
    if (fused_front(B, H, W, ds))
        return project_front1(compute_maps ? depth : nullptr, map_points, map_counts, Nmax, prev_poses, intrinsics, H, W, ds, map_normals,
                              capT, vertex, normal, gvertex_out, gnormal, cam_out, (int32_t *)w.rows, w.tgt, w.tnrm, nt, tgt_index, w.scan,
                              w.scan_orig, w.pix_start, frame, w.sub, w.sub_bytes, st);
    if (compute_maps &&
        (rc = vertex_normal_maps_cam(depth, intrinsics, prev_poses, B, H, W, vertex, normal, gvertex_out, gnormal, cam_out, st))) return rc;
    if (B == 1)
        return project_target1(map_points, map_counts, Nmax, prev_poses, intrinsics, H, W, ds, map_normals, capT, w.rows, w.nrows, w.tgt,
                               w.tnrm, nt, w.scan, w.scan_orig, w.pix_start, tgt_index, nullptr, w.sub, w.sub_bytes, st, &frame);
    if ((rc = gs_downsample_frame(depth, gvertex, nullptr, nullptr, B, H, W, ds, capS, src, nullptr, nullptr, src_pix, ns, w.sub,
                                  w.sub_bytes, (gs_stream_t)st))) return rc;
    if ((rc = gs_project_active(map_points, map_counts, B, Nmax, prev_poses, intrinsics, H, W, ds, w.rows, w.nrows, w.sub, w.sub_bytes,
                                (gs_stream_t)st))) return rc;
    return gs_build_icp_target(w.rows, w.nrows, (int64_t)B * Nmax, B, H, W, ds, map_points, map_normals, Nmax, capT, w.tgt, w.tnrm, nt,
                               w.scan, w.scan_orig, w.pix_start, tgt_index, nullptr, w.sub, w.sub_bytes, (gs_stream_t)st);
}

// the search hints of batch element b's loop: the pixel-ordered target of the workspace, the source cloud's ds-grid pixels
// and the bucketing camera (pose, intrinsics: 16 floats each)
static inline gs_icp_hints loc_hints(const LocWs &w, const int32_t *src_pix, int b, int H, int W, int ds, int capS, int capT,
                                     const float *pose, const float *intrinsics) {
    return gs_icp_hints{w.scan + (size_t)b * capT * 3, w.scan_orig + (size_t)b * capT, src_pix + (size_t)b * capS,
                        w.pix_start + (size_t)b * (capS + 1), nullptr, cdiv(W, ds), cdiv(H, ds), pose, intrinsics, ds};
}

// ------------------------------------------------------------------ PointFusion map update on an arena
struct FuseWs {
    float *gV, *gN, *alpha;          // (B,H,W,3) x2, (B,H,W)
    void *state;                     // correspondence stage: per-pixel keys / winners, per-point pixel, per-block counts
    int32_t *ctr;                    // counter block: active, unique, overflow, max_dot bits, any-similar flag
    int32_t *appended;               // (B)
    int *totals;                     // (B) rows each sequence's append pass selected
    void *sub;
    size_t sub_bytes;
};
constexpr int kCtrWords = 64;  // counter block (zeroed by the maps kernel): ctr[0..], appended at +64, totals at +128
static size_t fuse_layout(int B, int H, int W, int Nmax, void *ws, FuseWs *out) {
    const size_t npix = (size_t)B * H * W;
    Carve c{(char *)ws};
    FuseWs scratch, &w = out ? *out : scratch;
    w.gV = c.take<float>(npix * 12); w.gN = c.take<float>(npix * 12); w.alpha = c.take<float>(npix * 4);
    w.state = c.take(fusion_corr_state_bytes(B, H, W, Nmax));
    w.ctr = c.take<int32_t>((size_t)(kCtrWords + 2 * 64) * 4);
    w.appended = w.ctr + kCtrWords; w.totals = (int *)(w.ctr + kCtrWords + 64);
    w.sub_bytes = append_scratch_bytes((int64_t)H * W);
    w.sub = c.take(w.sub_bytes);
    return c.off;
}

// gs_pointfusion_update_backward: the frame's maps again (B,H,W,3), alpha and its adjoint (B,H,W), the compaction's scratch
struct FuseBwdWs {
    float *V, *N, *gV, *gN, *alpha, *g_alpha;
    void *cws;
};
static size_t fuse_bwd_layout(int B, int H, int W, void *ws, FuseBwdWs *out) {
    const size_t npix = (size_t)B * H * W;
    Carve c{(char *)ws};
    FuseBwdWs scratch, &w = out ? *out : scratch;
    w.V = c.take<float>(npix * 12); w.N = c.take<float>(npix * 12); w.gV = c.take<float>(npix * 12); w.gN = c.take<float>(npix * 12);
    w.alpha = c.take<float>(npix * 4); w.g_alpha = c.take<float>(npix * 4);
    w.cws = c.take(append_scratch_bytes((int64_t)H * W));
    c.take(256);  // spare: nothing lives here, the size has always carried it
    return c.off;
}

// gs_aggregate_update: the frame's global maps (B,H,W,3), the counters its memset clears -- overflow flag (1), rows appended
// per sequence (B), counter_bytes in all -- and the compaction's scratch
struct AggWs {
    float *gV, *gN;
    int32_t *overflow, *appended;
    size_t counter_bytes;
    void *cws;
};
static size_t agg_layout(int B, int H, int W, void *ws, AggWs *out) {
    const size_t npix = (size_t)B * H * W;
    Carve c{(char *)ws};
    AggWs scratch, &w = out ? *out : scratch;
    w.gV = c.take<float>(npix * 12); w.gN = c.take<float>(npix * 12);
    const size_t counters = c.off;
    w.overflow = c.take<int32_t>(4); w.appended = c.take<int32_t>((size_t)B * 4);
    w.counter_bytes = c.off - counters;
    w.cws = c.take(append_scratch_bytes((int64_t)H * W));
    return c.off;
}

__global__ void fuse_stats_k(const int32_t *__restrict__ nrows, const int32_t *__restrict__ ucnt, const int32_t *__restrict__ overflow,
                             const float *__restrict__ max_dot, const int32_t *__restrict__ appended, int B,
                             int32_t *__restrict__ stats) {
    if (threadIdx.x == 0) {
        stats[0] = *nrows; stats[1] = *ucnt; stats[2] = *overflow; stats[3] = __float_as_int(*max_dot);
    }
    if ((int)threadIdx.x < B) stats[4 + threadIdx.x] = appended[threadIdx.x];
}

// ------------------------------------------------------------------ differentiable localisation
// Tape of one gs_slam_localize_taped call: what the reverse pass cannot cheaply recompute.
struct LocTape {
    float *src;         // (B, capS, 3) ds-grid source cloud
    int32_t *src_pix;   // (B, capS)   ds-grid pixel of every source point
    int32_t *ns, *nt;   // (B)
    int32_t *tgt_index; // (B, capT)   map index of every target slot
    float *T;           // (B, 16)     ICP result (before composition with the previous pose)
    char *icp;          // B x icp_tape bytes
    size_t icp_bytes;
};
static size_t loc_tape_layout(int B, int H, int W, int ds, int Nmax, int numiters, int grad_lm, void *tape, LocTape *out) {
    const int capS = cdiv(H, ds) * cdiv(W, ds), capT = target_cap(Nmax);
    Carve c{(char *)tape};
    LocTape scratch, &t = out ? *out : scratch;
    t.src = c.take<float>((size_t)B * capS * 12); t.src_pix = c.take<int32_t>((size_t)B * capS * 4);
    t.ns = c.take<int32_t>((size_t)B * 4); t.nt = c.take<int32_t>((size_t)B * 4);
    t.tgt_index = c.take<int32_t>((size_t)B * capT * 4); t.T = c.take<float>((size_t)B * 64);
    t.icp_bytes = align_up(gs_icp_tape_bytes(capS, numiters, grad_lm), 256);
    t.icp = c.take<char>((size_t)B * t.icp_bytes);
    return c.off;
}

// Workspace of the localisation reverse pass; its two modes differ in the last piece only, the ICP reverse pass's own.
struct LocBwdWs {
    float *tgt, *tnrm, *g_tgt, *g_nrm;  // (capT, 3): one batch element at a time
    float *g_src;                       // (capS, 3)
    float *g_T, *g_init, *eye;          // (B, 16)
    void *sub;
    size_t sub_bytes;
};
static size_t loc_bwd_layout(bool det, int B, int H, int W, int ds, int Nmax, int numiters, int grad_lm, void *ws, LocBwdWs *out) {
    const int capS = cdiv(H, ds) * cdiv(W, ds), capT = target_cap(Nmax);
    Carve c{(char *)ws};
    LocBwdWs scratch, &w = out ? *out : scratch;
    w.tgt = c.take<float>((size_t)capT * 12); w.tnrm = c.take<float>((size_t)capT * 12);
    w.g_tgt = c.take<float>((size_t)capT * 12); w.g_nrm = c.take<float>((size_t)capT * 12);
    w.g_src = c.take<float>((size_t)capS * 12);
    w.g_T = c.take<float>((size_t)B * 64); w.g_init = c.take<float>((size_t)B * 64); w.eye = c.take<float>((size_t)B * 64);
    w.sub_bytes = det ? gs_icp_backward_det_ws_bytes(capS, capT, numiters, grad_lm) : gs_icp_backward_ws_bytes(capS);
    w.sub = c.take(w.sub_bytes);
    return c.off;
}

// adjoint of compose_k: out = T . P
__global__ void compose_bwd_k(const float *__restrict__ T, const float *__restrict__ P, const float *__restrict__ gO, int B,
                              float *__restrict__ gT, float *__restrict__ gP) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float *a = T + 16 * b, *p = P + 16 * b, *g = gO + 16 * b;
    float *ga = gT + 16 * b, *gp = gP + 16 * b;
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) ga[4 * i + k] = ((g[4 * i] * p[4 * k] + g[4 * i + 1] * p[4 * k + 1]) + g[4 * i + 2] * p[4 * k + 2]) + g[4 * i + 3] * p[4 * k + 3];
        ga[4 * i + 3] = g[4 * i + 3];
    }
    for (int k = 0; k < 3; ++k)
        for (int j = 0; j < 4; ++j) gp[4 * k + j] = (a[k] * g[j] + a[4 + k] * g[4 + j]) + a[8 + k] * g[8 + j];
    for (int j = 0; j < 4; ++j) { ga[12 + j] = 0.0f; gp[12 + j] = 0.0f; }
}

// target / normals of every slot again from the map (what gs_build_icp_target gathered in the forward pass)
__global__ void regather_k(const int32_t *__restrict__ tgt_index, const int32_t *__restrict__ nt, int capT,
                           const float *__restrict__ map_points, const float *__restrict__ map_normals, int Nmax,
                           float *__restrict__ tgt, float *__restrict__ tnrm) {
    const int b = blockIdx.y, n = min(nt[b], capT);
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        const int64_t srcI = (int64_t)b * Nmax + tgt_index[(int64_t)b * capT + k], dst = (int64_t)b * capT + k;
        st3(tgt, dst, ld3(map_points, srcI));
        st3(tnrm, dst, ld3(map_normals, srcI));
    }
}

// adjoints back to where the clouds came from: source slot i -> its ds-grid pixel of the (zeroed) global vertex
// map adjoint; target slot k -> its map point (every map point is at most one slot: plain stores)
__global__ void scatter_grads_k(const float *__restrict__ g_src, const int32_t *__restrict__ src_pix, const int32_t *__restrict__ ns,
                                int capS, int Wd, int ds, int H, int W, float *__restrict__ g_gvertex /* this b */,
                                const float *__restrict__ g_tgt, const float *__restrict__ g_nrm,
                                const int32_t *__restrict__ tgt_index, const int32_t *__restrict__ nt, int capT,
                                float *__restrict__ g_map_points, float *__restrict__ g_map_normals /* this b */, int accumulate) {
    const int n_s = min(*ns, capS), n_t = min(*nt, capT);
    const int stride = gridDim.x * blockDim.x;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_s; i += stride) {
        const int pix = src_pix[i];
        const int64_t at = (int64_t)(pix / Wd) * ds * W + (int64_t)(pix % Wd) * ds;
        st3(g_gvertex, at, ld3(g_src, i));
    }
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n_t; k += stride) {
        const int64_t at = tgt_index[k];
        f3 gp = g_map_points ? ld3(g_tgt, k) : f3{0, 0, 0}, gq = g_map_normals ? ld3(g_nrm, k) : f3{0, 0, 0};
        if (accumulate) {  // a running adjoint of the whole map (one slot per map point: no atomics needed)
            if (g_map_points) { const f3 o = ld3(g_map_points, at); gp = f3{o.x + gp.x, o.y + gp.y, o.z + gp.z}; }
            if (g_map_normals) { const f3 o = ld3(g_map_normals, at); gq = f3{o.x + gq.x, o.y + gq.y, o.z + gq.z}; }
        }
        if (g_map_points) st3(g_map_points, at, gp);
        if (g_map_normals) st3(g_map_normals, at, gq);
    }
}

}  // namespace gs

using namespace gs;

extern "C" {

void gs_set_graph_mode(int mode) { g_graph_mode = mode; }

void gs_set_fused_setup(int on) { g_fused_setup = on; }

int gs_graph_stats(double *out4) {
    GS_REQUIRE(out4, "gs_graph_stats: NULL argument");
    std::lock_guard<std::mutex> lock(g_graph_mu);
    out4[0] = g_auto_samples; out4[1] = g_auto_min_us; out4[2] = g_captures; out4[3] = g_replays;
    return GS_OK;
}

int gs_compose_poses(const float *T, const float *P, int B, float *out, gs_stream_t stream) {
    GS_REQUIRE(T && P && out && B > 0, "gs_compose_poses: bad arguments");
    hipLaunchKernelGGL(compose_k, dim3(cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, T, P, B, out);
    GS_LAUNCH_CHECK("gs_compose_poses");
    return GS_OK;
}

size_t gs_slam_localize_ws_bytes(int B, int H, int W, int ds, int Nmax) {
    if (B <= 0 || H <= 0 || W <= 0 || ds <= 0 || Nmax <= 0) return 0;
    return loc_layout(B, H, W, ds, Nmax, nullptr, nullptr);
}

int gs_slam_localize(const float *depth, const float *intrinsics, const float *prev_poses, int B, int H, int W, int ds,
                     const float *map_points, const float *map_normals, const int32_t *map_counts, int Nmax,
                     int use_grad_lm, int numiters, float damp, float dist_thresh, float lambda_max, float Bp, float B2,
                     float nu, float *vertex, float *normal, float *gvertex, float *gnormal, float *out_poses, void *ws,
                     size_t ws_bytes, gs_stream_t stream) {
    GS_REQUIRE(depth && intrinsics && prev_poses && map_points && map_normals && map_counts && gvertex && out_poses,
               "gs_slam_localize: NULL argument (gvertex is required, the other maps are optional)");
    GS_REQUIRE(B > 0 && H >= 2 && W >= 2 && ds > 0 && Nmax > 0 && numiters >= 0, "gs_slam_localize: bad shape");
    GS_REQUIRE_WS("gs_slam_localize", ws, ws_bytes, gs_slam_localize_ws_bytes(B, H, W, ds, Nmax));
    hipStream_t st = (hipStream_t)stream;
    LocWs w;
    loc_layout(B, H, W, ds, Nmax, ws, &w);
    const int capS = cdiv(H, ds) * cdiv(W, ds), capT = target_cap(Nmax);
    int rc;
    if ((rc = enqueue_front(depth, gvertex, intrinsics, prev_poses, B, H, W, ds, map_points, map_normals, map_counts, Nmax, w, w.src,
                            w.src_pix, w.ns, w.nt, nullptr, true, vertex, normal, gvertex, gnormal, w.cam, st))) return rc;
    // fold_compose: the loop's last launch also writes out_poses = T . prev_poses.  Only for eager launches: a
    // captured graph must not bake the caller's prev_poses / out_poses addresses in (they change every call); for the same
    // reason the loops read the camera from the workspace, never from the caller's tensors.
    auto enqueue_loops = [&](hipStream_t s, bool fold_compose) -> int {
        for (int b = 0; b < B; ++b) {  // sequences are independent; one device-resident loop each
            const gs_icp_hints hints = loc_hints(w, w.src_pix, b, H, W, ds, capS, capT, w.cam + 32 * b, w.cam + 32 * b + 16);
            const int r = icp_localize_run(use_grad_lm, w.src + (size_t)b * capS * 3, w.ns + b, capS, w.tgt + (size_t)b * capT * 3,
                                           w.tnrm + (size_t)b * capT * 3, w.nt + b, capT, numiters, damp, dist_thresh, lambda_max, Bp,
                                           B2, nu, &hints, w.T + 16 * b, w.sub, w.sub_bytes, s, nullptr, 0,
                                           fold_compose ? prev_poses + 16 * b : nullptr, fold_compose ? out_poses + 16 * b : nullptr);
            if (r) return r;
        }
        return GS_OK;
    };
    bool launched = false;
    if (graphs_allowed() && numiters > 0) {
        const GraphKey key{ws, B, capS, capT, numiters, use_grad_lm, damp, dist_thresh, lambda_max, Bp, B2, nu,
                           icp_config_stamp(), H, W, ds};
        if ((rc = graph_replay(key, st, [&](hipStream_t cs) { return enqueue_loops(cs, false); }, &launched))) return rc;
    }
    if (!launched) {
        if (numiters > 0)  // composed by the loop's last launch
            return eager_timed(B * ((use_grad_lm ? 2 * numiters : numiters + 1) + 2), [&] { return enqueue_loops(st, true); });
        if ((rc = enqueue_loops(st, false))) return rc;
    }
    return gs_compose_poses(w.T, prev_poses, B, out_poses, stream);
}

size_t gs_pointfusion_update_ws_bytes(int B, int H, int W, int Nmax) {
    if (B <= 0 || H <= 0 || W <= 0 || Nmax <= 0) return 0;
    return fuse_layout(B, H, W, Nmax, nullptr, nullptr);
}

static int pointfusion_update_impl(const float *depth, const float *rgb, const float *intrinsics, const float *poses, int B, int H, int W,
                                   float *map_points, float *map_normals, float *map_colors, float *map_ccounts, int32_t *map_counts,
                                   int Nmax, float dist_th, float dot_th, float sigma, int32_t *stats, void *ws, size_t ws_bytes,
                                   gs_stream_t stream, void *tape, const char *name) {
    GS_REQUIRE(depth && rgb && intrinsics && poses && map_points && map_normals && map_colors && map_ccounts && map_counts,
               "%s: NULL argument", name);
    GS_REQUIRE(B > 0 && B <= 60 && H >= 2 && W >= 2 && Nmax > 0, "%s: bad shape", name);
    GS_REQUIRE_WS(name, ws, ws_bytes, gs_pointfusion_update_ws_bytes(B, H, W, Nmax));
    hipStream_t st = (hipStream_t)stream;
    FuseWs w;
    fuse_layout(B, H, W, Nmax, ws, &w);
    int rc;
    // live frame under its final pose: global maps, the sample confidence from the LOCAL vertex map
    // (fusionutils.py:650-652), and -- riding on the same pass over the pixels -- the correspondence stage's per-pixel
    // state and the counter block initialised (no memset, no alpha launch)
    unsigned long long *pix_key; unsigned int *pix_n;
    fusion_corr_init_ptrs(w.state, B, H, W, Nmax, &pix_key, &pix_n);
    if ((rc = vertex_normal_maps_fusion(depth, intrinsics, poses, B, H, W, w.gV, w.gN, w.alpha, sigma, 1e-7f, pix_key, pix_n, w.ctr,
                                        kCtrWords + 2 * 64, st))) return rc;
    // find_correspondences (fusionutils.py:549-577): active -> similar -> best unique per pixel, without the tables
    if ((rc = fusion_correspond(w.state, map_points, map_normals, map_ccounts, map_counts, B, Nmax, poses, intrinsics, H, W, w.gV, w.gN,
                                dist_th, dot_th, w.ctr, st))) return rc;
    // differentiable form: the winners and the matched rows' values before the merge go to the tape
    if (tape && (rc = fusion_tape_record(w.state, tape, B, H, W, Nmax, map_counts, map_points, map_normals, map_colors, map_ccounts, st)))
        return rc;
    // fuse_with_map (fusionutils.py:654-720): merge in place, then append the unmatched valid pixels
    if ((rc = fusion_merge_corr(w.state, w.ctr, w.gV, w.gN, rgb, w.alpha, B, H, W, Nmax, map_counts, map_points, map_normals, map_colors,
                                map_ccounts, st))) return rc;
    const int64_t HW = (int64_t)H * W;
    for (int b = 0; b < B; ++b) {
        const float *src[4] = {w.gV + b * HW * 3, w.gN + b * HW * 3, rgb + b * HW * 3, w.alpha + b * HW};
        float *dst[4] = {map_points + (size_t)b * Nmax * 3, map_normals + (size_t)b * Nmax * 3, map_colors + (size_t)b * Nmax * 3,
                         map_ccounts + (size_t)b * Nmax};
        const int widths[4] = {3, 3, 3, 1};
        if ((rc = fusion_append_corr(w.state, B, H, W, Nmax, b, depth, src, widths, dst, map_counts + b, Nmax, w.totals + b, w.sub, st)))
            return rc;
    }
    if ((rc = fusion_finish(w.state, B, H, W, Nmax, w.ctr, map_counts, w.totals, Nmax, w.appended, stats, st))) return rc;
    if (tape && (rc = fusion_tape_appended(tape, B, H, W, w.appended, st))) return rc;
    return GS_OK;
}

int gs_pointfusion_update(const float *depth, const float *rgb, const float *intrinsics, const float *poses, int B, int H, int W,
                          float *map_points, float *map_normals, float *map_colors, float *map_ccounts, int32_t *map_counts,
                          int Nmax, float dist_th, float dot_th, float sigma, int32_t *stats, void *ws, size_t ws_bytes,
                          gs_stream_t stream) {
    return pointfusion_update_impl(depth, rgb, intrinsics, poses, B, H, W, map_points, map_normals, map_colors, map_ccounts, map_counts,
                                   Nmax, dist_th, dot_th, sigma, stats, ws, ws_bytes, stream, nullptr, "gs_pointfusion_update");
}

size_t gs_pointfusion_update_tape_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return fusion_tape_bytes(B, H, W);
}

int gs_pointfusion_update_taped(const float *depth, const float *rgb, const float *intrinsics, const float *poses, int B, int H, int W,
                                float *map_points, float *map_normals, float *map_colors, float *map_ccounts, int32_t *map_counts,
                                int Nmax, float dist_th, float dot_th, float sigma, int32_t *stats, void *tape, size_t tape_bytes,
                                void *ws, size_t ws_bytes, gs_stream_t stream) {
    GS_REQUIRE_TAPE("gs_pointfusion_update_taped", tape, tape_bytes, gs_pointfusion_update_tape_bytes(B, H, W), GS_ERR_INVALID_ARG);
    return pointfusion_update_impl(depth, rgb, intrinsics, poses, B, H, W, map_points, map_normals, map_colors, map_ccounts, map_counts,
                                   Nmax, dist_th, dot_th, sigma, stats, ws, ws_bytes, stream, tape, "gs_pointfusion_update_taped");
}

size_t gs_pointfusion_update_backward_ws_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return fuse_bwd_layout(B, H, W, nullptr, nullptr);
}

int gs_pointfusion_update_backward(const float *depth, const float *rgb, const float *intrinsics, const float *poses, int B, int H,
                                   int W, float *map_points, float *map_normals, float *map_colors, float *map_ccounts,
                                   int32_t *map_counts, int Nmax, float sigma, const void *tape, size_t tape_bytes, float *G_points,
                                   float *G_normals, float *G_colors, float *G_ccounts, float *g_vertex, float *g_gvertex,
                                   float *g_gnormal, float *g_rgb, void *ws, size_t ws_bytes, gs_stream_t stream) {
    const char *name = "gs_pointfusion_update_backward";
    GS_REQUIRE(depth && rgb && intrinsics && poses && map_points && map_normals && map_colors && map_ccounts && map_counts && tape &&
                   G_points && G_normals && G_colors && G_ccounts && g_vertex && g_gvertex && g_gnormal && g_rgb, "%s: NULL argument", name);
    GS_REQUIRE(B > 0 && B <= 60 && H >= 2 && W >= 2 && Nmax > 0, "%s: bad shape", name);
    GS_REQUIRE_TAPE(name, tape, tape_bytes, gs_pointfusion_update_tape_bytes(B, H, W), GS_ERR_INVALID_ARG);
    GS_REQUIRE_WS(name, ws, ws_bytes, gs_pointfusion_update_backward_ws_bytes(B, H, W));
    hipStream_t st = (hipStream_t)stream;
    const size_t npix = (size_t)B * H * W;
    FuseBwdWs w;
    fuse_bwd_layout(B, H, W, ws, &w);
    int rc;
    // the frame's maps and sample confidences again (cheaper to recompute than to keep per frame)
    if ((rc = gs_vertex_normal_maps(depth, intrinsics, poses, B, 1, H, W, w.V, w.N, w.gV, w.gN, stream))) return rc;
    if ((rc = gs_get_alpha(w.V, (int64_t)npix, sigma, 1e-7f, w.alpha, stream))) return rc;
    if ((rc = fusion_update_reverse(tape, B, H, W, Nmax, depth, w.gV, w.gN, rgb, w.alpha, map_points, map_normals, map_colors, map_ccounts,
                                    map_counts, G_points, G_normals, G_colors, G_ccounts, g_gvertex, g_gnormal, g_rgb, w.g_alpha, w.cws,
                                    st))) return rc;
    // alpha = f(local vertex map): its adjoint is the only one the local vertex map receives from the update
    // (gs_get_alpha_backward adds into its output)
    GS_HIP(hipMemsetAsync(g_vertex, 0, npix * 12, st), name);
    return gs_get_alpha_backward(w.V, (int64_t)npix, sigma, 1e-7f, w.g_alpha, g_vertex, stream);
}

size_t gs_aggregate_update_ws_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return agg_layout(B, H, W, nullptr, nullptr);
}

int gs_aggregate_update(const float *depth, const float *rgb, const float *intrinsics, const float *poses, int B, int H, int W,
                        float *map_points, float *map_normals, float *map_colors, int32_t *map_counts, int Nmax, int32_t *stats,
                        void *ws, size_t ws_bytes, gs_stream_t stream) {
    const char *name = "gs_aggregate_update";
    GS_REQUIRE(depth && rgb && intrinsics && poses && map_points && map_normals && map_colors && map_counts, "%s: NULL argument", name);
    GS_REQUIRE(B > 0 && B <= 60 && H >= 2 && W >= 2 && Nmax > 0, "%s: bad shape", name);
    GS_REQUIRE_WS(name, ws, ws_bytes, gs_aggregate_update_ws_bytes(B, H, W));
    hipStream_t st = (hipStream_t)stream;
    AggWs w;
    agg_layout(B, H, W, ws, &w);
    GS_HIP(hipMemsetAsync(w.overflow, 0, w.counter_bytes, st), name);
    int rc;
    if ((rc = gs_vertex_normal_maps(depth, intrinsics, poses, B, 1, H, W, nullptr, nullptr, w.gV, w.gN, stream))) return rc;
    const int64_t HW = (int64_t)H * W;
    for (int b = 0; b < B; ++b) {
        const float *src[3] = {w.gV + b * HW * 3, w.gN + b * HW * 3, rgb + b * HW * 3};
        float *dst[3] = {map_points + (size_t)b * Nmax * 3, map_normals + (size_t)b * Nmax * 3, map_colors + (size_t)b * Nmax * 3};
        const int widths[3] = {3, 3, 3};
        if ((rc = append_valid_pixels(3, depth + b * HW, HW, src, widths, dst, map_counts + b, Nmax, w.appended + b, w.overflow, w.cws,
                                      st))) return rc;
    }
    if (stats) {
        hipLaunchKernelGGL(fuse_stats_k, dim3(1), dim3(64), 0, st, w.overflow, w.overflow, w.overflow, (const float *)w.overflow, w.appended, B,
                           stats);
        GS_LAUNCH_CHECK(name);
    }
    return GS_OK;
}

size_t gs_slam_localize_tape_bytes(int B, int H, int W, int ds, int Nmax, int numiters, int use_grad_lm) {
    if (B <= 0 || H <= 0 || W <= 0 || ds <= 0 || Nmax <= 0 || numiters < 0) return 0;
    return loc_tape_layout(B, H, W, ds, Nmax, numiters, use_grad_lm, nullptr, nullptr);
}

int gs_slam_localize_taped(const float *depth, const float *gvertex, const float *intrinsics, const float *prev_poses, int B, int H,
                           int W, int ds, const float *map_points, const float *map_normals, const int32_t *map_counts, int Nmax,
                           int use_grad_lm, int numiters, float damp, float dist_thresh, float lambda_max, float Bp, float B2,
                           float nu, float *out_poses, void *tape, size_t tape_bytes, void *ws, size_t ws_bytes,
                           gs_stream_t stream) {
    GS_REQUIRE(depth && gvertex && intrinsics && prev_poses && map_points && map_normals && map_counts && out_poses && tape,
               "gs_slam_localize_taped: NULL argument");
    GS_REQUIRE(B > 0 && H >= 2 && W >= 2 && ds > 0 && Nmax > 0 && numiters >= 0, "gs_slam_localize_taped: bad shape");
    GS_REQUIRE_WS("gs_slam_localize_taped", ws, ws_bytes, gs_slam_localize_ws_bytes(B, H, W, ds, Nmax));
    GS_REQUIRE_TAPE("gs_slam_localize_taped", tape, tape_bytes, gs_slam_localize_tape_bytes(B, H, W, ds, Nmax, numiters, use_grad_lm),
                    GS_ERR_INVALID_ARG);
    hipStream_t st = (hipStream_t)stream;
    LocWs w;
    loc_layout(B, H, W, ds, Nmax, ws, &w);
    LocTape tp;
    loc_tape_layout(B, H, W, ds, Nmax, numiters, use_grad_lm, tape, &tp);
    const int capS = cdiv(H, ds) * cdiv(W, ds), capT = target_cap(Nmax);
    int rc;
    // (the maps are the caller's: gvertex is an input here -- the fused form's count launch carries no maps' tiles)
    if ((rc = enqueue_front(depth, gvertex, intrinsics, prev_poses, B, H, W, ds, map_points, map_normals, map_counts, Nmax, w, tp.src,
                            tp.src_pix, tp.ns, tp.nt, tp.tgt_index, false, nullptr, nullptr, nullptr, nullptr, nullptr, st))) return rc;
    for (int b = 0; b < B; ++b) {
        const gs_icp_hints hints = loc_hints(w, tp.src_pix, b, H, W, ds, capS, capT, prev_poses + 16 * b, intrinsics + 16 * b);
        if ((rc = icp_localize_run(use_grad_lm, tp.src + (size_t)b * capS * 3, tp.ns + b, capS, w.tgt + (size_t)b * capT * 3,
                                   w.tnrm + (size_t)b * capT * 3, tp.nt + b, capT, numiters, damp, dist_thresh, lambda_max, Bp, B2, nu,
                                   &hints, tp.T + 16 * b, w.sub, w.sub_bytes, st, tp.icp + (size_t)b * tp.icp_bytes, tp.icp_bytes,
                                   prev_poses + 16 * b, out_poses + 16 * b)))
            return rc;
    }
    if (numiters == 0) return gs_compose_poses(tp.T, prev_poses, B, out_poses, stream);
    return GS_OK;
}

size_t gs_slam_localize_backward_ws_bytes(int B, int H, int W, int ds, int Nmax) {
    if (B <= 0 || H <= 0 || W <= 0 || ds <= 0 || Nmax <= 0) return 0;
    return loc_bwd_layout(false, B, H, W, ds, Nmax, 0, 0, nullptr, nullptr);
}

size_t gs_slam_localize_backward_det_ws_bytes(int B, int H, int W, int ds, int Nmax, int numiters, int grad_lm) {
    if (B <= 0 || H <= 0 || W <= 0 || ds <= 0 || Nmax <= 0) return 0;
    return loc_bwd_layout(true, B, H, W, ds, Nmax, numiters, grad_lm, nullptr, nullptr);
}

static int localize_backward(bool det, const float *prev_poses, int B, int H, int W, int ds, const float *map_points,
                             const float *map_normals, int Nmax, int use_grad_lm, int numiters, float dist_thresh,
                             float lambda_max, float Bp, float B2, float nu, const void *tape, size_t tape_bytes,
                             const float *grad_out_poses, float *grad_gvertex, float *grad_map_points, float *grad_map_normals,
                             float *grad_prev_poses, int accumulate_map_grads, void *ws, size_t ws_bytes, gs_stream_t stream) {
    const char *name = det ? "gs_slam_localize_backward_det" : "gs_slam_localize_backward";
    GS_REQUIRE(prev_poses && map_points && map_normals && tape && grad_out_poses && grad_gvertex && grad_prev_poses,
               "%s: NULL argument", name);
    GS_REQUIRE(B > 0 && H >= 2 && W >= 2 && ds > 0 && Nmax > 0 && numiters >= 0, "%s: bad shape", name);
    GS_REQUIRE_WS(name, ws, ws_bytes, loc_bwd_layout(det, B, H, W, ds, Nmax, numiters, use_grad_lm, nullptr, nullptr));
    GS_REQUIRE_TAPE(name, tape, tape_bytes, gs_slam_localize_tape_bytes(B, H, W, ds, Nmax, numiters, use_grad_lm), GS_ERR_INVALID_ARG);
    hipStream_t st = (hipStream_t)stream;
    LocTape tp;
    loc_tape_layout(B, H, W, ds, Nmax, numiters, use_grad_lm, (void *)tape, &tp);
    const int capS = cdiv(H, ds) * cdiv(W, ds), capT = target_cap(Nmax);
    LocBwdWs w;
    loc_bwd_layout(det, B, H, W, ds, Nmax, numiters, use_grad_lm, ws, &w);
    auto icp_backward = det ? gs_icp_point_to_plane_backward_det : gs_icp_point_to_plane_backward;

    GS_HIP(hipMemsetAsync(grad_gvertex, 0, (size_t)B * H * W * 12, st), name);
    if (grad_map_points && !accumulate_map_grads) GS_HIP(hipMemsetAsync(grad_map_points, 0, (size_t)B * Nmax * 12, st), name);
    if (grad_map_normals && !accumulate_map_grads) GS_HIP(hipMemsetAsync(grad_map_normals, 0, (size_t)B * Nmax * 12, st), name);
    hipLaunchKernelGGL(eye4_k, dim3(cdiv(16 * B, 64)), dim3(64), 0, st, w.eye, B);
    hipLaunchKernelGGL(compose_bwd_k, dim3(cdiv(B, 64)), dim3(64), 0, st, tp.T, prev_poses, grad_out_poses, B, w.g_T, grad_prev_poses);
    GS_LAUNCH_CHECK(name);
    const int gb = min(cdiv(capS, 256), 512);
    for (int b = 0; b < B; ++b) {
        // NB the gathered arrays hold one batch element at a time: index them with b = 0
        hipLaunchKernelGGL(regather_k, dim3(gb, 1), dim3(256), 0, st, tp.tgt_index + (size_t)b * capT, tp.nt + b, capT,
                           map_points + (size_t)b * Nmax * 3, map_normals + (size_t)b * Nmax * 3, Nmax, w.tgt, w.tnrm);
        GS_LAUNCH_CHECK(name);
        int rc;
        if ((rc = icp_backward(tp.src + (size_t)b * capS * 3, tp.ns + b, capS, w.tgt, w.tnrm, tp.nt + b, capT, w.eye + 16 * b, numiters,
                               dist_thresh, use_grad_lm, lambda_max, Bp, B2, nu, tp.icp + (size_t)b * tp.icp_bytes, tp.icp_bytes,
                               w.g_T + 16 * b, w.g_src, grad_map_points ? w.g_tgt : nullptr, grad_map_normals ? w.g_nrm : nullptr,
                               w.g_init + 16 * b, w.sub, w.sub_bytes, stream)))
            return rc;
        hipLaunchKernelGGL(scatter_grads_k, dim3(gb), dim3(256), 0, st, w.g_src, tp.src_pix + (size_t)b * capS, tp.ns + b, capS,
                           cdiv(W, ds), ds, H, W, grad_gvertex + (size_t)b * H * W * 3, w.g_tgt, w.g_nrm, tp.tgt_index + (size_t)b * capT,
                           tp.nt + b, capT, grad_map_points ? grad_map_points + (size_t)b * Nmax * 3 : nullptr,
                           grad_map_normals ? grad_map_normals + (size_t)b * Nmax * 3 : nullptr, accumulate_map_grads);
        GS_LAUNCH_CHECK(name);
    }
    return GS_OK;
}

int gs_slam_localize_backward(const float *prev_poses, int B, int H, int W, int ds, const float *map_points,
                              const float *map_normals, int Nmax, int use_grad_lm, int numiters, float dist_thresh,
                              float lambda_max, float Bp, float B2, float nu, const void *tape, size_t tape_bytes,
                              const float *grad_out_poses, float *grad_gvertex, float *grad_map_points, float *grad_map_normals,
                              float *grad_prev_poses, int accumulate_map_grads, void *ws, size_t ws_bytes, gs_stream_t stream) {
    return localize_backward(false, prev_poses, B, H, W, ds, map_points, map_normals, Nmax, use_grad_lm, numiters, dist_thresh, lambda_max,
                             Bp, B2, nu, tape, tape_bytes, grad_out_poses, grad_gvertex, grad_map_points, grad_map_normals, grad_prev_poses,
                             accumulate_map_grads, ws, ws_bytes, stream);
}

int gs_slam_localize_backward_det(const float *prev_poses, int B, int H, int W, int ds, const float *map_points,
                                  const float *map_normals, int Nmax, int use_grad_lm, int numiters, float dist_thresh,
                                  float lambda_max, float Bp, float B2, float nu, const void *tape, size_t tape_bytes,
                                  const float *grad_out_poses, float *grad_gvertex, float *grad_map_points, float *grad_map_normals,
                                  float *grad_prev_poses, int accumulate_map_grads, void *ws, size_t ws_bytes, gs_stream_t stream) {
    return localize_backward(true, prev_poses, B, H, W, ds, map_points, map_normals, Nmax, use_grad_lm, numiters, dist_thresh, lambda_max,
                             Bp, B2, nu, tape, tape_bytes, grad_out_poses, grad_gvertex, grad_map_points, grad_map_normals, grad_prev_poses,
                             accumulate_map_grads, ws, ws_bytes, stream);
}

}  // extern "C"
