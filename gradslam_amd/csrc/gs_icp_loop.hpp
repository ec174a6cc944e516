// gs_icp_loop.hpp -- the association launch of the ICP loops (knn1_loop_k: search, linearisation epilogue and the
// preceding step folded into its prologue; the design is in the comment above it) and the loops' set-up kernels.
// Included by icp.hip.
#pragma once

#include "gs_icp_step.hpp"
#include "gs_project.hpp"

namespace gs {

// Association launch of the loops, with the PRECEDING step folded into its prologue.
// A tiny dependent kernel costs ~4.5 us of stream time on this part however little it computes, so the loop's
// O(1) step (reduce the previous launch's partial sums, LM / gradLM decision, 6x6 solve, exp) is not a launch
// of its own: every block of the next association recomputes it from the previous launch's outputs (S_in,
// partials_in -- complete and visible at kernel start, no inter-block hand-off inside a launch) into LDS, and
// block 0 alone publishes the new state (S_out, tape record, trace, out_T).  State and partial sums are
// double-buffered across launches so that no block reads what another block of the same launch writes.
// Then: in = (first ? user source : pts[p_cur]) transformed by dT, out = pts[out_slot], NN -> best[out_slot]
// (out_slot < 0: the other one of the two ping-pong slots).  Seed: the current cloud's NN of the same source index
// when there is one, else the sampled seed pass.
//
// GRID (all search hints given): the association is a GRID SEARCH WITH A GEOMETRIC PROOF.
//   window : the target is bucketed by ds-grid pixel of the camera it was selected with (scan order, hints.pix_start).
//            Every lane examines ALL targets of the 3 x 3 pixels around the pixel its point projects to (three
//            contiguous slot ranges, exact: LaneWin), staged through LDS by coalesced loads issued before the
//            folded step, so they cost no time.  The lanes of a tile move together, so their windows lie in at most
//            four row bands, each one contiguous slot range (row-major pixels), which share a pool of POOL staged points.
//   proof  : every target OUTSIDE the window projects at least 2 ds - 0.5 image pixels from the window's centre pixel,
//            i.e. lies beyond one of four planes through the camera centre; the point's distance to the nearest of those
//            planes bounds its distance to all of them from below (cam_bound2).  A window best strictly inside that
//            bound IS the nearest neighbour, tie-break included, and no box is touched: nothing is carried from launch
//            to launch, the first association of a loop is proven like every other.  Lanes that fail (no map point
//            within centimetres: new image regions, depth edges) take the exact chunk-box search, restricted to them.
// The result is the brute-force scan's in every case; only the cost differs (~100 candidates per point at ten targets
// per pixel instead of ~800 and no box tests).
// What stays the same for every launch of one loop lives in the workspace (written once by icp_prepare_k), not in
// the kernel arguments: at ~100 scalar registers a 1024-thread block no longer shares its CU with a second one (the
// hardware admits floor(800 / (ceil(sgpr / 16) 16 + 16)) waves per SIMD: 8 up to 80 SGPRs, 7 from 82 on -- whatever
// the compiler's occupancy estimate says), and the association kernel lives on that second block.
struct LoopConst {
    const float *user_src, *tgt, *nrm, *boxes, *sboxes;
    const int32_t *d_ns, *d_nt;
    float *trace, *out_T;
    gs_icp_hints hints;
    GradParams gp;
    float thresh;
    int ns, nt;            // *d_ns, *d_nt as icp_prepare_k found them (one dependent load less at every kernel start)
    int cert_off;          // measurements only (GS_CERT_OFF=1): never trust a proof -> every association searches exactly
    int tile_points;       // source points per block (lanes 0 .. tile_points - 1 of every wave hold one each): 64, or what
                           // gs_set_tile_points forces (tests)
    int grid_variant;         // this loop launches knn1_loop_k<true> (for the loop counters only)
    // the camera the targets were bucketed with (hints.cam_pose / cam_K as icp_prepare_k read them): world -> camera as
    // project_point (gs_project.hpp) applies it, and the pinhole constants.  cam_ok = 0: K is not a plain pinhole
    // matrix (skew, a projective third row ...) -> no geometric proof, every association searches exactly.
    CamK cam;
    int cam_ok;
    int32_t *cells;           // (2, cells_stride): the ds-grid pixel every point of the cloud an association wrote projects to,
    int cells_stride;         // by launch parity -- where the NEXT launch centres its windows (knn1_loop_k)
};

// world point -> camera coordinates of the bucketing camera, with project_point's arithmetic (gs_project.hpp)
__device__ __forceinline__ f3 cam_point(const CamK &k, const f3 p) {
    return f3{dot3_fma(p.x, p.y, p.z, k.R[0], k.R[3], k.R[6]) + k.T[0],
              dot3_fma(p.x, p.y, p.z, k.R[1], k.R[4], k.R[7]) + k.T[1],
              dot3_fma(p.x, p.y, p.z, k.R[2], k.R[5], k.R[8]) + k.T[2]};
}
// the ds-grid pixel (row-major id) whose centre is nearest to the projection of p (clamped into the grid; any value is
// safe: the proof below is evaluated against whatever centre was chosen)
__device__ __forceinline__ int cam_cell(const CamK &k, const f3 p) {
    const f3 q = cam_point(k, p);
    const float zs = (q.z != 0.0f) ? q.z : 1.0f;
    const float ds = (float)k.ds;
    const float u = ((k.fx * q.x + k.cx * q.z) / zs) / ds, v = ((k.fy * q.y + k.cy * q.z) / zs) / ds;
    const int cc = (int)fminf(fmaxf(rintf(u), 0.0f), (float)(k.Wd - 1));
    const int cr = (int)fminf(fmaxf(rintf(v), 0.0f), (float)(k.Hd - 1));
    return cr * k.Wd + cc;
}
// GEOMETRIC PROOF.  Squared lower bound on the distance from s to every target OUTSIDE the (2R+1)^2 grid pixels around
// `centre`.  A target sits in grid pixel (r, c) iff its projection (u, v) rounds to the image pixel (r ds, c ds), so
// |u - c ds| <= 0.5 and |v - r ds| <= 0.5 (+ ~1e-3 of fp32 error in the bucketing's own projection).  A target outside the
// window therefore has u >= U+ = (cc + R + 1) ds - 0.5, or u <= U- = (cc - R - 1) ds + 0.5, or the same in v.  With
// z > 0 (only points in front of the camera are targets), u >= U+ means fx x + (cx - U+) z >= 0: a half-space whose
// boundary plane passes through the camera centre -- and likewise for the other three sides.  The distance from s to a
// half-space it is not in is the distance to its plane; the minimum over the (up to four) sides that can hold targets
// at all -- beyond the image border there are none -- bounds the distance to every outside target from below.  Rigid
// transforms preserve distances, so the bound is evaluated in camera coordinates.  Margins: 0.52 instead of 0.5 px,
// 0.2 % + 10 um off the bound (the plane normals are normalised with the hardware's 1-ulp reciprocal square root):
// orders of magnitude above fp32 rounding of the terms.  0 = no proof.
__device__ __forceinline__ float cam_bound2(const CamK &k, const f3 s, const int centre, const int R) {
    const f3 q = cam_point(k, s);
    const int cr = centre / k.Wd, cc = centre - cr * k.Wd;
    const float ds = (float)k.ds;
    const float hw = (float)(R + 1) * ds - 0.52f;
    const float uc = (float)cc * ds, vc = (float)cr * ds;
    float L = INFINITY;
    if (cc + R + 1 < k.Wd) { const float a = k.cx - (uc + hw); L = fminf(L, -(k.fx * q.x + a * q.z) * __builtin_amdgcn_rsqf(k.fx * k.fx + a * a)); }
    if (cc - R - 1 >= 0) { const float a = k.cx - (uc - hw); L = fminf(L, (k.fx * q.x + a * q.z) * __builtin_amdgcn_rsqf(k.fx * k.fx + a * a)); }
    if (cr + R + 1 < k.Hd) { const float a = k.cy - (vc + hw); L = fminf(L, -(k.fy * q.y + a * q.z) * __builtin_amdgcn_rsqf(k.fy * k.fy + a * a)); }
    if (cr - R - 1 >= 0) { const float a = k.cy - (vc - hw); L = fminf(L, (k.fy * q.y + a * q.z) * __builtin_amdgcn_rsqf(k.fy * k.fy + a * a)); }
    L = L * 0.998f - 1e-5f;
    return L > 0.0f ? L * L : 0.0f;  // (NaN compares false: no proof)
}

// SECOND WINDOW of the grid search, for the lanes whose first window carried no proof (`need`), in tiles with more than six of
// them -- the tiles that would take the tile-level search.
// The first window is centred on the pixel the point projected to in the PREVIOUS launch.  After the loop's large early steps
// most points sit in another cell, and in the strip the camera's motion uncovered the nearest target is two or three cells
// away: the proof fails although the neighbour is close by, and the lane would pay for the chunk-box search (a tile with more
// than six such lanes: the tile-level search, twice a proven tile's time).  So, first: a window centred on the cell the point
// projects to NOW, c' = cam_cell(cam, s), with the smallest radius R' in 1 .. 3 whose bound cam_bound2(cam, s, c', R') exceeds
// the lane's current best -- if the best IS the neighbour, that window proves it; a lane without a best, or with none inside
// radius 3, has no second window.  Its 2 R' + 1 rows are exact slot ranges from pix_start (lanewin::recentred_row: clamped as
// the planner clamps), read from the staged pool where a row lies wholly inside a staged band and from memory otherwise; the
// NW waves share every lane's sequence as in the main scan (every NW-th slot, all reads of a wave in one batch) and publish by atomicMin.
// After one barrier the proof is evaluated for (c', R'): the window was examined completely, whatever it was read from.
// Results cannot change: the key is a minimum over (distance, index) whoever finds it, the proof is cam_bound2 for a window
// examined completely, and a lane it does not prove enters the exact search with a seed at least as good as before.  (The
// covered chunks of the fallback searches stay the first window's: a subset of what was examined.)
// Block-uniform decisions: taken at all only if the tile's longest first-window sequence is at most WIN2_CAP slots (a dense
// target is refused before any request is made: a re-centred window of radius 1 holds about as many) and, with the rows'
// lengths known, if the longest re-centred sequence is (the refusals happen before / after the first of the two barriers, for
// the whole block alike).  Returns the lanes still in need; `word` receives took << 8 | refused << 9 |
// lanes proven << 16 for the counters, which the kernel adds up at its very end (window_count).  Barriers: one before the scan (the rows' ends are in LDS, and every wave has
// read the keys its first proof -- and with it this decision -- rests on), one after it.
constexpr int WIN2_CAP = 64;  // slots: 49 pixels of a radius-3 window at one target per pixel, with some room

template <int NW>
__device__ __forceinline__ bool knn_second_window(KnnShared &sh, const f3 s, const bool need, const float bd0, const int nt,
                                                  const int32_t *__restrict__ pix_start, const float *__restrict__ scan,
                                                  const int32_t *__restrict__ scan_orig, unsigned int &word) {
    using namespace lanewin;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the rows of the second window live in the last kRows2 x 64 int2 of the pool (its tail: the staged bands fill it from the
    // front, the searches' list and the epilogue's rows lie in front too) -- a tile whose bands reach that far is refused
    constexpr int W2_ELEMS = kRows2 * 64 * (int)sizeof(int2) / (int)sizeof(float4);  // pool elements the rows take
    int2 *const wrow2 = reinterpret_cast<int2 *>(sh.u.stage + 4 * (POOL - W2_ELEMS));
    const int first_len = sh.wrow[0][lane].y + sh.wrow[1][lane].y + sh.wrow[2][lane].y;
    if (wave_max_i(first_len) > WIN2_CAP || sh.band[2 * WBANDS] > POOL - W2_ELEMS) {
        word |= 0x200u;
        return need;
    }
    int c2 = 0, R2 = 0;
    float bound_new = 0.0f;
    if (need && bd0 < INFINITY) {
        c2 = cam_cell(sh.cam, s);
#pragma unroll
        for (int r = 3; r >= 1; --r) {
            const float b = cam_bound2(sh.cam, s, c2, r);
            if (bd0 * 1.0001f < b) { R2 = r; bound_new = b; }
        }
    }
    if (!__any(R2 > 0)) return need;
    // Row k's ends are requested by wave k alone, for every lane, and handed to the others through LDS: requested by every wave,
    // the fourteen loads of a lane were 8 x 14 vector-memory instructions per block, and those -- not the trips -- are what a
    // block on this path waits for (one address unit per CU).  (A lane without a second window asks for pixel 0.)  The barrier
    // is the one the scan needs anyway: behind it every wave has read the keys its first proof rests on.
    const int Wd = sh.cam.Wd, nc = sh.cam.Wd * sh.cam.Hd;
    static_assert(NW >= kRows2, "one wave per row of the re-centred window");
    if (wave < kRows2) {
        const PixRow pr = recentred_row(c2, wave, R2, Wd, nc);
        const bool have = pr.first <= pr.last;
        const int lo_raw = pix_start[have ? pr.first : 0], hi_raw = pix_start[have ? pr.last + 1 : 0];
        const int lo = min(max(lo_raw, 0), nt), hi = min(max(hi_raw, 0), nt);
        wrow2[wave * 64 + lane] = make_int2(lo, (have && hi > lo) ? hi - lo : 0);
    }
    __syncthreads();
    // the staged bands (the plan is the prologue's: first slot | pool offset or INT_MAX | length); a row wholly inside one is
    // read from the pool
    const int pl = sh.band[min(lane, 2 * WBANDS)], ps = sh.plan[min(lane, 2 * WBANDS - 1)];
    auto where = [pl, ps](const int lo, const int hi) {
        int base = LaneWin::base(lo, 0, 0x7fffffff);
#pragma unroll
        for (int q = 0; q < WBANDS; ++q) {
            const int bb = __builtin_amdgcn_readlane(pl, q), bp = __builtin_amdgcn_readlane(ps, q), bn = __builtin_amdgcn_readlane(ps, WBANDS + q);
            if (bp != 0x7fffffff && lo >= bb && hi <= bb + bn) base = LaneWin::base(lo, bb, bp);
        }
        return base;
    };
#define GS_W2_ROW(k)                                \
    const int2 w##k = wrow2[k * 64 + lane];         \
    const int n##k = w##k.y;                        \
    const int b##k = where(w##k.x, w##k.x + w##k.y);
    GS_W2_ROW(0) GS_W2_ROW(1) GS_W2_ROW(2) GS_W2_ROW(3) GS_W2_ROW(4) GS_W2_ROW(5) GS_W2_ROW(6)
#undef GS_W2_ROW
    const int p1 = n0, p2 = p1 + n1, p3 = p2 + n2, p4 = p3 + n3, p5 = p4 + n4, p6 = p5 + n5, total = p6 + n6;
    const int a0 = b0, a1 = seq_adj(b1, p1), a2 = seq_adj(b2, p2), a3 = seq_adj(b3, p3), a4 = seq_adj(b4, p4), a5 = seq_adj(b5, p5),
              a6 = seq_adj(b6, p6);
    if (wave_max_i(total) > WIN2_CAP) {
        word |= 0x200u;
        return need;
    }
    {
        float bd = INFINITY;
        int bi = 0x7fffffff;
        // Every wave takes every NW-th candidate of every lane's sequence: at most NE = WIN2_CAP / NW each.  All of them are
        // requested in ONE batch: a trip to memory for data another kernel of the step wrote costs a microsecond or more, and a
        // loop of dependent trips (measured: two reads in flight per trip, four trips for a radius-3 window) cost the block
        // 15 us -- more than the tile-level search it was meant to spare.  The branches are wave-uniform and around requests
        // only (nothing is waited for inside): a turn no lane of the wave has a candidate for, or none from memory, issues
        // nothing.  Candidates in the pool are read from LDS behind the requests.
        constexpr int NE = WIN2_CAP / NW;
        static_assert(NE * NW == WIN2_CAP, "the cap is a whole number of candidates per wave");
        const float4 *pool = reinterpret_cast<const float4 *>(sh.u.stage);
        int e[NE];
        f3 g3[NE];
        int gj[NE];
#pragma unroll
        for (int u = 0; u < NE; ++u) {
            const int p = wave + u * NW;
            e[u] = p < total ? element7(p, p1, p2, p3, p4, p5, p6, a0, a1, a2, a3, a4, a5, a6) : 0;  // (0: pool element 0, dropped)
            g3[u] = f3{0.0f, 0.0f, 0.0f};
            gj[u] = 0;
        }
#pragma unroll
        for (int u = 0; u < NE; ++u) {
            if (__any(e[u] < 0)) {
                const int slot = e[u] < 0 ? LaneWin::mem_slot(e[u]) : 0;
                g3[u] = ld3(scan, slot);
                gj[u] = scan_orig[slot];
            }
        }
#pragma unroll
        for (int u = 0; u < NE; ++u) {
            const bool has = wave + u * NW < total;
            if (!__any(has)) continue;
            const float4 ql = pool[max(e[u], 0)];
            const bool mem = e[u] < 0;
            const float4 q = make_float4(mem ? g3[u].x : ql.x, mem ? g3[u].y : ql.y, mem ? g3[u].z : ql.z, mem ? __int_as_float(gj[u]) : ql.w);
            const float d = has ? dist2(s, q.x, q.y, q.z) : INFINITY;
            const int jj = __float_as_int(q.w);
            const bool better = (d < bd) | ((d == bd) & (jj < bi));
            bd = better ? d : bd;
            bi = better ? jj : bi;
        }
        if (bd < INFINITY) atomicMin(&sh.key[lane], pack_key(bd, bi));
    }
    __syncthreads();
    float bd;
    int bi;
    key_unpack(sh.key[lane], bd, bi);
    const bool still = need & !((R2 > 0) & (bd * 1.0001f < bound_new));
    const unsigned long long before = __ballot(need), after = __ballot(still);
    word |= 0x100u | ((unsigned)(__popcll(before) - __popcll(after)) << 16);
    return still;
}

template <bool GRID, int NL, int NW>
// (NW: waves per block, 16 or 8 -- chosen by the host, loop_waves; every result is the same bit for bit: the neighbour is a
// minimum over packed keys whoever finds it, and the row sums keep their groups and their order)
// (argument order: what the first batch of requests needs comes first -- the leading sixteen dwords of the kernel arguments
// can be preloaded into SGPRs with the dispatch, -amdgpu-kernarg-preload-count in the Makefile)
__global__ __launch_bounds__(NW * 64, 2 * NW / 4) void knn1_loop_k(const LoopConst *__restrict__ C, const IcpState *__restrict__ S_in,
                                                         const float *__restrict__ partials_in, const int32_t *__restrict__ pix_ws,
                                                         const int32_t *__restrict__ cells_in, int cap, int tile_points,
                                                         int phase /* first | launch parity << 1 */, int step_mode, int look_slot,
                                                         int nblocks_in, IcpState *__restrict__ S_out, float *__restrict__ rec, int out_slot,
                                                         LoopBufs B, float *__restrict__ partials /* gridDim.x x NACC */,
                                                         const float *__restrict__ user_src) {
    static_assert(NW == 16 || NW == 8, "row groups, tile_box and the J epilogue are laid out for sixteen or eight waves");
    const int first = phase & 1, par = phase >> 1;
    __shared__ KnnShared sh;
    __shared__ IcpState st_sm;
    __shared__ float acc_sm[NACC];
    __shared__ double lu_sm[42];
    constexpr int kWords = sizeof(IcpState) / 4;
    GS_STAMP(6);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile0 = blockIdx.x * tile_points;
    const int i = tile0 + lane;
    constexpr bool grid = GRID;  // (the host launches this variant only with complete hints and camera)
    // ---- Everything whose address follows from the kernel's ARGUMENTS is requested here, in one go, before anything is
    // waited for: the state, the partial rows of the folded step, and (GRID) what the staging waves need first -- the
    // lane's own pixel (the workspace's copy of hints.src_pix: pix_ws), the pixel its point projected to in the previous
    // launch (cells_in), wave 2's seed keys and its copy of the camera constants.  Every trip to memory at kernel start costs
    // 1.5-2 us (the data was written by other XCDs' CUs).  Until round 3's last session these requests stood behind the
    // loop constants (C->ns for the bounds, C->hints.* / C->cells for the addresses: a trip of their own), the state's load
    // was waited for on the spot (another, in waves 0 and 1), and the pointers taken from the constants made FLAT loads,
    // which every later wait for a scalar load also waits for (the compiler's s_waitcnt vmcnt(0) lgkmcnt(0)): four trips in
    // a row before the first window centre was known (phase stamps: 3.2 us after kernel entry).  Now the indices are
    // clamped to the arrays' capacity (cap: all of them are the workspace's own, sized by it) instead of tested against ns.
    // No branch stands between these requests and nothing is tested on them before all are out: the compiler places a load
    // where its scheduling region first needs it, and sinks a load below a branch whose other side does not use it -- with the
    // block's early exit tested first, every request stood behind the trip for ns again.  Hence: addresses nobody needs are
    // clamped to something harmless instead of branched around; ns / nt come by a VECTOR load (lane & 1 picks) in the same
    // batch instead of the scalar load the compiler would issue only where the exit test wants it; and the empty asm below
    // names every requested value, so that none of the requests can move past it.
    __shared__ unsigned int rp_cnt;  // GRID: waves whose part of the row sums (and of the state) is in LDS (rp_finish_wave0)
    if constexpr (GRID) {
        // rp_cnt = 0 must be visible to every wave before any of them counts itself in: wave 0 waits for its LDS write, and
        // all meet at a RAW barrier (no fence needed, nothing else is in flight yet; at kernel start the waves of a block
        // arrive within ~0.1 us of each other)
        if (threadIdx.x == 0) { rp_cnt = 0; sh.plan_ready = 0; }
        if (wave == 0) __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
        __builtin_amdgcn_s_barrier();
    }
    const int ic = min(i, cap - 1);
    const int st_w = reinterpret_cast<const int *>(S_in)[min((int)threadIdx.x, kWords - 1)];
    float rp_a[RP_LOADS];
    // (consumed only if a step is folded in: then the launch has <= 512 blocks, one round; ten loads cover the 300 rows of a
    // 160 x 120 frame -- every instruction here is executed by sixteen waves on four SIMDs)
    // (NL: the host instantiates the ten-load form for launches of <= 320 blocks)
    // GRID: waves 1 and 2 (the planner and the lanes' wave: the critical path of the prologue) sum no rows; their four row
    // groups are the second duty of waves 14 and 15, which otherwise only wait for the plan.  (Same groups, same order
    // inside each: the sums do not change.)
    // NW = 8: sixteen thread groups for the 32 row groups.  GRID: the twelve outside waves 1 and 2 take groups w, w + 12 and
    // (w < 8) w + 24, w = the thread group's rank among the twelve; chunk boxes: every thread group takes g and g + 16.
    int rp_g, rp_g2, rp_g3 = -1;
    if constexpr (NW == 16) {
        rp_g = (GRID && (wave == 1 || wave == 2)) ? -1 : (int)(threadIdx.x >> 5);
        rp_g2 = (GRID && wave >= 14) ? (int)(threadIdx.x >> 5) - 26 : -1;
    } else if constexpr (GRID) {
        const int tg = threadIdx.x >> 5, w = tg < 2 ? tg : tg - 4;
        const bool sums = wave != 1 && wave != 2;
        rp_g = sums ? w : -1;
        rp_g2 = sums ? w + 12 : -1;
        rp_g3 = (sums && w < 8) ? w + 24 : -1;  // (waves 0, 3, 4, 5: wave-uniform)
    } else {
        rp_g = threadIdx.x >> 5;
        rp_g2 = rp_g + 16;
    }
    float rp_b[RP_LOADS], rp_c[RP_LOADS];
#pragma unroll
    for (int u = 0; u < RP_LOADS; ++u) { rp_a[u] = 0.0f; rp_b[u] = 0.0f; rp_c[u] = 0.0f; }
    if (rp_g >= 0) rp_issue_padded<NL>(partials_in, rp_g, rp_a);  // (wave-uniform branches around loads only: nothing is waited for inside)
    if (rp_g2 >= 0) rp_issue_padded<NL>(partials_in, rp_g2, rp_b);
    if constexpr (NW != 16 && GRID) {
        if (rp_g3 >= 0) rp_issue_padded<NL>(partials_in, rp_g3, rp_c);
    }
    static_assert(offsetof(LoopConst, nt) == offsetof(LoopConst, ns) + 4, "ns | nt are read as a pair");
    const int nn = reinterpret_cast<const int *>(&C->ns)[lane & 1];
    int e_h = 0, e_c = -1, e_cam = 0;
    unsigned long long e_k0 = 0, e_k1 = 0;
    if constexpr (GRID) {
        e_h = pix_ws[ic];
        e_c = cells_in[ic];
        // wave 2's seeds for either outcome of the step: outside tape mode the two neighbour arrays are slots 0 and 1 (which
        // of them is current is decided below, when the state has arrived); tape mode names the slots in the state
        const int ik = wave == 2 ? ic : 0;
        e_k0 = B.N(0)[ik]; e_k1 = B.N(1)[ik];
        e_cam = reinterpret_cast<const int *>(&C->cam)[min(lane, (int)(sizeof(CamK) / 4) - 1)];
        asm volatile("" ::"v"(e_h), "v"(e_c), "v"(e_cam), "v"((unsigned)e_k0), "v"((unsigned)(e_k0 >> 32)),
                     "v"((unsigned)e_k1), "v"((unsigned)(e_k1 >> 32)));
    }
    if constexpr (NW != 16 && GRID)
        asm volatile("" ::"v"(rp_c[0]), "v"(rp_c[1]), "v"(rp_c[2]), "v"(rp_c[3]), "v"(rp_c[4]), "v"(rp_c[5]), "v"(rp_c[6]), "v"(rp_c[7]), "v"(rp_c[8]),
                     "v"(rp_c[9]), "v"(rp_c[10]), "v"(rp_c[11]), "v"(rp_c[12]), "v"(rp_c[13]), "v"(rp_c[14]), "v"(rp_c[15]));
    if constexpr (GRID || NW != 16)
        asm volatile("" ::"v"(rp_b[0]), "v"(rp_b[1]), "v"(rp_b[2]), "v"(rp_b[3]), "v"(rp_b[4]), "v"(rp_b[5]), "v"(rp_b[6]), "v"(rp_b[7]), "v"(rp_b[8]),
                     "v"(rp_b[9]), "v"(rp_b[10]), "v"(rp_b[11]), "v"(rp_b[12]), "v"(rp_b[13]), "v"(rp_b[14]), "v"(rp_b[15]));
    asm volatile("" ::"v"(st_w), "v"(nn), "v"(rp_a[0]), "v"(rp_a[1]), "v"(rp_a[2]), "v"(rp_a[3]), "v"(rp_a[4]), "v"(rp_a[5]), "v"(rp_a[6]),
                 "v"(rp_a[7]), "v"(rp_a[8]), "v"(rp_a[9]), "v"(rp_a[10]), "v"(rp_a[11]), "v"(rp_a[12]), "v"(rp_a[13]), "v"(rp_a[14]),
                 "v"(rp_a[15]));
    GS_STAMP(8);  // (diagnostic build: the first batch has arrived)
    const int ns = __builtin_amdgcn_readlane(nn, 0), nt = __builtin_amdgcn_readlane(nn, 1);
    const bool ok = lane < tile_points && i < ns;
    const bool tile_live = tile0 < ns && nt > 0;
    // The launch covers the cloud's CAPACITY; blocks beyond its actual size leave at once.  Their partial rows are zeros
    // (added behind every thread's live rows by the next launch: x + 0 = x).  (Block 0 publishes the state: it always stays.)
    if (tile0 >= ns && blockIdx.x != 0) {
        if (threadIdx.x < NACC) partials[blockIdx.x * NACC + threadIdx.x] = 0.0f;
        return;
    }
    f3 e_pp{0.0f, 0.0f, 0.0f};
    unsigned long long e_ka = 0, e_kb = 0;
    if (GRID && grid && tile_live && wave != 0 && ok) {
        if (first && C->cam_ok) e_pp = ld3(user_src, i);  // (the first launch: no step is folded into it)
        if (wave == 2 && !first) {
            const int ba = S_in->b_cur;
            if (look_slot < 0) { e_ka = ba == 0 ? e_k0 : e_k1; e_kb = ba == 0 ? e_k1 : e_k0; }
            else { e_ka = B.N(ba)[i]; e_kb = B.N(look_slot)[i]; }
        }
    }

    // ---- the O(1) step is wave 0's; GRID: the other fifteen waves meanwhile work out the window of every lane and the
    // row bands of the tile, stage the bands' targets into LDS and fetch the seed for either outcome of the step.
    // Nothing of that depends on the step, so it costs the association no time.
    if (threadIdx.x < kWords) reinterpret_cast<int *>(&st_sm)[threadIdx.x] = st_w;
    if (step_mode >= 0) {
        if constexpr (GRID) {
            float v = 0.0f, v2 = 0.0f, v3 = 0.0f;
            if (rp_g >= 0) v = rp_sum_padded<NL>(rp_a);
            if (rp_g2 >= 0) v2 = rp_sum_padded<NL>(rp_b);
            if constexpr (NW != 16) {
                if (rp_g3 >= 0) v3 = rp_sum_padded<NL>(rp_c);
            }
            rp_finish_wave0<NW>(v, rp_g, v2, rp_g2, v3, rp_g3, acc_sm, &rp_cnt);  // wave 0 leaves it with acc_sm and every wave's st_sm words visible TO IT
        } else if constexpr (NW == 16) {
            rp_finish(rp_sum_padded<NL>(rp_a), acc_sm);  // ends with a barrier: st_sm and acc_sm are visible
        } else {
            rp_finish2(rp_sum_padded<NL>(rp_a), rp_sum_padded<NL>(rp_b), acc_sm);
        }
        GS_STAMP(9);  // (diagnostic build: the rows are summed)
        // (the record takes the state BEFORE the step from the global copy: wave 0 is about to change the LDS one)
        if (blockIdx.x == 0 && rec && threadIdx.x < kWords) reinterpret_cast<int *>(rec)[REC_STATE + threadIdx.x] = st_w;
    }
    if (wave == 0) {
        const bool pub = blockIdx.x == 0;  // the one block whose copy of the new state is published
        if (step_mode >= 0)
            step_wave0(&st_sm, acc_sm, step_mode, C->gp, pub ? C->trace : nullptr, pub ? C->out_T : nullptr, look_slot, pub ? rec : nullptr, lu_sm, true);
        GS_STAMP(10);  // (wave 0: the step is done)
    } else if (!grid && tile_live && !first && wave == 1) {
        // chunk-box search: the seed (the previous neighbour's target point) for either outcome of the step, fetched
        // while wave 0 computes it -- two dependent loads less on the association's critical path
        if (ok) {
            const int ba = S_in->b_cur, bb = look_slot >= 0 ? look_slot : 1 - ba;
            const unsigned long long ka = B.N(ba)[i], kb = B.N(bb)[i];
            // (one of the two arrays may never have been written -- the outcome that cannot happen: clamp as unsigned)
            const int sa = (int)min((uint32_t)(ka & 0xffffffffu), (uint32_t)(nt - 1)), sb = (int)min((uint32_t)(kb & 0xffffffffu), (uint32_t)(nt - 1));
            const f3 qa = ld3(C->tgt, sa), qb = ld3(C->tgt, sb);
            *reinterpret_cast<float4 *>(sh.seed[0][lane]) = make_float4(qa.x, qa.y, qa.z, __int_as_float(sa));
            *reinterpret_cast<float4 *>(sh.seed[1][lane]) = make_float4(qb.x, qb.y, qb.z, __int_as_float(sb));
        }
    } else if (grid && tile_live) {
        // Three roles.  Wave 1 PLANS: every lane's window centre, the displacement of the tile's majority, the tile's row
        // bands and (one trip) their slot ranges -> LDS, then a flag.  Wave 2 prepares the LANES: the seeds for either
        // outcome of the step and each lane's own window rows (its loads leave at once; the rows are packed against the plan
        // when it is there).  The other thirteen sleep until the plan is in LDS; then all fifteen stage the bands' targets.
        // Every staging wave used to derive the same plan for itself -- ~200 instructions x 15 waves on four SIMDs: the
        // issue slots, not the memory trips, were what the phase stamps showed between "first batch arrived" and "centre
        // known" (1.6 us, r04a) -- and wave 1 carried the seeds and rows on top of the plan.
        const int Wd = C->hints.grid_w, nc = C->hints.grid_w * C->hints.grid_h;
        constexpr int R = 1;
        int bbase[WBANDS], pstart[WBANDS], bcnt[WBANDS], used = 0;  // per band: first slot, pool offset (INT_MAX: not in the pool), length; pool fill
#pragma unroll
        for (int q = 0; q < WBANDS; ++q) { bbase[q] = 0; pstart[q] = 0x7fffffff; bcnt[q] = 0; }
        // Window centre: the grid pixel the point projects to.  The point itself is only known once the step (wave 0,
        // concurrently) has produced dT -- but it is within millimetres of the cloud the PREVIOUS launch wrote, whatever
        // the step decides, and that launch left the pixel of every point it wrote in C->cells (by launch parity: one
        // load at an address known at kernel start; first launch: the caller's cloud under the initial transform,
        // exactly).  The centre only selects which window is examined; the proof below is evaluated for the point's
        // actual position against it.
        const int h = ok ? min(max(e_h, 0), nc - 1) : 0;
        int c = h;
        if (wave <= 2 && ok && C->cam_ok) c = first ? cam_cell(C->cam, xform(S_in->dT, e_pp)) : min(max(e_c, 0), nc - 1);
        int row_lo[WROWS], row_hi[WROWS];
        float4 sd[2] = {make_float4(0.0f, 0.0f, 0.0f, 0.0f), make_float4(0.0f, 0.0f, 0.0f, 0.0f)};
#pragma unroll
        for (int r = 0; r < WROWS; ++r) { row_lo[r] = 0; row_hi[r] = 0; }
        if (wave == 2) {
            // the first / one-past-last slots of the lane's three window rows, and the seeds (the step leaves b_cur as it is or
            // moves it to the look-ahead's array): requested now, used when the plan is there
#pragma unroll
            for (int r = 0; r < WROWS; ++r) {
                const int g = c + (r - 1) * Wd;
                row_lo[r] = C->hints.pix_start[min(max(g - 1, 0), nc - 1)];
                row_hi[r] = C->hints.pix_start[min(max(g + 1, 0), nc - 1) + 1];
            }
            if (ok) {
                int sj[2];
                if (first) {
                    const int slot = min(max(C->hints.pix_start[h], 0), nt - 1);
                    sj[0] = sj[1] = min(max(C->hints.scan_orig[slot], 0), nt - 1);
                } else {
                    // (one of the two arrays may never have been written -- the outcome that cannot happen: clamp as unsigned)
                    sj[0] = (int)min((uint32_t)(e_ka & 0xffffffffu), (uint32_t)(nt - 1));
                    sj[1] = (int)min((uint32_t)(e_kb & 0xffffffffu), (uint32_t)(nt - 1));
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const f3 q = ld3(C->tgt, sj[u]);
                    sd[u] = make_float4(q.x, q.y, q.z, __int_as_float(sj[u]));
                }
            }
        }
        if (wave == 1) {
            // The lanes of a tile move together: their centres are their own pixels (consecutive in row-major order, also
            // across a row end) plus nearly the same displacement.  Relative to the tile's smallest displacement a lane
            // sits up to a pixel further along the row and / or one row further down (rel); what remains is contiguous
            // in row-major order again, so every row band of the tile is ONE slot range.
            // (wave reductions leave uniform values in vector registers: move them, and all that follows, to scalars)
            // The reference displacement is the MAJORITY's: a lane whose neighbour is far away (no map point near it) has a
            // centre anywhere, and taking the plain minimum would let one such lane cost the whole tile its windows.  Up to
            // three candidates (the first lanes not yet represented); supporters = lanes within a row and three columns.
            const int dsp = c - h;
            auto near = [&](int r) { return abs(r) <= 3 || abs(r - Wd) <= 3 || abs(r + Wd) <= 3; };
            const unsigned long long okm = __ballot(ok);
            unsigned long long pool = okm, sup = 0;
            for (int tries = 0; tries < 3 && pool; ++tries) {
                const int cand = __builtin_amdgcn_readlane(dsp, __builtin_ctzll(pool));
                const unsigned long long m = __ballot(ok && near(dsp - cand));
                if (__popcll(m) > __popcll(sup)) sup = m;
                if (2 * __popcll(m) >= __popcll(okm)) break;
                pool &= ~m;
            }
            GS_STAMP(13);
            const bool mine = ok && ((sup >> lane) & 1);
            const int dmin = __builtin_amdgcn_readfirstlane(wave_min_i(mine ? dsp : 0x7fffffff));
            const int e = mine ? dsp - dmin : 0;
            int rel = mine ? (e >= Wd / 2) + (e >= Wd + Wd / 2) : 2;  // rel > 1: no window (a lane that does not move with its tile)
            const bool in = mine && rel <= 1 && abs(e - rel * Wd) <= 6;
            if (!in) rel = 2;
            const int beta = c - rel * Wd;
            const int bmin = __builtin_amdgcn_readfirstlane(wave_min_i(in ? beta : 0x7fffffff));
            const int bmax = __builtin_amdgcn_readfirstlane(wave_max_i(in ? beta : (int)0x80000000));
            const bool two_rows = __any(in && rel == 1);
            // Band kk covers the pixels [bmin + (kk - R) Wd - R, bmax + (kk - R) Wd + R], kk = 0 .. 2 R (+ 1 if the lanes sit in
            // two rows), R = 1 (radius 2 = five rows, six bands was measured: ~1 us per launch more on a dense target, nothing
            // gained on a sparse one).  All first-slot loads are issued before any is used: taken one band after the other
            // they were four dependent trips through the scalar cache (2.4 us, r03h).
            int boff[WBANDS];
            {
                int lo_raw[WBANDS], hi_raw[WBANDS];
                bool want[WBANDS];
#pragma unroll
                for (int kk = 0; kk < WBANDS; ++kk) {
                    const int a = bmin + (kk - R) * Wd - R, b = bmax + (kk - R) * Wd + R;
                    want[kk] = kk <= 2 * R + (two_rows ? 1 : 0) && bmax >= bmin && b >= 0 && a <= nc - 1;
                    lo_raw[kk] = C->hints.pix_start[min(max(a, 0), nc - 1)];
                    hi_raw[kk] = C->hints.pix_start[min(max(b, 0), nc - 1) + 1];
                }
                sh.centre[lane] = c;
                sh.wflag[lane] = rel;  // (provisional: wave 2 completes it)
#pragma unroll
                for (int kk = 0; kk < WBANDS; ++kk) {
                    bbase[kk] = 0; bcnt[kk] = 0; boff[kk] = used;
                    const int lo = min(max(lo_raw[kk], 0), nt) & ~(CHUNK - 1);
                    const int hi = min((min(max(hi_raw[kk], 0), nt) + CHUNK - 1) & ~(CHUNK - 1), nt);
                    if (want[kk] && hi > lo) {
                        bbase[kk] = lo; bcnt[kk] = hi - lo;
                        // a band the pool has no room for is read from memory by the lanes themselves (slower, but the
                        // window stays complete and with it the proof): pool offset -1
                        if (used + (hi - lo) <= POOL) used += hi - lo; else boff[kk] = -1;
                    }
                }
            }
            // the plan: LDS, then the flag (release)
            if (lane < WBANDS) {
                int bb = bbase[0], bo = boff[0], bn = bcnt[0];
#pragma unroll
                for (int q = 1; q < WBANDS; ++q) { bb = lane == q ? bbase[q] : bb; bo = lane == q ? boff[q] : bo; bn = lane == q ? bcnt[q] : bn; }
                sh.band[lane] = bb; sh.band[WBANDS + lane] = bo;
                sh.plan[lane] = (bo >= 0 && bn > 0) ? bo : 0x7fffffff;
                sh.plan[WBANDS + lane] = bn;
            }
            if (lane == 0) { sh.band[2 * WBANDS] = used; sh.cnt = 0; }
            sh.key[lane] = KEY_NONE;
            if (lane == 0) __hip_atomic_store(&sh.plan_ready, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
            for (int q = 0; q < WBANDS; ++q) pstart[q] = (boff[q] >= 0 && bcnt[q] > 0) ? boff[q] : 0x7fffffff;
        } else {
            while (__hip_atomic_load(&sh.plan_ready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == 0u) __builtin_amdgcn_s_sleep(2);
            const int pl = sh.band[min(lane, 2 * WBANDS)], ps = sh.plan[min(lane, 2 * WBANDS - 1)];
#pragma unroll
            for (int q = 0; q < WBANDS; ++q) {
                bbase[q] = __builtin_amdgcn_readlane(pl, q);
                pstart[q] = __builtin_amdgcn_readlane(ps, q);
                bcnt[q] = __builtin_amdgcn_readlane(ps, WBANDS + q);
            }
            used = __builtin_amdgcn_readlane(pl, 2 * WBANDS);
        }
        GS_STAMP(14);
        // staging loads first (they are the long ones), the per-lane rows behind them
        constexpr int ST = NW * 64 - 64, NR = (POOL + ST - 1) / ST;
        float4 sreg[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int e = (int)threadIdx.x - 64 + ST * r;
            if (e < used) {
                int bb = 0, bo = 0;  // the staged band that holds pool element e: the last one that starts at or before it
#pragma unroll
                for (int q = 0; q < WBANDS; ++q) {
                    const bool here = e >= pstart[q];
                    bb = here ? bbase[q] : bb; bo = here ? pstart[q] : bo;
                }
                const int slot = bb + e - bo;
                const f3 q3 = ld3(C->hints.scan_points, slot);
                sreg[r] = make_float4(q3.x, q3.y, q3.z, __int_as_float(C->hints.scan_orig[slot]));
            }
        }
        if (wave == 2) {
            // (seeds and camera first: their nine registers are free again while the rows are worked out -- the sixteen-wave
            // form has 64 and must not spill)
            *reinterpret_cast<float4 *>(sh.seed[0][lane]) = sd[0];
            *reinterpret_cast<float4 *>(sh.seed[1][lane]) = sd[1];
            if (lane < (int)(sizeof(CamK) / 4)) reinterpret_cast<int *>(&sh.cam)[lane] = e_cam;
            const int rel = sh.wflag[lane];  // (the planner's; its centre is this wave's own c: same arithmetic on the same words)
            const bool in = rel <= 1;
            bool full = in;
#pragma unroll
            for (int r = 0; r < WROWS; ++r) {
                int packed = 0;
                int2 ex = make_int2(0, 0);
                const int g = c + (r - R) * Wd;
                if (in && r <= 2 * R && g + R >= 0 && g - R <= nc - 1) {
                    // the row's EXACT slots: the scan examines these and no others (the bands stay chunk aligned; a row is
                    // not widened to them -- LaneWin)
                    const int lo = min(max(row_lo[r], 0), nt), hi = min(max(row_hi[r], 0), nt);
                    if (hi > lo) {
                        // the row's band, from the plan in LDS (three reads behind the staging loads, which take far longer:
                        // selecting it from bbase / pstart / bcnt would keep those twelve registers alive across them)
                        const int kk = min(rel + r, WBANDS - 1);
                        const int bb = sh.band[kk], bp = sh.plan[kk], bn = sh.plan[WBANDS + kk];
                        // inside the tile's band (staged, or read from memory), or not examined (then the lane has no
                        // certificate: `full`)
                        if (lo >= bb && hi <= bb + bn) {
                            ex = make_int2(LaneWin::base(lo, bb, bp), hi - lo);
                            packed = LaneWin::pack(lo, hi, nt);
                        } else {
                            full = false;
                        }
                    }
                }
                sh.win[r][lane] = packed;
                sh.wrow[r][lane] = ex;
            }
            sh.wflag[lane] = min(rel, 2) | (full ? 4 : 0) | (R << 3);
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int e = (int)threadIdx.x - 64 + ST * r;
            if (e < used) *reinterpret_cast<float4 *>(&sh.u.stage[4 * e]) = sreg[r];
        }
        GS_STAMP(15);
    }
    __syncthreads();
    if (step_mode >= 0 && blockIdx.x == 0 && threadIdx.x < kWords) {
        const int v = reinterpret_cast<const int *>(&st_sm)[threadIdx.x];
        reinterpret_cast<int *>(S_out)[threadIdx.x] = v;
        if (rec) reinterpret_cast<int *>(rec)[REC_WORDS + REC_STATE + threadIdx.x] = v;
    }
    GS_STAMP(7);
    const IcpState *S = &st_sm;
    if (tile0 >= ns) {  // empty tile: its partial row must still be defined
        if (threadIdx.x < NACC) partials[blockIdx.x * NACC + threadIdx.x] = 0.0f;
        return;
    }
    const int p_cur = S->p_cur, b_cur = S->b_cur;
    const float *in = first ? user_src : B.P(p_cur);
    float *out = B.P(out_slot >= 0 ? out_slot : 1 - p_cur);
    unsigned long long *best = B.N(out_slot >= 0 ? out_slot : 1 - b_cur);
    f3 s{0.0f, 0.0f, 0.0f};
    if (ok) {
        s = xform(S->dT, ld3(in, i));
        if (wave == 0) st3(out, i, s);
    }
    if (nt <= 0) {
        if (ok && wave == 0) best[i] = KEY_NONE;
        if (threadIdx.x < NACC) partials[blockIdx.x * NACC + threadIdx.x] = 0.0f;
        return;
    }
    unsigned long long key;
    bool need = false;
    unsigned int win2_word = 0;  // second window: lanes still in need | took it << 8 | refused << 9 | lanes proven << 16 (window_count);
                                 // | tile-level search ran << 10: read by the diagnostic build only (slot 15)
    int rel = 2;  // grid search: the lane's centre row relative to the tile's first (0 / 1), | 4 = window fully staged
    if (grid) {
        GS_STAMP(0);
        rel = sh.wflag[lane];
        // the seed: one real candidate per lane, fetched for either outcome of the step
        if (wave == 0) {
            unsigned long long k0 = KEY_NONE;
            if (ok) {
                const int u = (first || b_cur == S_in->b_cur) ? 0 : 1;
                const float4 q = *reinterpret_cast<const float4 *>(sh.seed[u][lane]);
                k0 = pack_key(dist2(s, q.x, q.y, q.z), __float_as_int(q.w));
            }
            atomicMin(&sh.key[lane], k0);
        }
#ifdef GS_DIAG_STAMPS
        unsigned long long scan_diag = 0;  // this wave's trips through the scan loop << 8 | the tile's longest sequence << 32
#endif
        {   // Window: the lane's three rows are ONE sequence of n0 + n1 + n2 exact slots (LaneWin: no widening to chunks), and
            // every wave takes every NW-th of them, two per trip so that both candidate reads are in flight before either is
            // used.  The phase is a chain of dependent LDS round trips, not instruction bound: what counts is
            // their number.  The three (base, length) pairs come in one batch; where a candidate is read from follows from two
            // compares (lanewin::element).  Any order of examination gives the same key: a minimum over (distance, index).
            // RESULTS are what the chunk-widened scan gave.  A slot outside the lane's 3x3 pixels holds a target at distance^2
            // >= bound2 (cam_bound2), so: if the in-window best satisfies the proof below it is below every such target and
            // was the best of the widened scan too; if it does not, no such target could have satisfied it either.  The proven
            // lanes, need_mask and every path taken are the same; an unproven lane may enter the exact search with a looser
            // seed and leaves it with the same key.
            float bd = INFINITY;
            int bi = 0x7fffffff;
            const int2 w0 = sh.wrow[0][lane], w1 = sh.wrow[1][lane], w2 = sh.wrow[2][lane];
            static_assert(WROWS == 3, "the flattened scan names its three rows");
            const int total = w0.y + w1.y + w2.y;
            auto element = [&](const int p) { return lanewin::element(p, w0.y, w1.y, w0.x, w1.x, w2.x); };
            auto take = [&](const float4 q) {
                const float d = dist2(s, q.x, q.y, q.z);
                const int jj = __float_as_int(q.w);
                const bool better = (d < bd) | ((d == bd) & (jj < bi));
                bd = better ? d : bd;
                bi = better ? jj : bi;
            };
#ifdef GS_DIAG_STAMPS
            unsigned int n_iter = 0;
#endif
            const float4 *pool = reinterpret_cast<const float4 *>(sh.u.stage);
            if (!__any((w0.x | w1.x | w2.x) < 0)) {  // (an empty row's base is 0)
                for (int p = wave; p < total; p += 2 * NW) {
                    const int ea = element(p), eb = element(min(p + NW, total - 1));  // (past the end: the last one again, harmless)
                    const float4 qa = pool[ea], qb = pool[eb];
                    take(qa);
                    take(qb);
#ifdef GS_DIAG_STAMPS
                    ++n_iter;
#endif
                }
            } else {  // some band of the tile is not in the pool: its rows come straight from memory (rare: one at a time)
                for (int p = wave; p < total; p += NW) {
                    const int e = element(p);
                    float4 q;
                    if (e >= 0) {
                        q = pool[e];
                    } else {
                        const int slot = LaneWin::mem_slot(e);
                        const f3 g3 = ld3(C->hints.scan_points, slot);
                        q = make_float4(g3.x, g3.y, g3.z, __int_as_float(C->hints.scan_orig[slot]));
                    }
                    take(q);
#ifdef GS_DIAG_STAMPS
                    ++n_iter;
#endif
                }
            }
            if (ok && bd < INFINITY) atomicMin(&sh.key[lane], pack_key(bd, bi));
#ifdef GS_DIAG_STAMPS
            scan_diag = ((unsigned long long)n_iter << 8) | ((unsigned long long)(unsigned)wave_max_i(total) << 32);
#endif
        }
        __syncthreads();
        GS_STAMP(1);
        float bd;
        int bi;
        key_unpack(sh.key[lane], bd, bi);
        // proof: every target outside the window is at least sqrt(cam_bound2) away (see there); the window was examined
        // completely (rel & 4), so a best strictly inside the bound IS the nearest neighbour, tie-break included
        const float bound2 = (ok && C->cam_ok) ? cam_bound2(sh.cam, s, sh.centre[lane], rel >> 3) : 0.0f;
        const bool proven = !C->cert_off & ((rel & 4) != 0) & (bd * 1.0001f < bound2);
        need = ok & !proven;
        unsigned long long need_mask = __ballot(need);  // the same 64 lanes in every wave: block-uniform
        // diagnostic build: lanes in need | scan trips << 8 | longest sequence << 32 (each its own count, one slot: all
        // sixteen are taken -- the second window's word below shares slot 15 with the staging waves' stamp, which is safe only
        // because wave 0, the one that writes the word, runs the step and never stages)
#ifdef GS_DIAG_STAMPS
        GS_COUNT(12, (unsigned long long)__popcll(need_mask) | scan_diag);
#endif
        // The second window, for tiles with more than six lanes in need -- the tiles the tile-level search would take: 8 us on
        // a one-frame map where the second window is 3.7; for one to six lanes the point-serial search is 1.7 (measured,
        // DESIGN section 3).  A proven tile pays the branch and nothing else.  The sixteen-wave form -- the one dense targets
        // run -- never takes it: the window would be refused there anyway (ten targets per pixel: ~90 slots at radius 1), and
        // with the path compiled in its registers cost the 200-frame figures 1 to 2 % (profiles/r10f_full_ab.txt).
        if constexpr (NW == 8) {
            if (__popcll(need_mask) > 6 && C->cam_ok && !C->cert_off) {
                need = knn_second_window<NW>(sh, s, need, bd, nt, C->hints.pix_start, C->hints.scan_points, C->hints.scan_orig, win2_word);
                need_mask = __ballot(need);
            }
        }
        bool tile_search = __popcll(need_mask) > 6;
        if (!tile_search && need_mask) {
            tile_search = !knn_point_search<NW>(sh, s, need_mask, C->hints.scan_points, C->hints.scan_orig, C->boxes, C->sboxes, nt);  // ends with a barrier
        }
        if (tile_search) {
            tile_box(sh, s, need);
            __syncthreads();
            knn_prune_search<true, NW>(sh, s, ok, need, C->hints.scan_points, C->hints.scan_orig, C->boxes, C->sboxes, nt);  // ends with a barrier
        }
        if constexpr (NW == 8) win2_word |= (unsigned)__popcll(need_mask) | (tile_search ? 0x400u : 0u);
#ifdef GS_DIAG_STAMPS
        if (wave == 0) GS_COUNT(15, (unsigned long long)win2_word);  // (every block: the buffer keeps the earlier launches' words)
#endif

        GS_STAMP(2);
        key = ok ? sh.key[lane] : KEY_NONE;
        GS_STAMP(3);
        // diagnostic build: which CU the block ran on (slot 5 as knn_prune_search writes it; a proven tile never gets there)
        GS_COUNT(5, ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) << 16) |
                        ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 48));
    } else {
        int sj = -1;
        if (!first) {  // seeded from what wave 1 fetched during the step (knn_tile's -2: keys already in LDS)
            sj = -2;
            if (wave == 0) {
                unsigned long long k0 = KEY_NONE;
                if (ok) {
                    const float4 q = *reinterpret_cast<const float4 *>(sh.seed[b_cur == S_in->b_cur ? 0 : 1][lane]);
                    k0 = pack_key(dist2(s, q.x, q.y, q.z), __float_as_int(q.w));
                }
                sh.key[lane] = k0;
            }
        }
        const bool window_seed = first && C->hints.scan_points && C->hints.src_pix && C->hints.pix_start && C->hints.grid_w > 0;
        if (window_seed) sj = -2;  // seeded by knn_window_seed below (block-uniform decision)
        const float *scan = C->hints.scan_points ? C->hints.scan_points : C->tgt;
        const int32_t *scan_orig = C->hints.scan_points ? C->hints.scan_orig : nullptr;
        if (window_seed) knn_window_seed<NW>(sh, s, ok, i, C->hints, nt);
        key = knn_tile<NW>(sh, s, ok, sj, C->tgt, scan, scan_orig, C->boxes, C->sboxes, nt);
    }
    // linearise this tile straight away (J fused into K's epilogue): 29 sums over the tile's 64 points,
    // reduced through LDS by the whole block in a fixed order (two short stages instead of 29 butterflies)
    if (wave == 0) {
        if (ok) best[i] = key;
        if (grid && ok && C->cam_ok) C->cells[par * C->cells_stride + i] = cam_cell(sh.cam, s);  // where the next launch looks
        float acc[NACC];
#pragma unroll
        for (int k = 0; k < NACC; ++k) acc[k] = 0.0f;
        const Row r = make_row_from(s, ok, key, C->tgt, C->nrm, C->thresh);
        if (r.valid) accumulate_row(r, acc);
#pragma unroll
        for (int k = 0; k < NACC; ++k) sh.u.a.rows[k][lane] = acc[k];
    }
    __syncthreads();
    static_assert(NACC * 16 <= NW * 64, "the J epilogue's first stage is one pass");
    if (threadIdx.x < NACC * 16) {
        const int k = threadIdx.x >> 4, p4 = (threadIdx.x & 15) * 4;
        sh.u.a.part[k][threadIdx.x & 15] = ((sh.u.a.rows[k][p4] + sh.u.a.rows[k][p4 + 1]) + sh.u.a.rows[k][p4 + 2]) + sh.u.a.rows[k][p4 + 3];
    }
    __syncthreads();
    if (threadIdx.x < NACC) {
        float v = 0.0f;
#pragma unroll
        for (int q = 0; q < 16; ++q) v += sh.u.a.part[threadIdx.x][q];
        partials[blockIdx.x * NACC + threadIdx.x] = v;
    }
    if constexpr (GRID && NW == 8) {
        if (threadIdx.x == 0 && (win2_word & 0x300u)) window_count(win2_word);  // (behind the block's last store: nothing waits for it)
    }
}

__global__ void icp_init_state_k(IcpState *S, const float *__restrict__ init_T /* NULL = identity */, float damp) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        for (int i = 0; i < 16; ++i) {
            const float v = init_T ? init_T[i] : ((i % 5 == 0) ? 1.0f : 0.0f);
            S->T[i] = v; S->dT[i] = v;
        }
        for (int i = 0; i < 44; ++i) S->cur[i] = 0.0f;
        S->damp = damp;
        S->p_cur = 1;  // the first association writes pts[0] / best[0]
        S->b_cur = 1; S->b_first = 0;
        S->it = 0;
    }
}

// one launch for the loop's preparations: initial state (one lane), the target's chunk boxes and, per SUPER = 64
// chunks (one block), their common box -- the second level the point-serial search consults first
__global__ __launch_bounds__(SUPER * CHUNK) void icp_prepare_k(IcpState *S, const float *__restrict__ init_T, float damp,
                                                              const float *__restrict__ tgt, const int32_t *__restrict__ d_nt,
                                                              float *__restrict__ boxes, float *__restrict__ sboxes,
                                                              LoopConst lc, LoopConst *__restrict__ lc_out, float *__restrict__ part0,
                                                              float *__restrict__ part1, int rows_written, int rows_read) {
    static_assert(SUPER * CHUNK == 1024, "one block per super-box");
    // rows the loop's launches read at kernel start but never write (knn1_loop_k's unmasked row sums): zeros
    for (int q = rows_written * NACC + blockIdx.x * blockDim.x + threadIdx.x; q < rows_read * NACC; q += gridDim.x * blockDim.x) {
        part0[q] = 0.0f; part1[q] = 0.0f;
    }
    __shared__ float wb[16][6];
    if (blockIdx.x == 0 && threadIdx.x < sizeof(LoopConst) / 4) {  // the loop's constants, for its association launches
        int v = reinterpret_cast<const int *>(&lc)[threadIdx.x];
        if (threadIdx.x == offsetof(LoopConst, ns) / 4) v = *lc.d_ns;
        if (threadIdx.x == offsetof(LoopConst, nt) / 4) v = *lc.d_nt;
        if (threadIdx.x == offsetof(LoopConst, tile_points) / 4) {  // (any one thread: the loop counters of gs_loop_counts)
            atomicAdd(&g_loop_counts[0], 1u);
            if (lc.grid_variant) atomicAdd(&g_loop_counts[1], 1u);
            if (lc.tile_points != 64) atomicAdd(&g_loop_counts[2], 1u);
        }
        reinterpret_cast<int *>(lc_out)[threadIdx.x] = v;
    }
    // the loop's own copy of hints.src_pix, defined up to the cloud's capacity: the association kernel requests it at kernel
    // start by an index clamped to the capacity, before it knows ns (knn1_loop_k)
    if (lc.cells) {
        const int n = *lc.d_ns;
        int32_t *pix = lc.cells + 2 * (size_t)lc.cells_stride;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < lc.cells_stride; i += gridDim.x * blockDim.x)
            pix[i] = (i < n && lc.hints.src_pix) ? lc.hints.src_pix[i] : 0;
    }
    if (blockIdx.x == 0) {  // the bucketing camera, after the plain copy above (same words)
        __syncthreads();
        if (threadIdx.x == 0 && lc.hints.cam_pose && lc.hints.cam_K && lc.hints.ds > 0) {
            const float *T = lc.hints.cam_pose, *K = lc.hints.cam_K;
            const Cam c = make_cam(T, K);
            for (int q = 0; q < 9; ++q) lc_out->cam.R[q] = c.R[q];
            for (int q = 0; q < 3; ++q) lc_out->cam.T[q] = c.tinv[q];
            lc_out->cam.fx = K[0]; lc_out->cam.fy = K[5]; lc_out->cam.cx = K[2]; lc_out->cam.cy = K[6];
            lc_out->cam.ds = lc.hints.ds; lc_out->cam.Wd = lc.hints.grid_w; lc_out->cam.Hd = lc.hints.grid_h;
            // project_point divides (K row 0 / 1) . [x y z 1] by (K row 2) . [x y z 1]: the proof's planes assume the
            // plain pinhole form u = fx x / z + cx, v = fy y / z + cy
            const bool pinhole = K[1] == 0.0f && K[3] == 0.0f && K[4] == 0.0f && K[7] == 0.0f && K[8] == 0.0f && K[9] == 0.0f &&
                                 K[10] == 1.0f && K[11] == 0.0f && K[0] != 0.0f && K[5] != 0.0f;
            lc_out->cam_ok = pinhole ? 1 : 0;
        }
    }
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        for (int i = 0; i < 16; ++i) {
            const float v = init_T ? init_T[i] : ((i % 5 == 0) ? 1.0f : 0.0f);
            S->T[i] = v; S->dT[i] = v;
        }
        for (int i = 0; i < 44; ++i) S->cur[i] = 0.0f;
        for (int i = 0; i < 6; ++i) S->xi[i] = 0.0f;
        S->damp = damp;
        S->p_cur = 1;  // the first association writes pts[0] / best[0]
        S->b_cur = 1; S->b_first = 0;
        S->it = 0;
    }
    const int nt = *d_nt;
    const int j = blockIdx.x * (SUPER * CHUNK) + threadIdx.x;
    if (blockIdx.x * (SUPER * CHUNK) >= nt) return;
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
    // the block's box: finish the wave reduction, then the sixteen waves through LDS
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int off = 32; off >= CHUNK; off >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], off, kWave));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off, kWave));
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { wb[wave][0] = lo[0]; wb[wave][1] = lo[1]; wb[wave][2] = lo[2]; wb[wave][3] = hi[0]; wb[wave][4] = hi[1]; wb[wave][5] = hi[2]; }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = wb[0][threadIdx.x];
        for (int w = 1; w < 16; ++w) v = threadIdx.x < 3 ? fminf(v, wb[w][threadIdx.x]) : fmaxf(v, wb[w][threadIdx.x]);
        sboxes[6 * (int64_t)blockIdx.x + threadIdx.x] = v;
    }
}

__global__ void copy_best_last_k(const IcpState *__restrict__ S, LoopBufs B, const int32_t *__restrict__ d_ns,
                                 unsigned long long *__restrict__ out) {
    const unsigned long long *src = B.N(S->b_first);
    const int ns = *d_ns;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += gridDim.x * blockDim.x) out[i] = src[i];
}

}  // namespace gs
