// gs_icp_assoc.hpp -- the exact nearest-neighbour search (K) of the ICP loops: constants, packed keys, the row algebra
// the search's epilogue shares with the linearisation, and the tile search primitives up to knn_tile.  Included by icp.hip.
//
// K  The reference's association is an exact K=1 nearest-neighbour search (squared L2 accumulated
//    x->y->z in fp32 without FMA, strict '<' so the lowest index wins ties).  Three kernels compute it:
//    * knn1_brute_k (the verifier): every (source, target) pair.  FP32-VALU bound (8 flop/pair, no dense contraction
//      -> no MFMA; a |p|^2+|q|^2-2p.q matrix form would change rounding and tie-breaks).  Target points are read
//      with wave-uniform addresses, so they stream through the scalar cache into SGPRs; the launch is split over
//      (source tiles) x (target ranges) and merged with one 64-bit atomic min on the packed key dist_bits<<32 | index.
//    * knn1_box_k / knn1_loop_k<false> (chunk-box search): the same pairs, minus those that provably cannot win.
//      Target points are grouped in chunks of CHUNK = 16 consecutive points with an AABB each.  One 1024-thread
//      block serves one tile of up to 64 source points (in the loops 64, or fewer on a dense target: loop_tile_points):
//      every wave holds the same points (lane = point) and the 16 waves
//      share the target chunks -- a coarse pass (lanes = chunk boxes, against the tile's box and loosest bound), then
//      per-lane bounds ((ex^2+ey^2)+ez^2, e = per-axis gap to the box) and scans with candidates broadcast by
//      v_readlane.  Rounding is monotone and the bound uses the distance's own operation order, so bound <= distance
//      holds exactly in fp32: no epsilon, a chunk is skipped only on a STRICT '>', and the result is bit-identical to
//      the brute-force scan (lexicographic (distance, index) minimum).
//    * knn1_loop_k<true> (grid search with a geometric proof, dense targets with search hints): every point
//      examines the targets of the 3x3 ds-grid pixels around the pixel it projects to (staged in LDS); every other
//      target lies outside a pyramid through the camera centre, and the point's distance to the pyramid's faces proves
//      that the window's best is the nearest neighbour; points whose proof fails take the chunk-box search (see
//      cam_bound2 and the comment above knn1_loop_k).
#pragma once

#include <type_traits>

#include "gs_common.hpp"
#include "gs_lanewin.hpp"

namespace gs {

constexpr int KNN_T = 256;      // brute force: threads per block
constexpr int KNN_NW = 16;      // pruned search: waves per block, ALL serving the same 64 source points (knn1_box_k; the loops'
                                // association kernel takes its wave count as a template parameter NW: 16 or 8, see loop_waves)
constexpr int KNN_BT = KNN_NW * 64;
constexpr int KNN_COARSE = 512; // target points sampled by the seed pass when no seed is given
constexpr int CHUNK = 16;       // target points per AABB chunk
constexpr int WROWS = 3;        // grid search: rows of the window (radius 1; radius 2 = WROWS 5 with its six bands costs ~1 us per launch
                                // on a dense target and gains nothing on a sparse one: 22.9 against 21.1 us per launch at c2, r03f)
constexpr int WBANDS = WROWS + 1;  // row bands a tile stages at most (its lanes sit in two adjacent rows)
constexpr int SUPER = 64;       // chunks per super-box (= 1024 target points = one block of icp_prepare_k)
constexpr int KNN_LIST = 4096;  // chunk boxes handled per round (capacity of the LDS survivor list)
constexpr int NACC = 29;        // 21 (upper H) + 6 (g) + e + count
constexpr int LIN_T = 256;
constexpr int LIN_MAXB = 1024;  // max partial blocks of the stand-alone J kernel (best of 512/1024/2048 measured at 2^24 points)
constexpr unsigned long long KEY_NONE = ~0ull;

__device__ __forceinline__ unsigned long long pack_key(float d, int j) {
    return ((unsigned long long)fbits(d) << 32) | (unsigned int)j;
}
__device__ __forceinline__ float dist2(f3 s, float tx, float ty, float tz) {
    const float dx = s.x - tx, dy = s.y - ty, dz = s.z - tz;
    return (dx * dx + dy * dy) + dz * dz;  // contraction off: x->y->z, no fma
}

// ------------------------------------------------------------------ J: row algebra (shared by K's epilogue)
struct Row {
    float a[6], b;
    bool valid;
};

// reference odometry/icputils.py:203-230; every product / difference is rounded on its own
// (elementwise torch ops), so nothing here may fuse.
__device__ __forceinline__ Row make_row(const float *__restrict__ src, const float *__restrict__ tgt,
                                        const float *__restrict__ nrm, const unsigned long long *__restrict__ best,
                                        int i, int ns, float thresh) {
    Row r;
    r.valid = false;
    if (i >= ns) return r;
    const unsigned long long key = best[i];
    if (key == KEY_NONE) return r;  // no target at all
    const uint32_t j = (uint32_t)(key & 0xffffffffu);
    const float d2 = bitsf((uint32_t)(key >> 32));
    if (thresh >= 0.0f && !(d2 < thresh)) return r;  // NB squared distance vs threshold
    const f3 s = ld3(src, i), d = ld3(tgt, j), n = ld3(nrm, j);
    r.a[0] = n.x; r.a[1] = n.y; r.a[2] = n.z;
    r.a[3] = n.z * s.y - n.y * s.z;
    r.a[4] = n.x * s.z - n.z * s.x;
    r.a[5] = n.y * s.x - n.x * s.y;
    r.b = (n.x * (d.x - s.x) + n.y * (d.y - s.y)) + n.z * (d.z - s.z);
    r.valid = true;
    return r;
}

__device__ __forceinline__ void accumulate_row(const Row &r, float *acc) {
    int q = 0;
#pragma unroll
    for (int u = 0; u < 6; ++u)
#pragma unroll
        for (int v = u; v < 6; ++v) { acc[q] = __fmaf_rn(r.a[u], r.a[v], acc[q]); ++q; }
#pragma unroll
    for (int u = 0; u < 6; ++u) acc[21 + u] = __fmaf_rn(r.a[u], r.b, acc[21 + u]);
    acc[27] = __fmaf_rn(r.b, r.b, acc[27]);
    acc[28] += 1.0f;
}

// same row from values already in registers (the association kernel's epilogue)
__device__ __forceinline__ Row make_row_from(const f3 s, const bool ok, const unsigned long long key,
                                             const float *__restrict__ tgt, const float *__restrict__ nrm, float thresh) {
    Row r;
    r.valid = false;
    if (!ok || key == KEY_NONE) return r;
    const uint32_t j = (uint32_t)(key & 0xffffffffu);
    const float d2 = bitsf((uint32_t)(key >> 32));
    if (thresh >= 0.0f && !(d2 < thresh)) return r;
    const f3 d = ld3(tgt, j), n = ld3(nrm, j);
    r.a[0] = n.x; r.a[1] = n.y; r.a[2] = n.z;
    r.a[3] = n.z * s.y - n.y * s.z;
    r.a[4] = n.x * s.z - n.z * s.x;
    r.a[5] = n.y * s.x - n.x * s.y;
    r.b = (n.x * (d.x - s.x) + n.y * (d.y - s.y)) + n.z * (d.z - s.z);
    r.valid = true;
    return r;
}

// Cooperative exact search of one 64-point source tile by the NW waves of a block.  Every wave
// holds the same 64 source points (lane = point); the waves share the work over TARGET chunks:
//   seed   : one real candidate per lane (given index, or the best of a strided sample of the target)
//   coarse : lanes = chunk boxes.  A chunk survives iff the gap between ITS box and the TILE's box is not
//            above the largest seed distance of the tile: 64 boxes per wave-instruction, ~1 instruction
//            sequence per wave for a whole 19 k-point target.
//   fine   : surviving chunks are dealt round-robin to the waves; each is tested against every lane's
//            own bound (lanes = source points) and, if some lane still needs it, scanned: one coalesced
//            load of its CHUNK points, candidates broadcast with v_readlane.
// The lanes' running best lives in LDS as packed keys: waves publish improvements with ds_min_u64 and
// re-read before every fine test, so a hit found by one wave prunes the others' remaining chunks.  A
// stale read only prunes less, never wrongly.  All bounds use the distance's own operation order, so
// bound <= distance holds exactly in fp32 (monotone rounding): the result is the brute-force scan's.
constexpr int POOL = 4096;  // grid search: target points staged in LDS per tile (all window rows together): 64 KiB; two such
                             // blocks share a CU (tools/micro/coresidency.hip: up to 80 KiB each)

// the bucketing camera: rotation / translation world -> camera in project_point's layout, pinhole constants, grid
struct CamK {
    float R[9], T[3], fx, fy, cx, cy;
    int ds, Wd, Hd;
};
struct KnnShared {
    unsigned long long key[64];
    int cnt;
    float tbox[6];             // the source tile's AABB (lo.xyz, hi.xyz)
    // grid search (knn1_loop_k<true>)
    int win[WROWS][64];        // per lane: the COVERED chunks of its window rows, packed (LaneWin), from the staging waves
    int2 wrow[WROWS][64];      // per lane: the EXAMINED slots of its window rows: (LaneWin::base, length)
    int wflag[64];             // per lane: rel | full << 2 | window radius << 3
    int centre[64];            // per lane: the window's centre pixel
    CamK cam;                  // the bucketing camera (copied once per block: the proof reads it at LDS, not scalar-cache, latency)
    int band[2 * WBANDS + 1];  // staged bands: first slot x WBANDS, pool offset x WBANDS, pool fill
    int plan[2 * WBANDS];      // per band: its pool offset if it is in the pool and not empty, else INT_MAX | its length (for the staging waves)
    unsigned int plan_ready;   // set (release) by the planning wave once band / plan are written
    float seed[2][64][4];      // the seed for either outcome of the step: target point, reference index bits
    union alignas(16) {
        struct {
            int list[KNN_LIST];
            float rows[NACC][65];  // linearise epilogue: per-point products, padded against bank conflicts
            float part[NACC][16];
        } a;
        float stage[POOL * 4];  // window rows: (x, y, z, reference index bits) per target point
    } u;
};

// Counters (gs_loop_counts): what the DEVICE decided -- {loops prepared, loops whose association ran as a grid search
// (variant launched AND the target's actual count dense enough), loops cut into small tiles, tiles whose point-serial
// search overflowed its pair list and fell back to the tile-level search}.  One atomic per loop from icp_prepare_k (and
// one per overflowing tile: a rare path); tests read them to make sure a run really exercised those paths.
__device__ unsigned int g_loop_counts[4];
// Counters (gs_window_counts) of the grid search's second, re-centred window (knn_second_window): {blocks that took it, lanes it
// proved, lanes it handed on to the exact search, blocks the cap refused}.  Counted by one thread of a block on that path only,
// as the block's last instructions: an atomic to memory takes microseconds to be acknowledged, and the wave's next wait for a
// load waits for it too -- counted where the decision is taken, with every block of a launch on the path and all of them adding
// to one line, the counters cost a launch 15 to 20 us.  Hence also the stripes: a block adds to the stripe of its index
// (one 64-byte line each), the host sums them.
constexpr int WCOUNT_STRIPES = 64;
__device__ unsigned int g_window_counts[WCOUNT_STRIPES][16];
__device__ __forceinline__ void window_count(const unsigned int word /* still in need | took << 8 | refused << 9 | .. | proven << 16 */) {
    unsigned int *c = g_window_counts[blockIdx.x % WCOUNT_STRIPES];
    if (word & 0x100u) {
        atomicAdd(&c[0], 1u);
        atomicAdd(&c[1], (word >> 16) & 0xffu);
        atomicAdd(&c[2], word & 0xffu);
    } else {
        atomicAdd(&c[3], 1u);
    }
}

#ifdef GS_DIAG_STAMPS
// Diagnostic build only (libgradslam_hip_diag.so, never loaded by the product): per-wave phase stamps.  A block owns
// KNN_NW = 16 wave slots whatever its wave count (an eight-wave block leaves slots 8 .. 15 at zero).
__device__ unsigned long long *g_diag = nullptr;
#define GS_STAMP(slot)                                                                                   \
    do {                                                                                                 \
        if (g_diag && (threadIdx.x & 63) == 0)                                                           \
            g_diag[((size_t)blockIdx.x * KNN_NW + (threadIdx.x >> 6)) * 16 + (slot)] = wall_clock64();   \
    } while (0)
#define GS_COUNT(slot, v)                                                                                \
    do {                                                                                                 \
        if (g_diag && (threadIdx.x & 63) == 0)                                                           \
            g_diag[((size_t)blockIdx.x * KNN_NW + (threadIdx.x >> 6)) * 16 + (slot)] = (v);             \
    } while (0)
#define GS_TICK(var) const unsigned int var = (unsigned int)wall_clock64()
#define GS_ACCUM(acc, t0) acc += (unsigned int)wall_clock64() - (t0)
#else
#define GS_STAMP(slot)
#define GS_COUNT(slot, v)
#define GS_TICK(var)
#define GS_ACCUM(acc, t0)
#endif

// (rlane, dpp_i and the float reductions wave_min_f / wave_max_f: gs_common.hpp)
template <class Op>
__device__ __forceinline__ int wave_reduce_i(int v, Op op) {
    v = op(v, dpp_i<0xB1>(v));
    v = op(v, dpp_i<0x4E>(v));
    v = op(v, dpp_i<0x141>(v));
    v = op(v, dpp_i<0x140>(v));
    return op(op(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
              op(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// Test the n (<= 64) target points held one per lane in (px,py,pz) with target index pj against the
// lane's source point s; branch-free (distance, index) lexicographic update.
__device__ __forceinline__ void scan_held(const f3 s, const float px, const float py, const float pz, const int pj,
                                          const int n, float &bd, int &bi) {
    for (int k = 0; k < n; ++k) {
        const float d = dist2(s, rlane(px, k), rlane(py, k), rlane(pz, k));
        const int j = __builtin_amdgcn_readlane(pj, k);
        const bool better = (d < bd) | ((d == bd) & (j < bi));
        bd = better ? d : bd;
        bi = better ? j : bi;
    }
}

__device__ __forceinline__ void key_unpack(unsigned long long k, float &bd, int &bi) {
    bd = (k == KEY_NONE) ? INFINITY : bitsf((uint32_t)(k >> 32));
    bi = (k == KEY_NONE) ? 0x7fffffff : (int)(uint32_t)(k & 0xffffffffu);
}

// First association with pixel hints: every lane looks at the targets bucketed on the (2R+1)^2 ds-grid
// pixels around its own pixel (scan order = pixel order, pix_start = first slot per pixel), the window
// pixels shared over the waves.  A projective guess used as a SEED only: it hands the exact search a bound
// that is already the true nearest distance for almost every lane.
template <int NW>
__device__ __forceinline__ void knn_window_seed(KnnShared &sh, const f3 s, const bool ok, const int i,
                                                const gs_icp_hints &h, const int nt) {
    constexpr int R = 2, WIN = (2 * R + 1) * (2 * R + 1), CAP = 4;  // at most CAP targets per window pixel
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave == 0) sh.key[lane] = KEY_NONE;
    __syncthreads();
    float bd = INFINITY;
    int bi = 0x7fffffff;
    const int npix = h.grid_w * h.grid_h;
    const int p = ok ? min(max(h.src_pix[i], 0), npix - 1) : 0;
    const int pr = p / h.grid_w, pc = p - pr * h.grid_w;
    for (int wdx = wave; wdx < WIN; wdx += NW) {
        const int rr = pr + wdx / (2 * R + 1) - R, cc = pc + wdx % (2 * R + 1) - R;
        if (!ok || rr < 0 || rr >= h.grid_h || cc < 0 || cc >= h.grid_w) continue;
        const int q0 = rr * h.grid_w + cc;
        const int s0 = h.pix_start[q0], s1 = min(h.pix_start[q0 + 1], s0 + CAP);
        for (int slot = s0; slot < s1; ++slot) {
            const f3 q = ld3(h.scan_points, slot);
            const int oj = h.scan_orig[slot];
            const float d = dist2(s, q.x, q.y, q.z);
            const bool better = (d < bd) | ((d == bd) & (oj < bi));
            bd = better ? d : bd;
            bi = better ? oj : bi;
        }
    }
    if (wave == 0 && ok && bd == INFINITY) {  // empty window: the next target in pixel order is a valid seed
        const int slot = min(max(h.pix_start[p], 0), nt - 1);
        const f3 q = ld3(h.scan_points, slot);
        bd = dist2(s, q.x, q.y, q.z);
        bi = h.scan_orig[slot];
    }
    if (ok && bd < INFINITY) atomicMin(&sh.key[lane], pack_key(bd, bi));
    __syncthreads();
}

// The source tile's box over the lanes selected by `act`: one wave per component, published through LDS
// (the caller synchronises before reading sh.tbox).
__device__ __forceinline__ void tile_box(KnnShared &sh, const f3 s, const bool act) {  // (waves 1 .. 6: any block of >= 7 waves)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave >= 1 && wave <= 6) {
        const int a = wave - 1;
        const float v = (a % 3 == 0) ? s.x : ((a % 3 == 1) ? s.y : s.z);
        const float r = (a < 3) ? wave_min_f(act ? v : INFINITY) : wave_max_f(act ? v : -INFINITY);
        if (lane == 0) sh.tbox[a] = r;
    }
}

// Per-lane window rows of the grid search, in two descriptions (written by wave 2 of knn1_loop_k<true>):
//   examined (sh.wrow): the EXACT slot range [lo, hi) of the row's three pixels, pix_start[g - 1] .. pix_start[g + 2) -- what the
//                       window scan looks at;
//   covered  (sh.win):  the chunks that lie WHOLLY inside that range (lanewin::covered_chunks) -- what the fallback searches
//                       skip for this lane (covers), chunk-granular because they deal in chunk boxes.
// INVARIANT: examined set >= the slots of the lane's 3x3 window pixels (the proof's premise), and covered set <= examined set
// (a chunk is skipped for a lane only if that lane really looked at all of it).  A chunk examined in part is examined again by
// the fallback: harmless, the key is a minimum.
struct LaneWin {
    static_assert(lanewin::kChunk == CHUNK, "gs_lanewin.hpp states the chunk size for host programs");
    // covered, per window row: first chunk << 9 | number of chunks; 0 = none.  (Nine bits: a longer run is cut to 511 chunks --
    // a subset of the examined set still.)
    __device__ __forceinline__ static int pack(int lo, int hi, int nt) {
        const lanewin::Covered c = lanewin::covered_chunks(lo, hi, nt);
        return c.count > 0 ? (c.first << 9) | min(c.count, 511) : 0;
    }
    // examined, per window row: where its first slot is read from -- its element of the LDS pool (>= 0), or, when the row's band
    // is not in the pool and the candidates come from memory, its slot with the top bit set (< 0)
    __device__ __forceinline__ static int base(int lo, int band_lo, int pool_off /* INT_MAX: not in the pool */) {
        return pool_off != 0x7fffffff ? pool_off + (lo - band_lo) : (int)((unsigned)lo | 0x80000000u);
    }
    __device__ __forceinline__ static int mem_slot(int element) { return element & 0x7fffffff; }  // of an element < 0
    // do the covered chunks of point `who` (sh.win) include the chunk that starts at `slot`?
    __device__ __forceinline__ static bool covers(const KnnShared &sh, int who, int slot) {
        const int c = slot / CHUNK;
        // (the empty asm ties the LDS reads to this call: hoisted out of the search loops the rows would cost the
        // registers that decide whether two blocks share a CU; a few LDS reads per box test are cheap on this rare path)
        asm volatile("" : "+v"(who));
        bool in = false;
#pragma unroll
        for (int r = 0; r < WROWS; ++r) {
            const int w = sh.win[r][who];
            in |= (unsigned)(c - (w >> 9)) < (unsigned)(w & 511);
        }
        return in;
    }
};
__device__ __forceinline__ int wave_min_i(int v) {
    return wave_reduce_i(v, [](int a, int b) { return min(a, b); });
}
__device__ __forceinline__ int wave_max_i(int v) {
    return wave_reduce_i(v, [](int a, int b) { return max(a, b); });
}
__device__ __forceinline__ int sel4(int k, int a0, int a1, int a2, int a3) { return k == 0 ? a0 : (k == 1 ? a1 : (k == 2 ? a2 : a3)); }

// Exact search over the chunk boxes for the lanes selected by `act`, seeded by sh.key (tile box in sh.tbox, both
// visible): coarse pass with the tile's box and loosest bound, fine pass with per-lane bounds (see knn_tile).
// GRID: chunks inside a lane's own window `win` were examined already and are skipped for that lane.
// Ends with a barrier.
template <bool GRID, int NW>
__device__ __forceinline__ void knn_prune_search(KnnShared &sh, const f3 s, const bool ok, const bool act,
                                                 const float *__restrict__ scan, const int32_t *__restrict__ scan_orig,
                                                 const float *__restrict__ boxes, const float *__restrict__ sboxes /* or NULL */,
                                                 const int nt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int n_scanned = 0;
    // the tile's box (from LDS) and its loosest bound (same 64 points in every wave -> same value)
    float bd0;
    int bi0;
    key_unpack(sh.key[lane], bd0, bi0);
    const float tlx = sh.tbox[0], tly = sh.tbox[1], tlz = sh.tbox[2];
    const float thx = sh.tbox[3], thy = sh.tbox[4], thz = sh.tbox[5];
    const float bdmax = wave_max_f(act ? bd0 : 0.0f);

    const int nchunks = (nt + CHUNK - 1) / CHUNK;
#ifdef GS_DIAG_STAMPS
    unsigned int t_coarse = 0, t_fine = 0, t_bar = 0, n_tested = 0;
#endif
    for (int r0 = 0; r0 < nchunks; r0 += KNN_LIST) {
        if (threadIdx.x == 0) sh.cnt = 0;
        __syncthreads();
        GS_TICK(tc0);
        const int r1 = min(nchunks, r0 + KNN_LIST);
        // coarse: lanes = chunk boxes; box-to-box gap with the distance's accumulation order
        for (int c0 = r0 + wave * 64; c0 < r1; c0 += NW * 64) {
            if (sboxes) {
                // the 64 chunks of this round are one super-box (c0 is a multiple of SUPER): its box contains theirs, so
                // its gap to the tile's box is, axis by axis, at most theirs and -- same operation order, monotone
                // rounding -- its bound at most each of theirs: above the tile's loosest bound, all 64 are pruned at once
                static_assert(SUPER == 64 && KNN_LIST % SUPER == 0, "one coarse round = one super-box");
                const float *b = sboxes + 6 * (int64_t)__builtin_amdgcn_readfirstlane(c0 / SUPER);
                const float ex = fmaxf(fmaxf(b[0] - thx, tlx - b[3]), 0.0f);
                const float ey = fmaxf(fmaxf(b[1] - thy, tly - b[4]), 0.0f);
                const float ez = fmaxf(fmaxf(b[2] - thz, tlz - b[5]), 0.0f);
                const float lbs = (ex * ex + ey * ey) + ez * ez;
                if (!(lbs <= bdmax)) continue;
            }
            const int c = c0 + lane;
            bool pass = false;
            if (c < r1) {
                const float *b = boxes + 6 * (int64_t)c;
                const float ex = fmaxf(fmaxf(b[0] - thx, tlx - b[3]), 0.0f);
                const float ey = fmaxf(fmaxf(b[1] - thy, tly - b[4]), 0.0f);
                const float ez = fmaxf(fmaxf(b[2] - thz, tlz - b[5]), 0.0f);
                const float lbt = (ex * ex + ey * ey) + ez * ez;
                pass = lbt <= bdmax;
            }
            const unsigned long long m = __ballot(pass);
            if (m) {
                int base = 0;
                if (lane == 0) base = atomicAdd(&sh.cnt, __popcll(m));
                base = __builtin_amdgcn_readfirstlane(base);
                if (pass) sh.u.a.list[base + __popcll(m & ((1ull << lane) - 1ull))] = c;
            }
        }
        GS_ACCUM(t_coarse, tc0);
        GS_TICK(tb0);
        __syncthreads();
        GS_ACCUM(t_bar, tb0);
        GS_TICK(tf0);
        // fine: survivors dealt round-robin to the waves, handled four at a time: ONE round of loads
        // brings the boxes and the 4 x CHUNK candidate points of a group into registers (lane l holds
        // point l%CHUNK of the group's survivor l/CHUNK), then tests and scans run without memory ops
        const int nlist = sh.cnt;
        const int ni = (nlist > wave) ? (nlist - wave + NW - 1) / NW : 0;
        constexpr int SEG = 64 / CHUNK;
        for (int g = 0; g < ni; g += SEG) {
            const int seg = lane / CHUNK, idx = g + seg;
            const bool have = idx < ni;
            const int c = have ? sh.u.a.list[wave + NW * idx] : 0;
            const int j = c * CHUNK + (lane % CHUNK);
            const bool pv = have && j < nt;
            const f3 q = pv ? ld3(scan, j) : f3{0.0f, 0.0f, 0.0f};
            const int pj = pv ? (scan_orig ? scan_orig[j] : j) : 0x7fffffff;
            float b0 = 0, b1 = 0, b2 = 0, b3 = 0, b4 = 0, b5 = 0;
            if (have) {
                const float *b = boxes + 6 * (int64_t)c;
                b0 = b[0]; b1 = b[1]; b2 = b[2]; b3 = b[3]; b4 = b[4]; b5 = b[5];
            }
            const int ng = min(SEG, ni - g);
            for (int sg = 0; sg < ng; ++sg) {
                const int l0 = sg * CHUNK;
                float bd;
                int bi;
                key_unpack(sh.key[lane], bd, bi);
                const float ex = fmaxf(fmaxf(rlane(b0, l0) - s.x, s.x - rlane(b3, l0)), 0.0f);
                const float ey = fmaxf(fmaxf(rlane(b1, l0) - s.y, s.y - rlane(b4, l0)), 0.0f);
                const float ez = fmaxf(fmaxf(rlane(b2, l0) - s.z, s.z - rlane(b5, l0)), 0.0f);
                const float lb = (ex * ex + ey * ey) + ez * ez;
                const int cc = __builtin_amdgcn_readlane(c, l0);
                bool hit;
                if (GRID) {
                    const bool live = act & !LaneWin::covers(sh, lane, cc * CHUNK);  // not examined by this lane yet
                    hit = live & (lb <= bd);
                } else {
                    hit = act & (lb <= bd);
                }
                // skip the chunk iff EVERY lane's bound is strictly above its best
                if (!__any(hit)) continue;
                const int m = min(CHUNK, nt - cc * CHUNK);
                const float bdp = bd;
                const int bip = bi;
                for (int k = 0; k < m; ++k) {
                    const float d = dist2(s, rlane(q.x, l0 + k), rlane(q.y, l0 + k), rlane(q.z, l0 + k));
                    const int jj = __builtin_amdgcn_readlane(pj, l0 + k);
                    const bool better = (d < bd) | ((d == bd) & (jj < bi));
                    bd = better ? d : bd;
                    bi = better ? jj : bi;
                }
                if (ok && (bd < bdp || bi < bip)) atomicMin(&sh.key[lane], pack_key(bd, bi));
                ++n_scanned;
            }
#ifdef GS_DIAG_STAMPS
            n_tested += ng;
#endif
        }
        GS_ACCUM(t_fine, tf0);
        GS_TICK(tb1);
        __syncthreads();
        GS_ACCUM(t_bar, tb1);
    }
    GS_COUNT(8, (unsigned long long)t_coarse);
    GS_COUNT(9, (unsigned long long)t_fine);
    GS_COUNT(10, (unsigned long long)t_bar);
    GS_COUNT(11, (unsigned long long)n_tested);
    GS_COUNT(4, (unsigned long long)n_scanned);
    // diagnostic build: survivors of the last round | HW_ID << 16 | XCC_ID << 48 (which CU the block ran on)
    GS_COUNT(5, (unsigned long long)sh.cnt | ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) << 16) |
                    ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 48));
    (void)n_scanned;
}

// Exact search for a FEW points of the tile (bits of `need_mask`) by the whole block, two phases:
//   A  lanes = super-boxes (SUPER chunks each): every point is tested against all of them with its own bound; a
//      survivor becomes a (point, super-box) pair in the LDS list, the others bound the point's certificate radius;
//   B  the pairs are dealt round-robin to the waves: lanes = the super-box's chunks, tested against the point's
//      bound (chunks inside its window are skipped), survivors scanned at once, four per round, lanes = candidates.
// For one or two stragglers this costs a fraction of the tile-level search -- what a converging loop needs once nearly
// every proof holds.  sh.cnt must be zero on entry (all waves past their last use of the
// list's storage); ends with a barrier.  Returns false (block-uniform) when the pair list overflowed: nothing found is
// final then and the caller must search again with knn_prune_search<true>.
template <int NW>
__device__ __forceinline__ bool knn_point_search(KnnShared &sh, const f3 s, const unsigned long long need_mask,
                                                 const float *__restrict__ scan, const int32_t *__restrict__ scan_orig,
                                                 const float *__restrict__ boxes, const float *__restrict__ sboxes, const int nt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nchunks = (nt + CHUNK - 1) / CHUNK, nsb = (nchunks + SUPER - 1) / SUPER;
    for (unsigned long long rest = need_mask; rest; rest &= rest - 1) {  // phase A
        const int L = __builtin_ctzll(rest);
        const float px = rlane(s.x, L), py = rlane(s.y, L), pz = rlane(s.z, L);
        float bd;
        int bi;
        key_unpack(sh.key[L], bd, bi);  // wave-uniform
        for (int b0 = wave * 64; b0 < nsb; b0 += NW * 64) {
            const int sb = b0 + lane;
            bool hit = false;
            if (sb < nsb) {
                const float *b = sboxes + 6 * (int64_t)sb;
                const float ex = fmaxf(fmaxf(b[0] - px, px - b[3]), 0.0f);
                const float ey = fmaxf(fmaxf(b[1] - py, py - b[4]), 0.0f);
                const float ez = fmaxf(fmaxf(b[2] - pz, pz - b[5]), 0.0f);
                const float lb = (ex * ex + ey * ey) + ez * ez;
                hit = lb <= bd;
            }
            const unsigned long long m = __ballot(hit);
            if (m) {
                int base = 0;
                if (lane == 0) base = atomicAdd(&sh.cnt, __popcll(m));
                base = __builtin_amdgcn_readfirstlane(base);
                const int at = base + __popcll(m & ((1ull << lane) - 1ull));
                if (hit && at < KNN_LIST) sh.u.a.list[at] = (L << 24) | sb;
            }
        }
    }
    __syncthreads();
    // The list holds KNN_LIST (point, super-box) pairs IN TOTAL -- ~680 super-boxes (700 k targets) per point for six
    // points.  A far-away straggler (huge bound: every super-box passes) on a large target overflows it; which pairs
    // were dropped would depend on the atomics' arrival order, so nothing of this attempt is used: the caller runs the
    // tile-level search for these points instead (block-uniform decision).
    if (sh.cnt > KNN_LIST) {
        if (threadIdx.x == 0) atomicAdd(&g_loop_counts[3], 1u);
        __syncthreads();  // every wave has read sh.cnt before the caller's next search resets it
        return false;
    }
    const int npairs = sh.cnt;
    for (int pi = wave; pi < npairs; pi += NW) {  // phase B
        const int pr = sh.u.a.list[pi];
        const int L = pr >> 24, sb = pr & 0xffffff;
        const f3 p{rlane(s.x, L), rlane(s.y, L), rlane(s.z, L)};
        float bd;
        int bi;
        key_unpack(sh.key[L], bd, bi);
        const int c = sb * SUPER + lane;
        bool hit = false;
        if (c < nchunks && !LaneWin::covers(sh, L, c * CHUNK)) {
            const float *b = boxes + 6 * (int64_t)c;
            const float ex = fmaxf(fmaxf(b[0] - p.x, p.x - b[3]), 0.0f);
            const float ey = fmaxf(fmaxf(b[1] - p.y, p.y - b[4]), 0.0f);
            const float ez = fmaxf(fmaxf(b[2] - p.z, p.z - b[5]), 0.0f);
            const float lb = (ex * ex + ey * ey) + ez * ez;
            hit = lb <= bd;
        }
        unsigned long long hits = __ballot(hit);
        while (hits) {  // four surviving chunks per round: lane l takes candidate l % CHUNK of the (l / CHUNK)-th of them
            constexpr int SEG = 64 / CHUNK;
            int cc = -1;
#pragma unroll
            for (int q = 0; q < SEG; ++q) {
                const int b0 = hits ? __builtin_ctzll(hits) : -1;
                if (hits) hits &= hits - 1;
                if (lane / CHUNK == q) cc = b0;
            }
            unsigned long long k = KEY_NONE;
            if (cc >= 0) {
                const int j = (sb * SUPER + cc) * CHUNK + (lane % CHUNK);
                if (j < nt) {
                    const f3 q = ld3(scan, j);
                    const float d = dist2(p, q.x, q.y, q.z);
                    k = pack_key(d, scan_orig ? scan_orig[j] : j);
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long o = __shfl_xor(k, off, kWave);
                k = o < k ? o : k;
            }
            if (k < pack_key(bd, bi)) {  // wave-uniform
                if (lane == 0) atomicMin(&sh.key[L], k);
                key_unpack(k, bd, bi);
            }
        }
    }
    __syncthreads();
    return true;
}

// returns the packed key of lane's point (KEY_NONE when there is no target)
// tgt      : target points in REFERENCE order (seeds are reference indices; so are the returned ones)
// scan     : the same points in the order they are scanned (== tgt when scan_orig is NULL); boxes are
//            built over this order
// scan_orig: reference index of every scan slot, or NULL
template <int NW>
__device__ __forceinline__ unsigned long long knn_tile(KnnShared &sh, const f3 s, const bool ok, const int seed_j,
                                                       const float *__restrict__ tgt, const float *__restrict__ scan,
                                                       const int32_t *__restrict__ scan_orig,
                                                       const float *__restrict__ boxes, const float *__restrict__ sboxes,
                                                       const int nt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    GS_STAMP(0);
    if (wave == 0 && seed_j != -2) {  // -2: keys already seeded in LDS by knn_window_seed
        unsigned long long k0 = KEY_NONE;
        if (ok && seed_j >= 0) {
            const f3 q = ld3(tgt, seed_j);
            k0 = pack_key(dist2(s, q.x, q.y, q.z), seed_j);
        }
        sh.key[lane] = k0;
    }
    tile_box(sh, s, ok);
    __syncthreads();
    if (seed_j == -1) {
        // seed pass 1: a strided sample of KNN_COARSE target points, 16 per wave and step (uniform broadcast)
        const int M = min(nt, KNN_COARSE);
        const float stride = (float)nt / (float)M;
        float bd = INFINITY;
        int bi = 0x7fffffff;
        for (int k0 = wave * 16; k0 < M; k0 += NW * 16) {
            const int k = k0 + lane;
            const int n = min(16, M - k0);
            const int j = min((int)((float)k * stride), nt - 1);
            const f3 q = (lane < n) ? ld3(scan, j) : f3{0.0f, 0.0f, 0.0f};
            const int oj = (scan_orig && lane < n) ? scan_orig[j] : j;
            scan_held(s, q.x, q.y, q.z, oj, n, bd, bi);
        }
        if (ok && bd < INFINITY) atomicMin(&sh.key[lane], pack_key(bd, bi));
        __syncthreads();
        if (scan_orig == nullptr) {
        // seed pass 2: clouds are image ordered, so index neighbours of the best sample are spatial
        // neighbours: each lane refines over [j*-R, j*+R) of ITS sample, the waves split the offsets
        constexpr int R = 64;
        key_unpack(sh.key[lane], bd, bi);
        const int jstar = bi;
        for (int t = 0; t < 2 * R / NW; ++t) {
            const int j = min(max(jstar - R + wave * (2 * R / NW) + t, 0), nt - 1);
            const f3 q = ok ? ld3(tgt, j) : f3{0.0f, 0.0f, 0.0f};
            const float d = dist2(s, q.x, q.y, q.z);
            const bool better = (d < bd) | ((d == bd) & (j < bi));
            bd = better ? d : bd;
            bi = better ? j : bi;
        }
        if (ok && bi != jstar) atomicMin(&sh.key[lane], pack_key(bd, bi));
        __syncthreads();
        }
    }
    GS_STAMP(1);
    knn_prune_search<false, NW>(sh, s, ok, ok, scan, scan_orig, boxes, sboxes, nt);
    GS_STAMP(2);
    GS_STAMP(3);
    return ok ? sh.key[lane] : KEY_NONE;
}

}  // namespace gs
