// gs_lanewin.hpp -- range arithmetic of the grid search's per-lane window rows (knn1_loop_k<true>): pure integer functions
// with no HIP dependency, so a host program can include this header alone and check them exhaustively
// (tests/lanewin_check.cpp).  Included by gs_icp_assoc.hpp.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GS_LANEWIN_FN __host__ __device__ __forceinline__
#else
#define GS_LANEWIN_FN inline
#endif

namespace gs {
namespace lanewin {

constexpr int kChunk = 16;  // == CHUNK (gs_icp_assoc.hpp asserts it): target slots per AABB chunk

// A lane EXAMINES the exact slot range [lo, hi) of a window row, 0 <= lo <= hi <= nt.  The chunks it may call COVERED -- the
// ones the fallback searches skip for this lane -- are those whose every slot below nt lies in [lo, hi): chunk c holds the
// slots [c kChunk, min((c + 1) kChunk, nt)), so c is covered iff lo <= c kChunk and (c + 1) kChunk <= hi, or the range reaches
// nt and c is the target's last, partial chunk.  They are consecutive: [first, first + count).
struct Covered {
    int first, count;
};
GS_LANEWIN_FN Covered covered_chunks(int lo, int hi, int nt) {
    const int first = (lo + kChunk - 1) / kChunk;
    const int end = hi >= nt ? (nt + kChunk - 1) / kChunk : hi / kChunk;
    Covered c;
    c.first = first;
    c.count = (hi > lo && end > first) ? end - first : 0;
    return c;
}

// The three rows of a lane are examined as ONE sequence of n0 + n1 + n2 candidates: candidate p is element `off` of row
// `row`.  Two compares, no table.  (p < n0 + n1 + n2; empty rows are never selected.)
struct RowOff {
    int row, off;
};
GS_LANEWIN_FN RowOff locate(int p, int n0, int n1) {
    const int n01 = n0 + n1;
    RowOff r;
    r.row = (p >= n0 ? 1 : 0) + (p >= n01 ? 1 : 0);
    r.off = p - (p >= n01 ? n01 : (p >= n0 ? n0 : 0));
    return r;
}

// The same as one sum, for the scan's inner loop: given where each row's first candidate is read from (b0, b1, b2: indices into
// one array), candidate p is read from b[row] + off.  (Unsigned arithmetic: a base may carry a tag in its top bit.)
GS_LANEWIN_FN int element(int p, int n0, int n1, int b0, int b1, int b2) {
    const unsigned n01 = (unsigned)n0 + (unsigned)n1;
    const unsigned a1 = (unsigned)b1 - (unsigned)n0, a2 = (unsigned)b2 - n01;  // (loop invariant)
    return (int)((unsigned)p + ((unsigned)p >= n01 ? a2 : ((unsigned)p >= (unsigned)n0 ? a1 : (unsigned)b0)));
}

// The RE-CENTRED window of a lane whose first window carried no proof (knn_second_window): the (2R + 1) rows around the pixel
// `centre` the point projects to now, R = 1 .. 3.  Row k (0 .. 2R) is the pixels [g - R, g + R], g = centre + (k - R) Wd, clamped
// into the grid [0, nc - 1] exactly as the planner and the lanes' wave clamp the first window's rows: a row that leaves the
// grid altogether (above the first or below the last image row) is empty; at a row's end the range runs on into the
// neighbouring row instead of being cut -- a superset of the window's pixels, which is all the proof asks for.  The row's slots
// are pix_start[first] .. pix_start[last + 1).
struct PixRow {
    int first, last;  // pixels, inclusive; first > last: the row is empty
};
GS_LANEWIN_FN PixRow recentred_row(int centre, int k, int R, int Wd, int nc) {
    const int g = centre + (k - R) * Wd;
    PixRow p;
    if (R < 1 || k < 0 || k > 2 * R || g + R < 0 || g - R > nc - 1) {
        p.first = 0; p.last = -1;
        return p;
    }
    p.first = g - R < 0 ? 0 : g - R;
    p.last = g + R > nc - 1 ? nc - 1 : g + R;
    return p;
}
constexpr int kRows2 = 7;  // rows of the largest re-centred window (R = 3)

// Its rows are examined as one sequence too: with pre_k = n_0 + .. + n_(k-1) and adj_k = b_k - pre_k (b_k: where row k's first
// candidate is read from; unsigned arithmetic, a base may carry a tag in its top bit), candidate p of the sequence is read from
// p + adj_k for the LAST k with pre_k <= p (an empty row shares its pre with the next one, which then wins).  Scalars by value,
// no arrays and no references: the kernel keeps all fourteen in registers.
GS_LANEWIN_FN int seq_adj(int base, int pre) { return (int)((unsigned)base - (unsigned)pre); }
GS_LANEWIN_FN int element7(int p, int p1, int p2, int p3, int p4, int p5, int p6, int a0, int a1, int a2, int a3, int a4, int a5, int a6) {
    static_assert(kRows2 == 7, "written out");
    unsigned a = (unsigned)a0;
    a = p >= p1 ? (unsigned)a1 : a;
    a = p >= p2 ? (unsigned)a2 : a;
    a = p >= p3 ? (unsigned)a3 : a;
    a = p >= p4 ? (unsigned)a4 : a;
    a = p >= p5 ? (unsigned)a5 : a;
    a = p >= p6 ? (unsigned)a6 : a;
    return (int)((unsigned)p + a);
}

}  // namespace lanewin
}  // namespace gs
