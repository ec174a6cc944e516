// gs_lanewin.hpp -- range arithmetic of the grid search's per-lane window rows (knn1_loop_k<true>): pure integer functions
// with no HIP dependency, so a host program can include this header alone and check them exhaustively
// (tests/lanewin_check.cpp).  Included by gs_icp_assoc.hpp.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GS_LANEWIN_FN __host__ __device__ inline
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

}  // namespace lanewin
}  // namespace gs
