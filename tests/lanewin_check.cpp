// Exhaustive host check of gs_lanewin.hpp (the range arithmetic of the grid search's window rows).  Stand-alone: includes that
// header only.  Built and run by tests/test_lanewin_host.py with -fsanitize=address,undefined.
//   covered_chunks: for every target size nt in 1 .. 80 and every 0 <= lo <= hi <= nt, a chunk is reported as covered iff every
//                   slot it holds (below nt) lies in [lo, hi) -- i.e. the reported set is sound AND the largest such set;
//   locate/element: for every (n0, n1, n2) in 0 .. 20, every p < n0 + n1 + n2 maps to exactly one (row, offset) with
//                   offset < n[row], every (row, offset) is hit once, and element() is base[row] + offset, tagged bases included.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gs_lanewin.hpp"

namespace lw = gs::lanewin;

#define CHECK(cond, ...)                              \
    do {                                              \
        if (!(cond)) {                                \
            std::fprintf(stderr, "FAILED %s: ", #cond); \
            std::fprintf(stderr, __VA_ARGS__);        \
            std::fprintf(stderr, "\n");               \
            std::exit(1);                             \
        }                                             \
    } while (0)

int main() {
    long cases = 0;
    for (int nt = 1; nt <= 80; ++nt) {
        const int nchunks = (nt + lw::kChunk - 1) / lw::kChunk;
        for (int lo = 0; lo <= nt; ++lo) {
            for (int hi = lo; hi <= nt; ++hi) {
                const lw::Covered c = lw::covered_chunks(lo, hi, nt);
                CHECK(c.count >= 0 && c.first >= 0, "nt %d lo %d hi %d", nt, lo, hi);
                CHECK(c.count == 0 || c.first + c.count <= nchunks, "nt %d lo %d hi %d: chunk past the target", nt, lo, hi);
                for (int k = 0; k < nchunks; ++k) {
                    const int a = k * lw::kChunk, b = (k + 1) * lw::kChunk < nt ? (k + 1) * lw::kChunk : nt;  // the chunk's slots
                    const bool inside = lo <= a && b <= hi;  // (a < b: the chunk holds a slot)
                    const bool reported = k >= c.first && k < c.first + c.count;
                    // sound: reported -> wholly inside (ends at hi, or at nt for the last partial chunk); largest: inside -> reported
                    CHECK(reported == inside, "nt %d lo %d hi %d chunk %d: reported %d, wholly inside %d", nt, lo, hi, k, (int)reported,
                          (int)inside);
                }
                ++cases;
            }
        }
    }
    for (int n0 = 0; n0 <= 20; ++n0)
        for (int n1 = 0; n1 <= 20; ++n1)
            for (int n2 = 0; n2 <= 20; ++n2) {
                const int n[3] = {n0, n1, n2};
                // bases: two pool rows and one row read from memory (top bit set), placed so that sums wrap around
                const int base[3] = {7, 0, (int)(0x80000000u | 3u)};
                std::vector<int> hits[3] = {std::vector<int>(n0, 0), std::vector<int>(n1, 0), std::vector<int>(n2, 0)};
                for (int p = 0; p < n0 + n1 + n2; ++p) {
                    const lw::RowOff ro = lw::locate(p, n0, n1);
                    CHECK(ro.row >= 0 && ro.row < 3, "n %d %d %d p %d: row %d", n0, n1, n2, p, ro.row);
                    CHECK(ro.off >= 0 && ro.off < n[ro.row], "n %d %d %d p %d: row %d offset %d", n0, n1, n2, p, ro.row, ro.off);
                    ++hits[ro.row][ro.off];
                    const int e = lw::element(p, n0, n1, base[0], base[1], base[2]);
                    const int want = (int)((unsigned)base[ro.row] + (unsigned)ro.off);
                    CHECK(e == want, "n %d %d %d p %d: element %d, base + offset %d", n0, n1, n2, p, e, want);
                    CHECK((e < 0) == (ro.row == 2), "n %d %d %d p %d: the tag of row 2's base is lost", n0, n1, n2, p);
                }
                for (int r = 0; r < 3; ++r)
                    for (int o = 0; o < n[r]; ++o) CHECK(hits[r][o] == 1, "n %d %d %d: (row %d, offset %d) hit %d times", n0, n1, n2, r, o, hits[r][o]);
                ++cases;
            }
    std::printf("lanewin_check: %ld cases passed\n", cases);
    return 0;
}
