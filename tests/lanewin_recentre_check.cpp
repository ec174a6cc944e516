// Exhaustive host check of the re-centred window's index helpers in gs_lanewin.hpp (knn_second_window's rows).  Stand-alone:
// includes that header only.  Built and run by tests/test_lanewin_recentre_host.py with -fsanitize=address,undefined.
//   recentred_row: for every grid Wd x Hd in 1 .. 9 x 1 .. 7, every centre pixel, every radius R in 1 .. 3 and every row k in
//                  -1 .. 2R + 1: the reported pixel range equals a naive enumeration (the pixels g - R .. g + R, g = centre +
//                  (k - R) Wd, each clamped into [0, nc - 1]; nothing when all of them lie on one side of the grid or k is no
//                  row of the window), stays inside the grid, and the union over the rows holds every pixel (r, c) of the
//                  grid with |r - centre row| <= R and |c - centre column| <= R -- the premise of the proof (cam_bound2);
//   element7:      for seven row lengths in 0 .. 3 (all 4^7 combinations, empty rows anywhere) every p below the total maps to
//                  base[row] + offset of the naive walk over the rows, tagged bases (top bit) included, every element once.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "gs_lanewin.hpp"

namespace lw = gs::lanewin;

#define CHECK(cond, ...)                                \
    do {                                                \
        if (!(cond)) {                                  \
            std::fprintf(stderr, "FAILED %s: ", #cond); \
            std::fprintf(stderr, __VA_ARGS__);          \
            std::fprintf(stderr, "\n");                 \
            std::exit(1);                               \
        }                                               \
    } while (0)

int main() {
    long cases = 0;
    for (int Wd = 1; Wd <= 9; ++Wd)
        for (int Hd = 1; Hd <= 7; ++Hd) {
            const int nc = Wd * Hd;
            for (int centre = 0; centre < nc; ++centre)
                for (int R = 1; R <= 3; ++R) {
                    std::set<int> seen;
                    for (int k = -1; k <= 2 * R + 1; ++k) {
                        const lw::PixRow pr = lw::recentred_row(centre, k, R, Wd, nc);
                        // naive: the row's 2R + 1 pixels one by one, clamped
                        std::set<int> want;
                        const int g = centre + (k - R) * Wd;
                        bool below = true, above = true;
                        for (int d = -R; d <= R; ++d) {
                            below = below && g + d < 0;
                            above = above && g + d > nc - 1;
                        }
                        if (k >= 0 && k <= 2 * R && !below && !above)
                            for (int d = -R; d <= R; ++d) want.insert(g + d < 0 ? 0 : (g + d > nc - 1 ? nc - 1 : g + d));
                        if (want.empty()) {
                            CHECK(pr.first > pr.last, "Wd %d Hd %d centre %d R %d row %d: [%d, %d], expected none", Wd, Hd, centre, R, k, pr.first, pr.last);
                        } else {
                            CHECK(pr.first >= 0 && pr.last <= nc - 1 && pr.first <= pr.last, "Wd %d Hd %d centre %d R %d row %d: [%d, %d] leaves the grid", Wd, Hd,
                                  centre, R, k, pr.first, pr.last);
                            CHECK(pr.first == *want.begin() && pr.last == *want.rbegin(), "Wd %d Hd %d centre %d R %d row %d: [%d, %d], naive [%d, %d]", Wd, Hd,
                                  centre, R, k, pr.first, pr.last, *want.begin(), *want.rbegin());
                            CHECK(pr.last - pr.first <= 2 * R, "Wd %d Hd %d centre %d R %d row %d: %d pixels", Wd, Hd, centre, R, k, pr.last - pr.first + 1);
                            for (int p = pr.first; p <= pr.last; ++p) seen.insert(p);
                        }
                        ++cases;
                    }
                    const int cr = centre / Wd, cc = centre % Wd;
                    for (int r = 0; r < Hd; ++r)
                        for (int c = 0; c < Wd; ++c)
                            if (std::abs(r - cr) <= R && std::abs(c - cc) <= R)
                                CHECK(seen.count(r * Wd + c) == 1, "Wd %d Hd %d centre %d R %d: window pixel (%d, %d) in no row", Wd, Hd, centre, R, r, c);
                }
        }
    for (int code = 0; code < 4 * 4 * 4 * 4 * 4 * 4 * 4; ++code) {
        int n[lw::kRows2], base[lw::kRows2], pre[lw::kRows2 + 1];
        pre[0] = 0;
        for (int k = 0, c = code; k < lw::kRows2; ++k, c /= 4) {
            n[k] = c % 4;
            base[k] = (k % 2) ? (int)(0x80000000u | (unsigned)(100 * k + 3)) : 50 * k + 1;  // odd rows come from memory (tagged)
            pre[k + 1] = pre[k] + n[k];
        }
        std::vector<int> want;
        for (int k = 0; k < lw::kRows2; ++k)
            for (int o = 0; o < n[k]; ++o) want.push_back((int)((unsigned)base[k] + (unsigned)o));
        CHECK((int)want.size() == pre[lw::kRows2], "code %d", code);
        for (int p = 0; p < pre[lw::kRows2]; ++p) {
            const int e = lw::element7(p, pre[1], pre[2], pre[3], pre[4], pre[5], pre[6], base[0], lw::seq_adj(base[1], pre[1]),
                                       lw::seq_adj(base[2], pre[2]), lw::seq_adj(base[3], pre[3]), lw::seq_adj(base[4], pre[4]),
                                       lw::seq_adj(base[5], pre[5]), lw::seq_adj(base[6], pre[6]));
            CHECK(e == want[p], "lengths code %d p %d: element %d, naive %d", code, p, e, want[p]);
        }
        ++cases;
    }
    std::printf("lanewin_recentre_check: %ld cases passed\n", cases);
    return 0;
}
