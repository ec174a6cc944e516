"""The c2 step's launch chain from a `rocprofv3 --kernel-trace` database (rocpd SQLite, rocprofv3's default output).

    rocprofv3 --kernel-trace --stats -d DIR -o run -- python3 bench.py --gpus 1 --steps 50 --warmup 5
    python3 tools/c2_chain.py DIR/run_results.db
    python3 tools/c2_chain.py DIR/run_results.db --by-frame 48      (bench.py --steps 48: the run's last 48 steps)

A step of the plain bench run starts with a launch of `vertex_normal_k` (the live frame's maps) or, with the fused front end,
of the kernel that carries its tiles (`setup_count_k`).  The tool cuts the dispatch sequence at every such launch, keeps the
steps whose launch sequence is the most common one (the timed steps; warm-up, capture and the other parts of the run
differ), and prints per position in the chain: kernel, median and mean duration, median gap from the previous launch's end.

--by-frame K: bench.py cycles N_LIVE = 4 live frames, step i of the timed region taking frame 1 + i % 4, and the four frames'
loops do not cost the same (the further the frame from the map's, the more lanes lose their proof in the loop's early
launches).  A median over all steps sits between the frames and hides what the step pays, which is the mean.  With K = the
run's --steps (the timed region is the run's last K steps) the table is printed once per live frame: median, mean and spread
(max - min) per position.
"""
import collections
import sqlite3
import statistics
import sys

STARTS = ("vertex_normal_k", "setup_count_k")
N_LIVE = 4  # bench.py's


def short(name):
    n = name.split("(")[0]
    return n.replace("void ", "").replace("gs::", "")


def table(chain, sel, title):
    print(title)
    tot_span = statistics.median(st[-1][2] - st[0][1] for st in sel) / 1e3
    tot_mean = statistics.fmean(st[-1][2] - st[0][1] for st in sel) / 1e3
    busy = busy_mean = 0.0
    print("%-3s %-60s %9s %9s %9s %9s" % ("#", "kernel", "dur_us", "mean_us", "spread_us", "gap_us"))
    for i, k in enumerate(chain):
        durs = [(st[i][2] - st[i][1]) / 1e3 for st in sel]
        d, m = statistics.median(durs), statistics.fmean(durs)
        g = statistics.median(st[i][1] - st[i - 1][2] for st in sel) / 1e3 if i else 0.0
        busy += d
        busy_mean += m
        print("%-3d %-60s %9.2f %9.2f %9.2f %9.2f" % (i, k[:60], d, m, max(durs) - min(durs), g))
    print("launches per step: %d; first-start to last-end: median %.1f us, mean %.1f us; sum of median durations: %.1f us, of mean durations: %.1f us"
          % (len(chain), tot_span, tot_mean, busy, busy_mean))


def main(path, by_frame=0):
    c = sqlite3.connect(path)
    rows = c.execute("select name, start, end from kernels order by start").fetchall()
    steps, cur = [], None
    for name, s, e in rows:
        k = short(name)
        if any(k.startswith(p) for p in STARTS):
            cur = []
            steps.append(cur)
        if cur is not None:
            cur.append((k, s, e))
    sig = collections.Counter(tuple(k for k, _, _ in st) for st in steps)
    chain, n = sig.most_common(1)[0]
    sel = [st for st in steps if tuple(k for k, _, _ in st) == chain]
    table(chain, sel, "%d steps cut, %d with the most common chain of %d launches" % (len(steps), n, len(chain)))
    if by_frame:
        # the timed region is the run's last K steps, whatever their chain: a step with another chain keeps its place in the
        # cycle of frames and is left out of its frame's table (the tables say how many of K / 4 they hold)
        if by_frame > len(steps):
            raise SystemExit("--by-frame %d: the trace holds only %d steps" % (by_frame, len(steps)))
        timed = steps[-by_frame:]
        for f in range(N_LIVE):
            mine = [st for i, st in enumerate(timed) if i % N_LIVE == f and tuple(k for k, _, _ in st) == chain]
            print()
            table(chain, mine, "live frame %d: %d of the last %d steps" % (f + 1, len(mine), len(timed)))


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser(description="the c2 step's launch chain from a rocprofv3 --kernel-trace database")
    ap.add_argument("db", help="rocpd SQLite database (DIR/<name>_results.db)")
    ap.add_argument("--by-frame", type=int, default=0, metavar="K",
                    help="the run's --steps: print the table once per live frame (the timed region is the run's last K steps)")
    a = ap.parse_args()
    main(a.db, a.by_frame)
