"""The c2 step's launch chain from a `rocprofv3 --kernel-trace` database (rocpd SQLite, rocprofv3's default output).

    rocprofv3 --kernel-trace --stats -d DIR -o run -- python3 bench.py --gpus 1 --steps 50 --warmup 5
    python3 tools/c2_chain.py DIR/run_results.db

A step of the plain bench run starts with a launch of `vertex_normal_k` (the live frame's maps) or, with the fused front end,
of the kernel that carries its tiles (`setup_count_k`).  The tool cuts the dispatch sequence at every such launch, keeps the
steps whose launch sequence is the most common one (the timed steps; warm-up, capture and the other parts of the run
differ), and prints per position in the chain: kernel, median duration, median gap from the previous launch's end.
"""
import collections
import sqlite3
import statistics
import sys

STARTS = ("vertex_normal_k", "setup_count_k")


def short(name):
    n = name.split("(")[0]
    return n.replace("void ", "").replace("gs::", "")


def main(path):
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
    print("%d steps cut, %d with the most common chain of %d launches" % (len(steps), n, len(chain)))
    tot_span = statistics.median(st[-1][2] - st[0][1] for st in sel) / 1e3
    busy = 0.0
    print("%-3s %-60s %9s %9s" % ("#", "kernel", "dur_us", "gap_us"))
    for i, k in enumerate(chain):
        d = statistics.median(st[i][2] - st[i][1] for st in sel) / 1e3
        g = statistics.median(st[i][1] - st[i - 1][2] for st in sel) / 1e3 if i else 0.0
        busy += d
        print("%-3d %-60s %9.2f %9.2f" % (i, k[:60], d, g))
    print("launches per step: %d; median first-start to last-end: %.1f us; sum of median durations: %.1f us" % (len(chain), tot_span, busy))


if __name__ == "__main__":
    main(sys.argv[1])
