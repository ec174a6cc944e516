"""Records what every size query of the C ABI (gs_*_ws_bytes, gs_*_tape_bytes) returns, for a fixed list of shapes, into
tests/golden/ws_sizes.json.  tests/test_ws_sizes.py holds every later build to these numbers: Python's workspace cache rounds
sizes to powers of two and the workspace address is part of the captured graph's key, so a size that drifts changes
allocations and graph replay.

    python tools/gen_golden_ws_sizes.py [LIBRARY] [COMMIT]

LIBRARY is the libgradslam_hip.so to record (default: the in-tree build; it loads without a GPU), COMMIT the hash it was built
from (default: git rev-parse HEAD).  Arguments are given to each function by the NAME its parameter has in
include/gradslam_hip.h, so one scenario serves every function."""
import ctypes
import itertools
import json
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gradslam_amd import _native  # noqa: E402

FLAGS = ("grad_lm", "use_grad_lm", "has_color")
MILLION = 1024 * 1024  # rows of kSelfScanBlocks compaction blocks: one more row needs the scan launch


def shape(B, H, W, ds, Nmax, numiters, **more):
    """One scenario: the frame, the map's capacity, and what the per-op entries call the same quantities."""
    capS = -(-H // max(ds, 1)) * -(-W // max(ds, 1))
    s = dict(B=B, L=B, H=H, W=W, height=H, width=W, ds=ds, stride=ds, Nmax=Nmax, numiters=numiters, levels=3,
             max_ns=capS, max_nt=Nmax, n_rows=H * W, N_max=Nmax, M_max=Nmax, Na_max=capS, Nb_max=Nmax, Ns_max=capS, Nt_max=Nmax,
             K=8, C=3, nx=16, ny=12, nz=8)
    s.update(more)
    return s


SCENARIOS = [
    shape(1, 1, 1, 1, 1, 0, K=1, C=1, nx=1, ny=1, nz=1, levels=1),                # all dims 1, no iterations
    shape(1, 120, 160, 4, 19200, 10),                                             # the benchmark's step
    shape(2, 48, 64, 2, 3072, 3),
    shape(1, 480, 640, 4, 307200, 10),                                            # test_localize_backward_modes_share_one_layout
    shape(1, 12, 16, 2, 0, 2, max_ns=0, n_rows=0),                                # capacities the entries clamp
    shape(1, 12, 16, 2, -1, -1, max_ns=-1, n_rows=-1),
    shape(0, 12, 16, 2, 70, 2),                                                   # (gs_project_active clamps B)
    shape(1, 1024, 1024, 1, MILLION, 2, n_rows=MILLION, nx=4, ny=4, nz=4),        # kSelfScanBlocks compaction blocks ...
    shape(1, 1024, 1025, 1, MILLION + 1, 2, n_rows=MILLION + 1, nx=4, ny=4, nz=4),  # ... and one more
]


def declared_sizes():
    """[(name, [parameter names])] of the header's size queries, in header order."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(os.path.join(REPO, "include", "gradslam_hip.h")).read(), flags=re.S)
    out = []
    for name, params in re.findall(r"\bsize_t\s+(gs_\w+_(?:ws|tape)_bytes)\s*\(([^)]*)\)\s*;", text):
        out.append((name, [p.split()[-1] for p in params.split(",")]))
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else _native.LIB_PATH
    commit = sys.argv[2] if len(sys.argv) > 2 else subprocess.check_output(["git", "-C", REPO, "rev-parse", "HEAD"], text=True).strip()
    lib = ctypes.CDLL(path)
    sizes = {}
    for name, params in declared_sizes():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _native.SIGNATURES[name]
        flags = [p for p in params if p in FLAGS]
        rows = []
        for s in SCENARIOS:
            for values in itertools.product((0, 1), repeat=len(flags)):  # both values of every flag
                args = [dict(s, **dict(zip(flags, values)))[p] for p in params]
                if [args] not in [r[:1] for r in rows]:
                    rows.append([args, int(fn(*args))])
        sizes[name] = rows
    out = os.path.join(REPO, "tests", "golden", "ws_sizes.json")
    with open(out, "w") as f:
        body = ",\n".join('  "{}": [\n{}\n  ]'.format(n, ",\n".join("    " + json.dumps(r) for r in rows)) for n, rows in sizes.items())
        f.write('{\n "commit": "' + commit + '",\n "sizes": {\n' + body + "\n }\n}\n")  # one call per line
    print("wrote", out, len(sizes), "functions,", sum(len(r) for r in sizes.values()), "calls")


if __name__ == "__main__":
    main()
