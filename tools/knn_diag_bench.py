#!/usr/bin/env python3
"""Diagnostic only: EVERY association launch of the bench's c2 localisation step, for each of its four live frames (needs
make -C gradslam_amd/csrc diag).  tools/knn_diag_long.py stamps the last launch of a streamed two-frame run, a scene in which
every proof holds; bench.py cycles four live frames 1 to 4 cm from the map's frame against a one-frame map, and there the
loop's early steps move most points to another ds-grid cell.  The loop is cut after k = 1 .. 10 iterations; the stamps are
those of its last launch, association k + 1.

Per launch: lanes whose proof failed after the first window ("in need"), tiles with at least one, tiles with more than six
(these take the tile-level search), and -- builds with the re-centred second window -- the blocks that took it, the lanes
and tiles still in need after it, the tiles that then took the tile-level search.  Block-end stamps (us after the block's
kernel entry, p50 / mean) of tiles with none in need, with one to six, with more than six; and the kernel's span.
usage: knn_diag_bench.py [first live frame] [last live frame]      (default 1 4)"""
import ctypes, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gradslam_amd import _native
_native.LIB_PATH = os.path.join(ROOT, "gradslam_amd", "libgradslam_hip_diag.so")
import gradslam_amd as gs
from gradslam_amd.synthetic import make_sequence

f_lo = int(sys.argv[1]) if len(sys.argv) > 1 else 1
f_hi = int(sys.argv[2]) if len(sys.argv) > 2 else 4
dev = "cuda:0"
c, d, K, P = make_sequence(1, 5, 480, 640, seed=0)
c, d, K, P = c.to(dev), d.to(dev), K.to(dev), P.to(dev)
frames = gs.RGBDImages(c, d, K, P)
lib = _native.lib()
lib.gs_diag_set_buffer.argtypes = [ctypes.c_void_p]
nblk = 2048
dbg = torch.zeros(nblk * 16 * 16, dtype=torch.int64, device=dev)
assert lib.gs_diag_set_buffer(dbg.data_ptr()) == 0
have_counts = hasattr(lib, "gs_window_counts")
tick = 1e-2


def stat(x):
    return "%5.2f / %5.2f (n %3d)" % (np.percentile(x, 50), x.mean(), x.shape[0]) if x.shape[0] else "   -  /    -  (n   0)"


for live_idx in range(f_lo, f_hi + 1):
    print("live frame %d" % live_idx)
    print("  launch | lanes tiles >6 in need | 2nd window: blocks, lanes / tiles / >6 still in need, refused | block end us p50 / mean: "
          "none in need | 1-6 | >6 | span us")
    for k in range(1, 11):
        slam = gs.slam.PointFusion(odom="icp", dsratio=4, numiters=k, device=dev)
        with torch.no_grad():
            world_map, _ = slam.step(gs.Pointclouds(device=dev), frames[:, 0], None)
            torch.cuda.synchronize()
            dbg.zero_()
            if have_counts:
                wc = (ctypes.c_uint * 4)()
                assert lib.gs_window_counts(wc, 1) == 0
            live = gs.RGBDImages(c[:, live_idx:live_idx + 1].contiguous(), d[:, live_idx:live_idx + 1].contiguous(), K)
            slam._localize(world_map, live, frames[:, 0])
        torch.cuda.synchronize()
        raw = dbg.cpu().numpy().reshape(nblk, 16, 16)
        nw = int((raw[..., 6] != 0).any(0).sum())
        raw = raw[:, :nw]
        raw = raw[raw[..., 3].max(1) > 0]
        a = raw.astype(np.float64)
        need = (raw[:, 0, 12] & 0xff).astype(np.int64)
        # wave 0's slot 15 (builds with the second window; zero otherwise): lanes still in need | took the window << 8 |
        # refused by the cap << 9 | the tile-level search ran << 10
        w15 = raw[:, 0, 15]
        need2 = np.where((w15 >> 8) & 1, w15 & 0xff, need)
        end = (a[..., 3].max(1) - a[..., 6].min(1)) * tick
        span = (a[..., 3].max() - a[..., 6].min()) * tick
        print("  %6d | %5d %5d %4d | %4d  %5d / %4d / %4d  %4d | %s | %s | %s | %5.1f" % (
            k + 1, need.sum(), (need > 0).sum(), (need > 6).sum(), ((w15 >> 8) & 1).sum(), need2.sum(), (need2 > 0).sum(), (need2 > 6).sum(),
            ((w15 >> 9) & 1).sum(), stat(end[need == 0]), stat(end[(need > 0) & (need <= 6)]), stat(end[need > 6]), span))
