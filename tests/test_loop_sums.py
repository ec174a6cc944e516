"""The 29 linearisation sums of the ICP LOOPS (knn1_loop_k's fused epilogue, the fold of the partial rows in its prologue,
icp_step_k's reduce_partials) against float64 sums of the restated rows, at every seam of the row fold.

What a loop leaves behind is read from the tape of gs_icp_point_to_plane_taped (icp.hip tape_layout: records, then cloud slots,
then key slots, each 256-byte aligned).  Record r holds, at REC_LIN, the 44 words H | g | e | count that step r was given, at
REC_SLOT the slot the preceding association wrote, and opens with the IcpState BEFORE the step (gs_icp_step.hpp).

The restatement is the one of tests/test_linearize_exact.py (`_rows`, `_sums`), fed with the slot's cloud p (the kernel's fp32
bits), its keys, tgt and nrm:  a = [n ; p x n],  b = n . (t - p);  a row is kept iff its index is below the device count, its key is
not KEY_NONE and (thresh < 0 or d2 < thresh);  the sums are taken in float64.

Two comparisons, neither tuned on the code under test:
  * exact: a lattice scene (coordinates and normals from {-1, 0, 1}, no hints, identity start).  The first association's cloud is
    src itself, every product and every partial sum is an integer below 2^24 (asserted on the CPU), so record 0 owes the float64
    sums bit for bit whatever the tree.
  * bounded: every record of every run, |sum - float64 sum| <= 2 h 2^-24 sum |term|, h = the additions a term can pass through
    (`additions`, from the launch constants); the count (word 43) is exactly the number of kept rows.  (The one-point cloud of
    the one-tile seam has fewer rows than the step has unknowns: its record 0 is held to all of this, a later record only
    while the singular step left finite numbers.)

Forms of the fold (icp.hip icp_run, gs_icp_loop.hpp): up to 320 tiles under grid search ten loads per thread, up to 512 sixteen;
the finish by sixteen waves (rp_finish), eight (rp_finish2) or wave 0 (rp_finish_wave0<16 | 8>, grid search); above 512 tiles the
step is icp_step_k's reduce_partials in two rounds, above 1024 rows in three.  A loop's LAST step is icp_step_k at every size.

Every tile used the published pose: every block folds and steps for itself and only block 0 publishes, so the one place where
another block's fold shows is the cloud it writes.  Slot a's cloud is xform(dT, in) with dT from the state record a OPENS with
(the state after step a - 1; record 0: the initial state) and in = src (a = 0) or the cloud of that state's p_cur; every row
must be that map within the rounding of xform, 8 * 2^-24 * (|R| |in| + |t|) elementwise (four roundings per coordinate).

Worst error / bound measured on the MI355X stands next to each case (CASES, below).
"""
import functools
import math

import pytest
import torch

from tests import test_linearize_exact as L
from tests import test_loop_waves as W

DEV = W.DEV
U, EXACT = 2.0 ** -24, 2.0 ** 24
REC_WORDS, REC_LIN, REC_SLOT, REC_MODE = 160, 96, 140, 141       # gs_icp_step.hpp
ST_DT, ST_CUR, ST_P_CUR, ST_IT = 16, 32, 83, 86                   # IcpState: T | dT | cur[44] | xi[6] | damp | p_cur b_cur b_first it
STEP_ADOPT = 0
RP_FEW, RP_LOADS, FOLD_MAX = 10, 16, 512                         # gs_icp_reduce.hpp, icp.hip (fold = tiles <= 2 * 256)
SEAMS = [1, 2, 32, 33, 320, 321, 512, 513, 1024, 1025]
FULL_LAST_TILE = (33, 513)                                       # ns = 64 lb there, elsewhere the last tile holds one point
FORMS = [("boxes", 16), ("boxes", 8), ("grid", 16), ("grid", 8)]
assert 32 * RP_FEW == 320 and 32 * RP_LOADS == FOLD_MAX


def seam_ns(lb, tile=64):
    return tile * lb if lb in FULL_LAST_TILE and tile == 64 else tile * (lb - 1) + 1


def additions(lb):
    """Roundings a term can pass through: its own product (an fma onto zero), the tile's reduction in the epilogue (three
    additions inside a group of four lanes, sixteen groups), ceil(lb / 32) rows of its row group, the 32 groups."""
    return 1 + 3 + 16 + math.ceil(lb / 32) + 32


@pytest.fixture(scope="module")
def gs():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import gradslam_amd

    gradslam_amd._native.lib()  # fail loudly if the extension is missing
    return gradslam_amd


# ---------------------------------------------------------------------------------------------- scenes
@functools.lru_cache(maxsize=None)
def lattice(lb):
    """CPU float32 (src, tgt, nrm, keys): integer coordinates; the target has no point at x = 1, so a third of the rows have a
    residual.  keys: the exact nearest neighbour (squared distances are small integers; the lowest index wins a tie)."""
    ns, nt = seam_ns(lb), 300
    g = torch.Generator().manual_seed(7 + lb)
    src, tgt, nrm = (torch.randint(-1, 2, (n, 3), generator=g).float() for n in (ns, nt, nt))
    tgt[:, 0] = torch.randint(-1, 1, (nt,), generator=g).float()
    d2 = (src * src).sum(1)[:, None] + (tgt * tgt).sum(1)[None, :] - 2.0 * (src @ tgt.T)  # (integers below 2^24: exact)
    best = (d2.to(torch.int64) * 1024 + torch.arange(nt)[None, :]).min(dim=1).values
    keys = L._pack((best // 1024).float(), best % 1024)
    return src, tgt, nrm, keys


def lattice_ref(lb):
    src, tgt, nrm, keys = lattice(lb)
    return L._sums(*L._rows(src, tgt, nrm, keys, None)[:3])


def test_lattice_sums_stay_exact_in_float32():
    """The condition under which record 0 owes the float64 sums bit for bit: behind each accumulator the sum of ABSOLUTE values
    is below 2^24, so every partial sum in any order is an exactly representable integer.  And the scene is not trivial: g and
    e are not zero."""
    for lb in SEAMS:
        ref, ref_abs = lattice_ref(lb)
        assert float(ref_abs.max()) < EXACT, (lb, float(ref_abs.max()))
        assert torch.equal(ref, ref.round()) and float(ref[43]) == seam_ns(lb)
        if lb > 1:
            assert float(ref[42]) > 0 and bool(ref[36:42].abs().sum() > 0)


def test_seam_sizes():
    assert [seam_ns(lb) for lb in SEAMS] == [1, 65, 1985, 2112, 20417, 20481, 32705, 32832, 65473, 65537]
    assert all(math.ceil(seam_ns(lb) / 64) == lb for lb in SEAMS)
    assert [math.ceil(seam_ns(lb, 33) / 33) for lb in (512, 513)] == [512, 513]
    assert [additions(lb) for lb in (1, 32, 33, 512, 513, 1024, 1025)] == [53, 53, 54, 68, 69, 84, 85]


@functools.lru_cache(maxsize=None)
def _grid_scene_of(Hd, Wd):
    return W.grid_scene(seed=21, Hd=Hd, Wd=Wd, per_cell=2)


def grid_scene(ns, room_for=None):
    """The synthetic ds-grid scene of the grid-search tests with its source cloud (and src_pix) cut to ns points: the smallest
    of three sizes that holds them (or room_for points)."""
    room = ns if room_for is None else room_for
    Hd, Wd = (60, 80) if room <= 4000 else ((180, 240) if room <= 38000 else (240, 320))
    sc = dict(_grid_scene_of(Hd, Wd))
    assert sc["src"].shape[0] >= ns, (sc["src"].shape[0], ns)
    sc["src"], sc["src_pix"] = sc["src"][:ns].contiguous(), sc["src_pix"][:ns].contiguous()
    return sc


def lattice_scene(lb):
    src, tgt, nrm, _ = lattice(lb)
    return dict(src=src.to(DEV), tgt=tgt.to(DEV), nrm=nrm.to(DEV))


# ---------------------------------------------------------------------------------------------- running and reading
def run_form(gs, form, sc, tile=0, expect_blocks=None, **kw):
    """W.run_loops under one form of the kernel; the loop counters say that the form really ran."""
    lib = gs._native.lib()
    search, nw = form
    hints = "scan_points" in sc
    assert hints or search == "boxes"
    W._counts(lib, reset=True)
    try:
        assert lib.gs_set_loop_waves(nw) == nw
        lib.gs_set_grid_search(1 if search == "grid" else 0)
        lib.gs_set_tile_points(tile)
        out = W.run_loops(gs, sc, hints=hints, **kw)
    finally:
        lib.gs_set_tile_points(0)
        lib.gs_set_grid_search(1)
        assert lib.gs_set_loop_waves(0) == 0
    loops, grid_loops, forced, _ = W._counts(lib)
    assert (loops, grid_loops, forced) == (2, 2 if search == "grid" else 0, 2 if tile else 0), (form, loops, grid_loops, forced)
    if expect_blocks is not None:
        assert out["blocks"] == expect_blocks, (out["blocks"], expect_blocks)  # gs_icp_launch_geometry: the seam is the one meant
    return out


def read_tape(tape, cap, numiters, grad_lm):
    """-> (records (n, 160) float32, [cloud (cap, 3)], [keys (cap,) int64]) of a taped loop of capacity `cap`."""
    al = lambda x: (x + 255) // 256 * 256
    n = 2 * numiters if grad_lm else numiters + 1  # association launches = slots = steps
    rec_b, pts_b, best_b = al((n + 1) * REC_WORDS * 4), al(cap * 12), al(cap * 8)
    recs = tape[: n * REC_WORDS * 4].view(torch.float32).view(n, REC_WORDS)
    clouds = [tape[rec_b + a * pts_b: rec_b + a * pts_b + cap * 12].view(torch.float32).view(cap, 3) for a in range(n)]
    keys = [tape[rec_b + n * pts_b + a * best_b: rec_b + n * pts_b + a * best_b + cap * 8].view(torch.int64) for a in range(n)]
    return recs, clouds, keys


def state_int(rec, word):
    return int(rec[word: word + 1].view(torch.int32))


def check_records(out, sc, numiters, grad_lm, lb, thresh=None, n=None, what=""):
    """Every record of the taped run against the float64 restatement (module docstring): sums within the bound, count exactly;
    every slot's cloud the rigid map of its input by the state its record opens with; the plain loop's trace the records' words.
    -> (worst error / bound, kept share of record 0)."""
    src, tgt, nrm = sc["src"].cpu(), sc["tgt"].cpu(), sc["nrm"].cpu()
    cap = src.shape[0]
    n = cap if n is None else n
    recs, clouds, keys = read_tape(out["tape"], cap, numiters, grad_lm)
    h = additions(lb)
    worst, share0 = 0.0, None
    # (fewer rows than unknowns: the 6 x 6 system is singular and what follows the first step means nothing -- record 0, whose
    # cloud is src, is all such a loop is held to)
    assert n < 6 or (torch.isfinite(recs[:, REC_LIN: REC_LIN + 44]).all() and torch.isfinite(out["T_taped"]).all())
    for r in range(recs.shape[0]):
        slot = int(recs[r, REC_SLOT])
        assert slot == r and float(recs[r, REC_SLOT]) == r  # every association of a taped loop has a slot of its own, in order
        if n < 6 and r > 0 and not (torch.isfinite(clouds[slot][:n]).all() and torch.isfinite(recs[r, :ST_CUR]).all()):
            continue
        k = keys[slot][:n]
        assert bool(((k & 0xFFFFFFFF) < tgt.shape[0]).logical_or(k == L.KEY_NONE).all())
        A, b, keep, _ = L._rows(clouds[slot][:n], tgt, nrm, k, thresh, dtype=torch.float32)
        ref, ref_abs = L._sums(A, b, keep)
        got = recs[r, REC_LIN: REC_LIN + 44].double()
        assert float(got[43]) == float(keep.sum()), (what, r, float(got[43]), int(keep.sum()))
        tol = 2.0 * h * U * ref_abs[:43]
        err = (got[:43] - ref[:43]).abs()
        assert bool((err <= tol).all()), (what, r, float((err / tol.clamp_min(1e-300)).max()))
        worst = max(worst, float((err / tol.clamp_min(1e-300)).max()))
        if r == 0:
            share0 = float(keep.sum()) / n
        # the pose every tile used
        dT = recs[r, ST_DT: ST_DT + 16].double().view(4, 4)
        src_in = src[:n] if r == 0 else clouds[state_int(recs[r], ST_P_CUR)][:n]
        want = src_in.double() @ dT[:3, :3].T + dT[:3, 3]
        room = 8.0 * U * (src_in.double().abs() @ dT[:3, :3].abs().T + dT[:3, 3].abs())
        off = (clouds[slot][:n].double() - want).abs()
        assert bool((off <= room).all()), (what, r, "row", int((off / room.clamp_min(1e-300)).max(dim=1).values.argmax()),
                                           float((off / room.clamp_min(1e-300)).max()))
        if r > 0:  # the state a record opens with is the state the step before left: what ADOPT adopted are that step's sums
            if int(recs[r - 1, REC_MODE]) == STEP_ADOPT:
                assert torch.equal(recs[r, ST_CUR: ST_CUR + 44].view(torch.int32), recs[r - 1, REC_LIN: REC_LIN + 44].view(torch.int32))
        # the plain loop's trace row of this step: the state's sums, its error, the look-ahead's error, the state's count
        if int(recs[r, REC_MODE]) != STEP_ADOPT:
            tr = out["trace"][state_int(recs[r], ST_IT)]
            same = lambda x, y: torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
            assert same(tr[:43], recs[r, ST_CUR: ST_CUR + 43]) and same(tr[43:44], recs[r, REC_LIN + 42: REC_LIN + 43]), (what, r)
            assert same(tr[46:47], recs[r, ST_CUR + 43: ST_CUR + 44]), (what, r)
    assert torch.equal(out["T"], out["T_taped"])
    return worst, share0


def same_loop(a, b, cap_a, cap_b, n, numiters, grad_lm, what=""):
    """Two runs of capacities cap_a / cap_b with the same device count n: records, the first n rows of every slot, poses, trace."""
    ra, ca, ka = read_tape(a["tape"], cap_a, numiters, grad_lm)
    rb, cb, kb = read_tape(b["tape"], cap_b, numiters, grad_lm)
    assert torch.equal(ra.view(torch.int32), rb.view(torch.int32)), what
    for s in range(len(ca)):
        assert torch.equal(ca[s][:n].view(torch.int32), cb[s][:n].view(torch.int32)) and torch.equal(ka[s][:n], kb[s][:n]), (what, s)
    for k in ("T", "T_taped", "trace"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (what, k)
    assert torch.equal(a["best_last"][:n], b["best_last"][:n]) and torch.equal(a["best_last_taped"][:n], b["best_last_taped"][:n]), what
    assert torch.isfinite(ra[:, REC_LIN: REC_LIN + 44]).all() and torch.isfinite(a["T"]).all()


# ---------------------------------------------------------------------------------------------- exact
# (worst error / bound of the records behind record 0 on the MI355X: the table above CASES, below)
@pytest.mark.gpu
@pytest.mark.parametrize("lb", SEAMS)
def test_loop_sums_lattice_is_exact(gs, lb):
    """Record 0 (the folded prologue up to 512 tiles, icp_step_k above) is the float64 restatement bit for bit, under eight and
    sixteen waves; the keys are the exact nearest neighbours; the later records (numiters = 2: the last one is icp_step_k's at
    every size) are within the bound."""
    src, tgt, nrm, want_keys = lattice(lb)
    ref, ref_abs = lattice_ref(lb)
    assert float(ref_abs.max()) < EXACT
    sc = lattice_scene(lb)
    for form in FORMS[:2]:  # (no hints: chunk boxes)
        out = run_form(gs, form, sc, expect_blocks=lb, numiters=2)
        recs, clouds, keys = read_tape(out["tape"], src.shape[0], 2, 0)
        assert torch.equal(clouds[0], src) and torch.equal(keys[0], want_keys), (lb, form)
        got = recs[0, REC_LIN: REC_LIN + 44].double()
        assert torch.equal(got, ref), (lb, form, float((got - ref).abs().max()), float(got[43]), float(ref[43]))
        worst, _ = check_records(out, sc, 2, 0, lb, what=(lb, form))
        print("lattice lb %d %s/%d worst err / bound behind record 0: %.3f" % (lb, form[0], form[1], worst))


# ---------------------------------------------------------------------------------------------- bounded
# (lb, threshold rejecting about half, gradLM, numiters).  Worst error / bound over all records, measured on the MI355X:
#   LM, no threshold, lb = 1 .. 1025 in SEAMS' order:  0.008 0.037 0.032 0.031 0.037 0.027 0.023 0.026 0.016 0.015
#   threshold (kept share 0.500 each):                 lb 33: 0.042   lb 321 (gradLM): 0.024   lb 513: 0.023
#   gradLM, lb = 2, 33, 320, 512, 1025:                0.037 0.031 0.037 0.025 0.025
#   forced tile of 33, lb = 512 | 513:                 0.036 | 0.026
#   capacity 513 | 1025 | 321 tiles above the count:   0.029 | 0.027 | 0.036
#   lattice, the records behind the exact one, lb = 1 .. 1025:  0.000 0.010 0.014 0.023 0.013 0.016 0.017 0.019 0.016 0.016
CASES = [(lb, False, 0, 2) for lb in SEAMS] + [(33, True, 0, 2), (321, True, 1, 3), (513, True, 0, 2)] + \
        [(lb, False, 1, 3) for lb in (2, 33, 320, 512, 1025)]


def all_forms(gs, sc, lb, tile=0, **kw):
    """The loop under all four forms; every record, cloud, key and pose of the other three carries the bits of chunk boxes with
    sixteen waves (same keys, same row groups, same order)."""
    outs = [run_form(gs, form, sc, tile=tile, expect_blocks=lb, **kw) for form in FORMS]
    for form, o in zip(FORMS[1:], outs[1:]):
        for k in ("tape", "T", "T_taped", "trace", "best_last", "best_last_taped", "state_taped"):
            assert torch.equal(o[k], outs[0][k]), (lb, form, k)
    return outs[0]


def median_d2_thresh(gs, sc):
    """A squared distance about half of the first association's rows lie below (the scene's own nearest-neighbour distances)."""
    from gradslam_amd import ops

    d2, _ = ops.knn1_unpack(ops.knn1_raw(sc["src"], sc["tgt"]))
    return float(d2.median()) if d2.numel() > 1 else 2.0 * float(d2[0]) + 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("lb,thresholded,grad_lm,numiters", CASES)
def test_loop_sums_real_values(gs, lb, thresholded, grad_lm, numiters):
    ns = seam_ns(lb)
    sc = grid_scene(ns)
    thresh = median_d2_thresh(gs, sc) if thresholded else None
    out = all_forms(gs, sc, lb, numiters=numiters, grad_lm=grad_lm, thresh=-1.0 if thresh is None else thresh)
    worst, share0 = check_records(out, sc, numiters, grad_lm, lb, thresh=thresh, what=(lb, thresholded, grad_lm))
    print("lb %d thresh %s gradLM %d h %d worst err / bound %.3f kept share %.3f" % (lb, thresh, grad_lm, additions(lb), worst, share0))
    assert (0.4 < share0 < 0.6) if thresholded else share0 == 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("lb", [512, 513])
def test_loop_sums_forced_tile_of_33(gs, lb):
    """gs_set_tile_points(33): lanes 33 .. 63 of every tile are empty, 512 | 513 tiles are 16 864 | 16 897 points."""
    sc = grid_scene(seam_ns(lb, 33))
    out = all_forms(gs, sc, lb, tile=33, numiters=2)
    worst, _ = check_records(out, sc, 2, 0, lb, what=("tile 33", lb))
    print("tile 33 lb %d worst err / bound %.3f" % (lb, worst))


# ---------------------------------------------------------------------------------------------- capacity above count
@pytest.mark.gpu
@pytest.mark.parametrize("cap_lb,forms", [(513, FORMS), (1025, FORMS), (321, FORMS[2:])])
def test_loop_sums_capacity_above_count(gs, cap_lb, forms):
    """A launch sized for the capacity (513 and 1025 tiles: icp_step_k in two and three rounds; 321: the sixteen-load fold)
    with a device count of 100 tiles + 7 (321: of 320 tiles): the tiles beyond the count write zero rows and every record
    equals the run whose capacity is the count (101 tiles, 321: 320 -- the ten-load fold), bit for bit.  Source rows beyond
    the count hold NaN: they are not read."""
    cap = seam_ns(cap_lb)
    n = 64 * 100 + 7 if cap_lb != 321 else seam_ns(320)
    big = grid_scene(cap)
    big["src"] = big["src"].clone()
    big["src"][n:] = float("nan")
    small = grid_scene(n, room_for=cap)
    assert torch.equal(big["src"][:n], small["src"]) and torch.equal(big["tgt"], small["tgt"])
    for form in forms:
        a = run_form(gs, form, big, expect_blocks=cap_lb, numiters=2, ns_dev=n)
        b = run_form(gs, form, small, expect_blocks=math.ceil(n / 64), numiters=2)
        same_loop(a, b, cap, n, n, 2, 0, what=(cap_lb, form))
        if form == forms[0]:
            worst, _ = check_records(a, big, 2, 0, cap_lb, n=n, what=("capacity", cap_lb))
            print("capacity %d tiles, count %d: worst err / bound %.3f" % (cap_lb, n, worst))


# ---------------------------------------------------------------------------------------------- stale rows
@pytest.mark.gpu
def test_loop_sums_ignore_stale_partial_rows(gs):
    """Both partial-row regions of the workspace full of 0xFF (NaN) before a loop of 33 tiles: rows 33 .. 511, which the padded
    folds read unconditionally, are icp_prepare_k's to zero, rows 0 .. 32 the tiles' to write before they are read.  Everything
    finite and bit-equal to the run on a zeroed workspace, under all four forms."""
    lb = 33
    ns = seam_ns(lb)
    sc = grid_scene(ns)
    for form in FORMS:
        clean = run_form(gs, form, sc, expect_blocks=lb, numiters=2)
        stale = run_form(gs, form, sc, expect_blocks=lb, numiters=2, rows_fill=0xFF)
        same_loop(stale, clean, ns, ns, ns, 2, 0, what=form)
        assert torch.equal(stale["state_taped"], clean["state_taped"])
        rows = lambda o: o["partial_rows_taped"].view(2, -1)[:, : FOLD_MAX * 29 * 4]  # (row 512 is the spare one: never summed)
        assert torch.equal(rows(stale), rows(clean)) and torch.isfinite(rows(stale).contiguous().view(torch.float32)).all(), form
