"""The O(1) step of the device ICP loop, and its reverse pass, against a float64 restatement (oracle/icp_step.py).

Forward: every iteration of the device loop is checked on its own.  A run of k iterations gives T_k and k trace rows; the
restatement takes row k and T_{k-1} and must give the kernel's accept flag, damp and T_k.  Scenes are built to reach each
branch of the step (the pivoted solver fallback, both se3_exp branches, the gradLM clamp, the LM tie), and each test
asserts that its branch was reached.

Reverse: the loop's input gradients against float64 autograd through the same loop on the same inputs.  Both sides must
make the same discrete choices (associations, accept decisions, se3_exp branches); that is asserted first.  Each case
also names the adjoint terms it depends on, and the test shows that the float64 reference without that term is at least
10x its bound away from the kernel.

Bounds are at most 3x the worst value measured on an MI355X; the measurement is stated next to each."""
import numpy as np
import pytest
import torch

from oracle import icp_step as st
from tests.test_deterministic_grads import _surface

DEV = "cuda:0"
GP = (2.0, 1.0, 1.0, 200.0)  # the reference's defaults: lambda_max, B, B2, nu


# ------------------------------------------------------------------ scenes (fp32 CPU tensors: src, tgt, nrm)
def _motion(rx, ry, rz, tx, ty, tz):
    return torch.from_numpy(st.se3_exp64(np.array([tx, ty, tz, rx, ry, rz]), rx == ry == rz == 0))


def _moved(p, M):
    return st._xform(p.double(), M).float()


def scene(name):
    if name == "surface":  # resampled smooth surface: the target and the source never coincide
        tgt, nrm = _surface(32, 32, 1)
        return _moved(_surface(27, 27, 1)[0], _motion(0.02, -0.015, 0.03, 0.01, -0.02, 0.015)), tgt, nrm
    if name == "exact":  # the target moved by less than half its spacing: exact correspondences, fast convergence
        tgt, nrm = _surface(32, 32, 2)
        return _moved(tgt, _motion(0.004, -0.003, 0.005, 0.003, -0.002, 0.004)), tgt, nrm
    if name in ("corners", "corners_shift"):
        # eight targets near the corners of a cube, random normals: every association stays unambiguous under a large
        # step, so the step's rotation can be large (corners) or exactly zero (corners_shift: a pure translation)
        g = torch.Generator().manual_seed(1)
        c = torch.tensor([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=torch.float64)
        tgt = c + 0.1 * torch.randn(8, 3, generator=g, dtype=torch.float64)
        nrm = torch.randn(8, 3, generator=g, dtype=torch.float64)
        nrm = nrm / nrm.norm(dim=1, keepdim=True)
        M = _motion(0.25, 0.1, -0.15, 0.1, 0.3, -0.2) if name == "corners" else _motion(0, 0, 0, 0.1, 0.3, -0.2)
        return _moved(tgt, M), tgt.float(), nrm.float()
    if name == "planar":  # a tilted plane: H has rank 3, its fp32 rounding swamps damp = 1e-8
        g = torch.Generator().manual_seed(3)
        u = torch.rand(800, 2, generator=g, dtype=torch.float64)
        n = torch.tensor([0.3, -0.2, 0.93], dtype=torch.float64)
        n = n / n.norm()
        e1 = torch.linalg.cross(n, torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64))
        e1 = e1 / e1.norm()
        e2 = torch.linalg.cross(n, e1)
        tgt = u[:, :1] * e1 + u[:, 1:] * e2 + 0.5 * n
        return (tgt + 1e-4 * n).float(), tgt.float(), n.expand_as(tgt).float().contiguous()
    if name == "offset":  # the surface 0.25 off along z: the first step cuts the error by ~250
        tgt, nrm = _surface(64, 64, 4)
        return tgt + torch.tensor([0.0, 0.0, 0.25]), tgt, nrm
    if name == "zero":  # source == target: zero residual, xi = 0, new_err == err
        tgt, nrm = _surface(24, 24, 5)
        return tgt.clone(), tgt, nrm
    raise KeyError(name)


# ------------------------------------------------------------------ A: the restatement against the CPU oracle
@pytest.mark.parametrize("name,grad,n,damp", [("surface", None, 6, 1e-8), ("exact", None, 4, 1e-8), ("zero", None, 3, 1e-8),
                                              ("surface", GP, 4, 1e-8), ("offset", GP, 3, 1e-8),
                                              ("corners", GP, 2, -1.0)])
def test_restated_step_reproduces_oracle_trace(name, grad, n, damp):
    """Fed the oracle's own trace rows, the restatement gives the oracle's accept flags and damps bit for bit and its
    per-iteration T within the oracle's fp32 solve error (cond * 2^-24 * |xi|, plus fp32 se3_exp rounding).  The planar
    scene is left out: at cond ~1e9 the oracle's fp32 inverse has no correct digit."""
    from oracle import icp

    src, tgt, nrm = scene(name)
    tr = []
    if grad is None:
        icp.point_to_plane_ICP(src[None], tgt[None], nrm[None], torch.eye(4), numiters=n, damp=damp, trace=tr)
    else:
        lmax, Bg, B2, nu = grad
        icp.point_to_plane_gradICP(src[None], tgt[None], nrm[None], torch.eye(4), numiters=n, damp=damp, trace=tr,
                                   lambda_max=lmax, B=Bg, B2=B2, nu=nu)
    T_prev = np.eye(4)
    for k, rec in enumerate(tr):
        o = st.step(st.oracle_row(rec), T_prev, grad)
        assert o["accept"] == rec.get("accept", True), (name, k)
        if k + 1 < len(tr):
            assert np.float32(tr[k + 1]["damp"]) == o["damp"], (name, k)
        T_k = rec["T"].double().numpy()
        xi = np.abs(o["xi"]).max()
        tol = 1e-6 + 4 * o["cond"] * 2.0 ** -24 * xi * (1 + xi)
        assert np.abs(o["T"] - T_k).max() <= tol, (name, k, np.abs(o["T"] - T_k).max(), tol)
        T_prev = T_k


def test_restated_step_branches():
    """The restatement's own switches: fp32 th in the kernel's fma order, the tie, the solver path."""
    assert st.fma32(np.float32(1 + 2 ** -12), np.float32(1 + 2 ** -12), np.float32(-1)) == np.float32(2 ** -11 + 2 ** -24)
    assert st.theta32([0.0, 0.0, 9.9e-7])[()] < st.SMALL_ANGLE <= st.theta32([0.0, 6e-7, 8e-7])
    row = np.zeros(48, dtype=np.float32)
    row[:36] = np.eye(6, dtype=np.float32).reshape(-1)
    row[36:42] = 1e-3
    row[42] = row[43] = 0.5
    row[44] = 1e-8
    o = st.step(row, np.eye(4))
    assert not o["accept"] and o["damp"] == np.float32(2e-8) and o["path"] == "nopivot" and np.array_equal(o["T"], np.eye(4))
    row[44] = -2.0  # H + damp I = -I: every pivot negative
    assert st.step(row, np.eye(4))["path"] == "pivoted"


# ------------------------------------------------------------------ B: the forward step on the GPU
@pytest.fixture(scope="module")
def gs():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import gradslam_amd

    gradslam_amd._native.lib()  # fail loudly if the extension is missing
    return gradslam_amd


FWD = {  # name: (scene, numiters, damp, grad_params)
    "surface_lm": ("surface", 6, 1e-8, None),
    "exact_lm": ("exact", 4, 1e-8, None),
    "surface_grad": ("surface", 4, 1e-8, GP),
    "negdamp_grad": ("corners", 2, -1.0, GP),
    "planar_lm": ("planar", 3, 1e-8, None),
    "offset_grad": ("offset", 3, 1e-8, GP),
    "zero_lm": ("zero", 3, 1e-8, None),
}
# |T_k(kernel) - T_k(restated)| (T entries are O(1)) beyond the allowances below.  Measured worst on an MI355X: 1.36e-7
# (surface_lm, iteration 1); the pivoted steps 4.8e-8 (negdamp_grad) and 1.9e-9 (planar_lm at cond 2e8); offset_grad's
# 1.74e-5 is the fp32 coefficients' cancellation (allowance 8.9e-5 there).
TOL_T = 4e-7
_FWD_CACHE = {}


def _exp32_slack(o, grad):
    """The kernel evaluates se3_exp's coefficients in fp32 like the reference: (1 - cos th) / th^2 and (th - sin th) / th^3
    lose their digits to cancellation at small th, which moves T by up to 2^-24 |v| (1 / th + 1).  The restatement
    evaluates them in float64; this is the allowance for that difference (twice the estimate), zero on the small-angle
    branch, which has no such coefficient."""
    x = o["xi"] if grad is None else o["sxi"]
    small = o["small"] if grad is None else o["ssmall"]
    if small or not o["accept"]:
        return 0.0
    th = float(st.theta32(x[3:]))
    return 2.0 ** -23 * float(np.abs(x[:3]).max()) * (1.0 + 1.0 / th)


def _forward(gs, key):
    """Runs of 1..n iterations of the device loop; every row restated.  Cached per module."""
    if key in _FWD_CACHE:
        return _FWD_CACHE[key]
    name, n, damp, grad = FWD[key]
    src, tgt, nrm = (x.to(DEV) for x in scene(name))
    Ts, traces = [], []
    for k in range(1, n + 1):
        T, _, tr = gs.ops.icp_device_loop(src, tgt, nrm, torch.eye(4, device=DEV), k, damp, None, grad_params=grad,
                                          want_trace=True)
        Ts.append(T.cpu().numpy())
        traces.append(tr.cpu().numpy())
    out = []
    T_prev = np.eye(4)
    for k in range(n):
        o = st.step(traces[-1][k], T_prev, grad)
        o["T_kernel"] = Ts[k].astype(np.float64)
        out.append(o)
        T_prev = Ts[k]
    _FWD_CACHE[key] = (traces, out)
    return _FWD_CACHE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(FWD))
def test_device_step_matches_restatement(gs, key):
    traces, steps = _forward(gs, key)
    name, n, damp, grad = FWD[key]
    full = traces[-1]
    for k in range(1, n):  # a k-iteration run is the first k rows of the n-iteration run, bit for bit
        assert np.array_equal(traces[k - 1][:k].view(np.int32), full[:k].view(np.int32)), (key, k)
    worst = 0.0
    for k, o in enumerate(steps):
        row = full[k]
        assert bool(row[45]) == o["accept"], (key, k)
        if k + 1 < n:
            if grad is None:
                assert full[k + 1][44].view(np.int32) == o["damp"].view(np.int32), (key, k, full[k + 1][44], o["damp"])
            else:  # expf / powf on the device are not correctly rounded: a few ulp
                ulp = abs(int(full[k + 1][44].view(np.int32)) - int(o["damp"].view(np.int32)))
                assert ulp <= 4, (key, k, ulp)
        e = float(np.abs(o["T_kernel"] - o["T"]).max())
        xi = float(np.abs(o["xi"]).max())
        if xi > 1.0:  # not a moderate step: the fp64 solution of a near-singular system, compared finite only
            assert np.isfinite(o["T_kernel"]).all(), (key, k)
            print(key, k, o["path"], "|xi| %.2e: finite only" % xi)
            continue
        tol = TOL_T + o["cond"] * 1e-15 * xi * (1 + xi) + _exp32_slack(o, grad)
        print(key, k, o["path"], "small" if o["small"] else "th %.2e" % o["th"], "accept", o["accept"], "cond %.1e" % o["cond"],
              "T err %.2e tol %.2e" % (e, tol))
        worst = max(worst, e / tol * TOL_T)
        assert e <= tol, (key, k, e, tol)
    print(key, "worst T err (scaled) %.2e" % worst)


@pytest.mark.gpu
def test_pivoted_fallback_negative_damp(gs):
    """gradICP with damp = -1 between the two smallest eigenvalues of H: H + damp I is indefinite, so a pivot of the
    no-pivot elimination is negative and the step runs solve6_lu; the system stays well conditioned."""
    _, steps = _forward(gs, "negdamp_grad")
    paths = [o["path"] for o in steps]
    print("negdamp paths", paths, "cond", ["%.1e" % o["cond"] for o in steps])
    assert "pivoted" in paths
    assert all(o["cond"] < 1e3 for o in steps if o["path"] == "pivoted")


@pytest.mark.gpu
def test_pivoted_fallback_near_singular(gs):
    """A plane with damp = 1e-8: the fp32 H has rank 3 up to rounding, a pivot comes out <= 0 and the fallback solves a
    near-singular system.  test_device_step_matches_restatement holds the kernel's T to the fp64 solution of the same fp32
    matrix within TOL_T + cond * 1e-15 * |xi|; here the branch must have been reached."""
    _, steps = _forward(gs, "planar_lm")
    paths = [o["path"] for o in steps]
    print("planar paths", paths, "cond", ["%.1e" % o["cond"] for o in steps], "|xi|", ["%.1e" % np.abs(o["xi"]).max() for o in steps])
    assert "pivoted" in paths
    assert max(o["cond"] for o in steps if o["path"] == "pivoted") > 1e6


@pytest.mark.gpu
def test_small_angle_branch_both_sides(gs):
    """Converging LM runs: the iterations after the first take se3_exp's small-angle branch (th < 1e-6) and the full
    one, and the restated branch gives the kernel's T either way."""
    seen = set()
    for key in ("surface_lm", "exact_lm"):
        _, steps = _forward(gs, key)
        for o in steps[1:]:
            if o["accept"]:
                seen.add(o["small"])
        print(key, ["%.2e" % o["th"] for o in steps])
    assert seen == {True, False}, seen


@pytest.mark.gpu
def test_gradlm_clamp_reached(gs):
    """The gradLM gates clamp new_err - err to +-70: the offset scene's first step drops the error by more than that."""
    _, steps = _forward(gs, "offset_grad")
    raw = [float(o["raw_diff"]) for o in steps]
    print("offset raw diffs", raw, "clamped", [float(o["diff"]) for o in steps])
    assert raw[0] < -70.0 and steps[0]["diff"] == np.float32(-70.0)


@pytest.mark.gpu
def test_lm_tie_rejects(gs):
    """Zero residual: xi = 0, new_err == err == 0, the strict < rejects, damp doubles, T stays the identity."""
    traces, steps = _forward(gs, "zero_lm")
    full = traces[-1]
    for k, o in enumerate(steps):
        assert full[k][42] == 0.0 and full[k][43] == 0.0 and full[k][45] == 0.0, (k, full[k][42:46])
        assert not o["accept"] and np.array_equal(o["T_kernel"], np.eye(4))
        assert full[k][44] == np.float32(1e-8) * np.float32(2 ** k)


# ------------------------------------------------------------------ C: the reverse pass on the GPU
GRAD_CASES = {  # name: (scene, numiters, damp, grad_params, adjoint terms the gradients measurably depend on)
    # lm_n2 and grad_n3_small have converged by their last iteration: gC . dC enters as th^3 (th = 1e-2 at lm_n2's second
    # step, the small-angle branch has no C), their damp is 1e-8, and the sigma chain is weighted by a vanishing step.
    "lm_n1": ("corners", 1, 1e-8, None, ("dC",)),
    "lm_n2": ("corners", 2, 1e-8, None, ()),
    "grad_n1": ("corners", 1, 1e-8, GP, ("dC", "sigma")),
    "grad_n2_negdamp": ("corners", 2, -1.0, GP, ("dC", "sigma", "damp")),
    "grad_n3_small": ("corners_shift", 3, 1e-8, GP, ()),
}
# _errs of the kernel's gradients against the float64 reference.  Measured worst on an MI355X: 2.41e-6 (lm_n2, normals);
# every other tensor <= 2.2e-6, the pivoted reverse pass (grad_n2_negdamp) 6.1e-7.  The broken references measured
# dC 8.5e-5 / 8.3e-5 / 9.0e-5 (lm_n1, grad_n1, grad_n2_negdamp), sigma >= 1.7e-3, damp 0.14: all >= 10x TOL_G.
TOL_G = 7e-6
_W = torch.randn(4, 4, generator=torch.Generator().manual_seed(11))


def _ref_grads(src, tgt, nrm, n, damp, grad, ablate=()):
    x = [v.double().clone().requires_grad_(True) for v in (src, tgt, nrm, torch.eye(4))]
    T, log = st.loop_f64(*x, n, damp, grad, ablate)
    (T * _W.double()).sum().backward()
    return T.detach(), [v.grad for v in x], log


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def _errs(mine, ref):
    """max |g - g_ref| per input tensor (src, tgt, nrm, T0) over the largest |g_ref| entry of that tensor, floored at 1e-2
    of the largest entry of all four (the inputs are all O(1) here).  The floor matters where a loop has converged onto
    exact correspondences: T then no longer depends on the normals, their true gradient cancels to ~1e-8 of the others,
    and fp32 cannot resolve a quantity that small."""
    big = max(float(b.abs().max()) for b in ref)
    return [float((a.double() - b.double()).abs().max()) / max(float(b.abs().max()), 1e-2 * big) for a, b in zip(mine, ref)]


@pytest.mark.gpu
@pytest.mark.parametrize("flag", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("case", list(GRAD_CASES))
def test_loop_gradients_vs_float64(gs, case, flag):
    name, n, damp, grad, terms = GRAD_CASES[case]
    src, tgt, nrm = scene(name)
    T_ref, g_ref, log = _ref_grads(src, tgt, nrm, n, damp, grad)
    # the discrete choices: unambiguous associations, the same accept decisions and se3_exp branches as the kernel
    assert min(r["gap"] for r in log) > 1e-2, [r["gap"] for r in log]
    _, best, tr = gs.ops.icp_device_loop(src.to(DEV), tgt.to(DEV), nrm.to(DEV), torch.eye(4, device=DEV), n, damp, None,
                                         grad_params=grad, want_trace=True, want_best=True)
    tr = tr.cpu().numpy()
    assert torch.equal(gs.ops.knn1_unpack(best)[1].cpu(), log[-1]["idx"]), case
    T_prev = np.eye(4)
    for k, r in enumerate(log):
        o = st.step(tr[k], T_prev, grad)
        assert o["accept"] == r["accept"] and o["small"] == r["small"], (case, k)
        if grad is not None:
            assert o["ssmall"] == r["ssmall"], (case, k)
        T_prev = o["T"]
    # the gradients
    old = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(flag)
    try:
        x = [v.to(DEV).clone().requires_grad_(True) for v in (src, tgt, nrm, torch.eye(4))]
        T, _ = gs.ops.icp_loop_autograd(*x, n, damp, None, grad_params=grad)
        (T * _W.to(DEV)).sum().backward()
        torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(old)
    mine = [v.grad.cpu() for v in x]
    assert _rel(T.detach().cpu(), T_ref) < 1e-5
    errs = _errs(mine, g_ref)
    print(case, flag, "paths", [st.step(tr[k], np.eye(4), grad)["path"] for k in range(n)],
          "small", [r["small"] for r in log], "grad err", ["%.2e" % e for e in errs],
          "scale", ["%.1e" % float(b.abs().max()) for b in g_ref], "plain rel", ["%.1e" % _rel(a, b) for a, b in zip(mine, g_ref)])
    for key, e, a in zip(("src", "tgt", "nrm", "T0"), errs, mine):
        assert torch.isfinite(a).all() and e <= TOL_G, (case, key, e)
    # the test sees a missing adjoint term: the reference without it is >= 10x the bound away
    for term in terms:
        _, g_bad, _ = _ref_grads(src, tgt, nrm, n, damp, grad, (term,))
        d = max(_errs(mine, g_bad))
        print(case, flag, "without", term, "distance %.2e (%.0fx the bound)" % (d, d / TOL_G))
        assert d >= 10 * TOL_G, (case, term, d)
