"""The O(1) step of the ICP loops (step_wave0: folded into the association launches and, for a loop's last step, icp_step_k)
against recorded results, bit for bit.

The step's order of work is free -- the solve may start before the bookkeeping, the SE(3) exponential may be spread over lanes
-- but every value it produces is fixed: same operands, same floating-point operations.  tests/golden/step_chain.npz holds,
for three tiny scenes, the inputs and what gs_icp_point_to_plane (ten iterations, traced) left behind: pose, trace rows and
both copies of the loop state in the workspace.  The scenes, by construction:

  lm        a wavy surface, the source a noisy subset of it under a small motion: the loop converges and then stalls, so the
            LM decision takes both outcomes (trace column 45 holds zeros and ones -- asserted on the recorded trace);
  exact     the source IS a subset of the target and the initial pose is the identity: every residual is exactly zero, so
            g = 0, xi = 0 and |omega| < 1e-6 -- the small-angle branch of the exponential, at every step;
  singular  a plane with one normal and a NEGATIVE damping: H has exact zeros on its diagonal, so the unpivoted elimination
            meets the pivot H_jj + damp < 0 and hands the system to solve6_lu (the pivoted elimination), whose indefinite
            but regular system has a finite solution.

Comparisons are on the words (int32 views): equal bits, whatever a float's value is.
"""
import pytest
import torch

SCENES = ("lm", "exact", "singular")
NUMITERS = 10
DEV = "cuda:0"


def make_scenes():
    """The three scenes (CPU tensors), for tools/gen_golden_step_chain.py, which records the golden file; the tests read the
    inputs from the file, so they do not depend on the generator of the torch build at hand."""
    g = torch.Generator().manual_seed(7)
    out = {}
    # lm: z = 2 + 0.1 sin(3x) + 0.1 cos(2y) over [-1, 1]^2
    xy = torch.rand(300, 2, generator=g) * 2 - 1
    z = 2 + 0.1 * torch.sin(3 * xy[:, 0]) + 0.1 * torch.cos(2 * xy[:, 1])
    tgt = torch.cat([xy, z[:, None]], 1)
    n = torch.stack([-0.3 * torch.cos(3 * xy[:, 0]), 0.2 * torch.sin(2 * xy[:, 1]), torch.ones(300)], 1)
    n = n / n.norm(dim=1, keepdim=True)
    w = torch.tensor([0.01, -0.015, 0.02])
    W = torch.tensor([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = torch.linalg.matrix_exp(W)
    src = (tgt[:150] + 1e-3 * torch.randn(150, 3, generator=g)) @ R.T + torch.tensor([0.01, -0.02, 0.015])
    out["lm"] = dict(src=src.contiguous(), tgt=tgt.contiguous(), nrm=n.contiguous(), damp=1e-8)
    # exact: the source is the head of the target
    out["exact"] = dict(src=tgt[:100].clone().contiguous(), tgt=tgt.contiguous(), nrm=n.contiguous(), damp=1e-8)
    # singular: the plane z = 2, one normal, the source lifted and tilted a little; negative damping
    pxy = torch.rand(200, 2, generator=g) * 2 - 1
    ptgt = torch.cat([pxy, torch.full((200, 1), 2.0)], 1)
    pn = torch.zeros(200, 3)
    pn[:, 2] = 1.0
    psrc = ptgt[:90].clone()
    psrc[:, 2] += 0.01 + 0.02 * psrc[:, 0]
    out["singular"] = dict(src=psrc.contiguous(), tgt=ptgt.contiguous(), nrm=pn.contiguous(), damp=-1e-3)
    return out


def run_point_to_plane(src, tgt, nrm, damp):
    """gs_icp_point_to_plane without hints on a fresh zeroed workspace -> pose, trace, both state copies (host, int32 words)."""
    from gradslam_amd import _native as nv
    from gradslam_amd import ops

    lib = nv.lib()
    src, tgt, nrm = src.to(DEV), tgt.to(DEV), nrm.to(DEV)
    ns, nt = src.shape[0], tgt.shape[0]
    d_ns, d_nt = ops.dev_int(ns, DEV), ops.dev_int(nt, DEV)
    T0 = torch.eye(4, device=DEV)
    ws = torch.zeros(nv.ws_bytes("gs_icp_ws_bytes", ns, nt), dtype=torch.uint8, device=DEV)
    T = torch.zeros(4, 4, device=DEV)
    trace = torch.zeros(NUMITERS, 48, device=DEV)
    rc = lib.gs_icp_point_to_plane(src.data_ptr(), d_ns.data_ptr(), ns, tgt.data_ptr(), nrm.data_ptr(), d_nt.data_ptr(), nt,
                                   T0.data_ptr(), NUMITERS, float(damp), -1.0, None, T.data_ptr(), None, trace.data_ptr(),
                                   ws.data_ptr(), ws.numel(), nv.stream())
    assert rc == 0, lib.gs_last_error()
    torch.cuda.synchronize()
    state = ws[:2 * 512].cpu().view(torch.int32)  # icp.hip icp_ws_layout: state x 2, each 348 bytes in a 256-aligned slot
    return dict(T=T.cpu().view(torch.int32), trace=trace.cpu().view(torch.int32), state=state)


@pytest.fixture(scope="module")
def rec(golden):
    return golden("step_chain")


def test_golden_scenes_cover_the_branches(rec):
    """CPU: the recorded traces show what the scenes were built for."""
    tr = torch.from_numpy(rec["lm.trace"]).view(torch.float32)
    assert (tr[:, 45] == 0).any() and (tr[:, 45] == 1).any()
    # exact: the step solved g = 0 -> xi = 0 at every iteration (columns 36..41 of a trace row are g)
    tr = torch.from_numpy(rec["exact.trace"]).view(torch.float32)
    assert (tr[:, 36:42] == 0).all() and (tr[:, 42] == 0).all()
    # singular: zeros on H's diagonal and a negative damping throughout (it doubles or halves, never changes sign)
    tr = torch.from_numpy(rec["singular.trace"]).view(torch.float32)
    H = tr[:, :36].view(-1, 6, 6)
    assert (torch.diagonal(H, dim1=1, dim2=2) == 0).any(dim=1).all() and (tr[:, 44] < 0).all()
    assert torch.isfinite(torch.from_numpy(rec["singular.T"]).view(torch.float32)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_step_matches_recorded_bits(rec, name):
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    t = lambda k: torch.from_numpy(rec[name + "." + k])
    got = run_point_to_plane(t("src"), t("tgt"), t("nrm"), float(rec[name + ".damp"]))
    for k in ("T", "trace", "state"):
        assert torch.equal(got[k], t(k)), (name, k)
