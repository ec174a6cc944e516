"""The frame intake's stand-alone kernels against plain restatements: the multi-array compaction and its adjoint
(gs_compact_multi / gs_expand_multi behind ops.compact_multi_raw, mask_select_multi, select_rows_multi), the frame
downsample (gs_downsample_frame, out_pix included) and the raw-frame conversion (gs_frames_from_raw).

Compaction and downsample move words: every comparison is bitwise, against torch boolean-mask indexing and strided
slicing.  The conversion is compared with a float64 restatement of the rule in the kernel's header comment -- depth =
uint16 / scale at source pixel floor(y * (Hs / Hd)), clamped; colour bilinear with pixel centres at +0.5 and clamped
edges, optionally / 255; float64 throughout, rounded once -- which a CPU test shows to be the host path of the datasets
(datasets._base.resize_nearest / resize_bilinear and their scaling) to the last bit of float64.  Depth is a single
division and must match bitwise; colour must be a float32 neighbour of the float64 value, (0.5 + 2^-20) ulp: the kernel's
float64 expression may be contracted into fused multiply-adds, whose float64 rounding differences (2^-53 relative) are
far below the 2^-20 ulp of slack.  No tolerance here was measured on the code under test.
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

DEV = "cuda:0"

# the sizes of the gs_compact_rows seam test: 1024 items per block; 1024 * 1024 rows are 1024 blocks, the last size that
# scans its block counts inside the write pass, one row more takes the scan launch
SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049, 1024 * 1024, 1024 * 1024 + 1]
WIDTHS = [(3,), (3, 1), (3, 3, 3, 1), (6, 1, 4, 2)]


@pytest.fixture(scope="module")
def gs():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import gradslam_amd

    gradslam_amd._native.lib()  # fail loudly if the extension is missing
    return gradslam_amd


def _bits(x):
    return x.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------- a) compaction
def _masks(n):
    i = torch.arange(n)
    out = {"none": torch.zeros(n, dtype=torch.bool), "all": torch.ones(n, dtype=torch.bool), "first": i == 0, "last": i == n - 1,
           "3mod4": (i % 4) == 3}
    if n >= 1023:
        out["random30"] = torch.rand(n, generator=torch.Generator().manual_seed(n)) < 0.3
    return out


def _words(n, widths, seed):
    """Arrays of arbitrary 32-bit words (NaN payloads, -0.0, subnormals included) typed float32."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(-2 ** 31, 2 ** 31, (n, w), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32) for w in widths]


def _upstream(k, widths, seed):
    """Random float32 gradients with some -0.0 and NaN entries."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for w in widths:
        x = torch.randn(k, w, generator=g)
        r = torch.rand(k, w, generator=g)
        x[r < 0.1] = -0.0
        x[r > 0.9] = float("nan")
        out.append(x)
    return out


def _raw_multi(nv, name, k, srcs, widths, outs, mask8, n, cnt=None, short=0):
    a_src = (ctypes.c_void_p * max(len(srcs), 1))(*[None if s is None else s.data_ptr() for s in srcs])
    a_out = (ctypes.c_void_p * max(len(outs), 1))(*[None if o is None else o.data_ptr() for o in outs])
    a_w = (ctypes.c_int * max(len(widths), 1))(*widths)
    need = nv.ws_bytes("gs_compact_ws_bytes", n)
    ws = nv.workspace(need, DEV, "compact_test")
    if name == "gs_compact_multi":
        nv.call(name, k, a_src, a_w, a_out, nv.ptr(mask8), n, nv.ptr(cnt), nv.ptr(ws), need - short, nv.stream())
    else:
        nv.call(name, k, a_src, a_w, a_out, nv.ptr(mask8), n, nv.ptr(ws), need - short, nv.stream())
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_compact_multi_seams(gs, n):
    """Forward: every output is x[mask] bit for bit and the device count is mask.sum(), for one to four arrays, bool and
    uint8 masks, through compact_multi_raw, mask_select_multi (count read, count supplied) and select_rows_multi (gradients
    on and off).  Backward of mask_select_multi: zeros.index_put(mask, g) bit for bit, +0.0 words at rejected rows."""
    from gradslam_amd import ops

    masks = {name: m.to(DEV) for name, m in _masks(n).items()}
    for widths in WIDTHS:
        # (references by torch's own boolean indexing on the device, as in the gs_compact_rows seam test)
        xs = [x.to(DEV) for x in _words(n, widths, 13 * n + len(widths))]
        leaves = [x.clone().requires_grad_(True) for x in xs]      # the same words (NaNs and all) as float leaves
        ups_all = [u.to(DEV) for u in _upstream(n, widths, n + len(widths))]
        for name, mb in masks.items():
            want = [x[mb] for x in xs]
            k = int(mb.sum())
            ups = [u[:k].contiguous() for u in ups_all]
            want_g = [torch.zeros((n, w), device=DEV).index_put((mb,), u) for w, u in zip(widths, ups)]
            for m in (mb, mb.to(torch.uint8)):
                tag = (name, widths, m.dtype)
                outs, cnt = ops.compact_multi_raw(xs, m)
                assert int(cnt) == k and cnt.dtype == torch.int32, tag
                assert all(o.shape == x.shape for o, x in zip(outs, xs)), tag
                assert all(torch.equal(_bits(o[:k]), _bits(w)) for o, w in zip(outs, want)), tag
                with torch.no_grad():
                    for got in (ops.mask_select_multi(xs, m), ops.mask_select_multi(xs, m, n=k), ops.select_rows_multi(xs, m),
                                ops.select_rows_multi(leaves, m)):
                        assert all(g.shape == w.shape and torch.equal(_bits(g), _bits(w)) for g, w in zip(got, want)), tag
                ys = ops.select_rows_multi(leaves, m)
                assert all(y.requires_grad and torch.equal(_bits(y), _bits(w)) for y, w in zip(ys, want)), tag
                torch.autograd.backward(ys, ups)
                for x, wg in zip(leaves, want_g):
                    assert torch.equal(_bits(x.grad), _bits(wg)), tag
                    assert not _bits(x.grad)[~mb].any(), tag
                    x.grad = None


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_expand_multi_overwrites_every_row(gs, n):
    """The raw gs_expand_multi on NaN-filled outputs: selected rows receive their compacted row, every rejected row is
    written with +0.0 words (no NaN survives) -- the skip() writer, with no count output."""
    from gradslam_amd import _native as nv

    masks = {name: m.to(DEV) for name, m in _masks(n).items()}
    for widths in [(3, 1), (6, 1, 4, 2)]:
        ups_all = [u.to(DEV) for u in _upstream(n, widths, 3 * n + len(widths))]
        for name, mb in masks.items():
            k = int(mb.sum())
            ups = [u[:k].contiguous() for u in ups_all]
            want = [torch.zeros((n, w), device=DEV).index_put((mb,), u) for w, u in zip(widths, ups)]
            outs = [torch.full((n, w), float("nan"), device=DEV) for w in widths]
            # (an empty selection leaves nothing to read: any valid pointer stands in, as in the wrapper)
            _raw_multi(nv, "gs_expand_multi", len(widths), ups if k else outs, widths, outs, mb.to(torch.uint8), n)
            for o, w in zip(outs, want):
                assert torch.equal(_bits(o), _bits(w)), (name, widths)
                assert not _bits(o)[~mb].any() and not torch.isnan(o[~mb]).any(), (name, widths)


@pytest.mark.gpu
def test_multi_compaction_of_no_rows(gs):
    """n = 0.  Through the wrapper an empty tensor has either a NULL data pointer, which gs_compact_multi refuses by name,
    or a real one, and then every result is empty; with real buffers and n = 0 the count is zero and neither
    gs_compact_multi nor gs_expand_multi writes anything."""
    from gradslam_amd import _native as nv
    from gradslam_amd import ops

    empty = [torch.empty((0, 3), device=DEV), torch.empty((0, 1), device=DEV)]
    mask = torch.empty((0,), dtype=torch.bool, device=DEV)
    for fn in (ops.select_rows_multi, ops.mask_select_multi):
        try:
            got = fn(empty, mask)
        except RuntimeError as e:
            assert "gs_compact_multi" in str(e)
        else:
            assert [tuple(g.shape) for g in got] == [(0, 3), (0, 1)]
    srcs = [torch.rand((4, 3), device=DEV), torch.rand((4, 1), device=DEV)]
    m8 = torch.ones(4, dtype=torch.uint8, device=DEV)
    outs = [torch.full((4, 3), -5.0, device=DEV), torch.full((4, 1), -5.0, device=DEV)]
    cnt = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    _raw_multi(nv, "gs_compact_multi", 2, srcs, (3, 1), outs, m8, 0, cnt)
    assert int(cnt) == 0 and all(bool((o == -5.0).all()) for o in outs)
    _raw_multi(nv, "gs_expand_multi", 2, srcs, (3, 1), outs, m8, 0)
    assert all(bool((o == -5.0).all()) for o in outs)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["gs_compact_multi", "gs_expand_multi"])
def test_multi_compaction_refusals(gs, entry):
    """0 arrays, 5 arrays, a NULL member and a short workspace are refused by name, and nothing is written."""
    from gradslam_amd import _native as nv

    n = 2049
    srcs = [torch.rand((n, 3), device=DEV) for _ in range(5)]
    outs = [torch.full((n, 3), -5.0, device=DEV) for _ in range(5)]
    m8 = torch.ones(n, dtype=torch.uint8, device=DEV)
    cnt = torch.full((1,), -1, dtype=torch.int32, device=DEV)

    def refused(k, s, o, short=0):
        with pytest.raises(RuntimeError) as e:
            _raw_multi(nv, entry, k, s, (3,) * len(s), o, m8, n, cnt, short)
        torch.cuda.synchronize()
        assert all(bool((x == -5.0).all()) for x in outs) and int(cnt) == -1
        return str(e.value)

    for k in (0, 5):
        msg = refused(k, srcs, outs)
        assert entry + ":" in msg and "1..4 arrays" in msg and "code -1" in msg, msg
    msg = refused(3, [srcs[0], None, srcs[2]], outs[:3])
    assert entry + ": NULL array 1" in msg and "code -1" in msg, msg
    msg = refused(3, srcs[:3], [outs[0], outs[1], None])
    assert entry + ": NULL array 2" in msg, msg
    msg = refused(2, srcs[:2], outs[:2], short=1)
    assert entry + ": workspace too small" in msg and "code -2" in msg, msg
    _raw_multi(nv, entry, 4, srcs[:4], (3,) * 4, outs[:4], m8, n, cnt)   # the plain call next to them
    assert all(torch.equal(o, s) for o, s in zip(outs[:4], srcs[:4]))


# ---------------------------------------------------------------------------------------------- b) frame downsample
DS_SHAPES = [(5, 7, 2), (33, 65, 4), (17, 19, 1), (8, 8, 8), (6, 9, 16), (64, 80, 5), (40, 1030, 1)]
_SPECIALS = (0.0, -1.0, float("nan"), float("inf"), 1e-40, -0.0, -float("inf"))


@functools.lru_cache(maxsize=None)
def _ds_case(B, H, W, ds):
    """float32 CPU (depth (B,1,H,W,1), gV, gN, rgb (B,1,H,W,3)).  Element 0 is dense, element 1 keeps about half, the last
    of three keeps nothing on the grid (and is positive everywhere off it); 0, -1, NaN, +-inf, a subnormal and -0.0 sit
    on grid pixels and, where there are any, on pixels off the grid."""
    g = torch.Generator().manual_seed(H * 1000 + W * 10 + ds + B)
    depth = torch.rand(B, 1, H, W, 1, generator=g) + 0.5
    on = torch.zeros(H, W, dtype=torch.bool)
    on[::ds, ::ds] = True
    on_idx, off_idx = on.flatten().nonzero().view(-1), (~on).flatten().nonzero().view(-1)
    for b in range(B):
        d = depth[b].view(-1)
        if b == 1:
            d[on_idx[torch.rand(len(on_idx), generator=g) < 0.5]] = 0.0
        if B == 3 and b == 2:
            d[on_idx] = torch.tensor(_SPECIALS[:3] + _SPECIALS[5:])[torch.arange(len(on_idx)) % 5]
            continue
        for k, v in enumerate(_SPECIALS):
            if len(on_idx) > 1:
                d[on_idx[(5 * k + 1) % len(on_idx)]] = v      # (never grid pixel 0 of a one-pixel grid: it stays valid)
            if len(off_idx):
                d[off_idx[(7 * k + 2) % len(off_idx)]] = v
    gV, gN, rgb = (torch.rand(B, 1, H, W, 3, generator=g) for _ in range(3))
    return depth, gV, gN, rgb


def _ds_expected(case, ds):
    depth, gV, gN, rgb = case
    out = []
    for b in range(depth.shape[0]):
        m = depth[b, 0, ::ds, ::ds, 0] > 0           # NaN is rejected, +inf and the subnormal are kept
        out.append(tuple(x[b, 0, ::ds, ::ds][m] for x in (gV, gN, rgb)) + (m.flatten().nonzero().view(-1).to(torch.int32),))
    return out


def _raw_downsample(nv, depth, gV, gN, rgb, ds, cap, outs, pix, counts):
    B, _, H, W = depth.shape[:4]
    ws = nv.workspace(nv.ws_bytes("gs_downsample_frame_ws_bytes", H, W, ds), DEV, "downsample_test")
    nv.call("gs_downsample_frame", nv.ptr(depth), nv.ptr(gV), nv.ptr(gN), nv.ptr(rgb), B, H, W, ds, cap, nv.ptr(outs[0]),
            nv.ptr(outs[1]), nv.ptr(outs[2]), nv.ptr(pix), nv.ptr(counts), nv.ptr(ws), ws.numel(), nv.stream())
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,ds", DS_SHAPES)
@pytest.mark.parametrize("B", [1, 3])
def test_downsample_frame_is_strided_slicing(gs, B, H, W, ds):
    """Points, normals and colours are [::ds, ::ds] of the maps at the pixels with depth > 0, bit for bit in row-major
    grid order; counts exact; rows at and beyond the count stay zero through the wrapper and untouched through the raw
    call, whose out_pix holds the ds-grid pixel ids r * Wd + c."""
    from gradslam_amd import _native as nv
    from gradslam_amd import ops

    case = _ds_case(B, H, W, ds)
    want = _ds_expected(case, ds)
    Hd, Wd = -(-H // ds), -(-W // ds)
    ks = [len(w[3]) for w in want]
    assert ks[0] > 0 and (B == 1 or (ks[2] == 0 and (Hd * Wd == 1 or ks[0] != ks[1])))
    dev = [x.to(DEV) for x in case]
    op, on, oc, counts = ops.downsample_frame_raw(*dev, ds)
    assert counts.dtype == torch.int32 and counts.tolist() == ks
    for got, which in ((op, 0), (on, 1), (oc, 2)):
        assert got.shape == (B, Hd * Wd, 3)
        for b in range(B):
            assert torch.equal(_bits(got[b, :ks[b]]).cpu(), _bits(want[b][which])), (b, which)
            assert not _bits(got[b, ks[b]:]).any(), (b, which)
    cap = Hd * Wd + 3
    outs = [torch.full((B, cap, 3), -5.0, device=DEV) for _ in range(3)]
    pix = torch.full((B, cap), -7, dtype=torch.int32, device=DEV)
    counts = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    _raw_downsample(nv, *dev, ds, cap, outs, pix, counts)
    assert counts.tolist() == ks
    for b in range(B):
        for which in range(3):
            assert torch.equal(_bits(outs[which][b, :ks[b]]).cpu(), _bits(want[b][which])), (b, which)
            assert bool((outs[which][b, ks[b]:] == -5.0).all()), (b, which)
        assert torch.equal(pix[b, :ks[b]].cpu(), want[b][3]) and bool((pix[b, ks[b]:] == -7).all()), b


@pytest.mark.gpu
def test_downsample_frame_output_subsets_and_refusals(gs):
    """Any subset of the three outputs may be requested (the others stay untouched); an output without its source map and
    a capacity one below the grid size are refused by name."""
    from gradslam_amd import _native as nv

    B, H, W, ds = 3, 5, 7, 2
    case = _ds_case(B, H, W, ds)
    want = _ds_expected(case, ds)
    ks = [len(w[3]) for w in want]
    depth, gV, gN, rgb = (x.to(DEV) for x in case)
    cap = 3 * 4
    for sel in itertools.product((False, True), repeat=3):
        for with_pix in (False, True):
            outs = [torch.full((B, cap, 3), -5.0, device=DEV) for _ in range(3)]
            pix = torch.full((B, cap), -7, dtype=torch.int32, device=DEV)
            counts = torch.full((B,), -1, dtype=torch.int32, device=DEV)
            _raw_downsample(nv, depth, gV, gN, rgb, ds, cap, [o if s else None for o, s in zip(outs, sel)], pix if with_pix else None,
                            counts)
            assert counts.tolist() == ks, sel
            for b in range(B):
                for which in range(3):
                    k = ks[b] if sel[which] else 0
                    assert torch.equal(_bits(outs[which][b, :k]).cpu(), _bits(want[b][which][:k])), (sel, b, which)
                    assert bool((outs[which][b, k:] == -5.0).all()), (sel, b, which)
                k = ks[b] if with_pix else 0
                assert torch.equal(pix[b, :k].cpu(), want[b][3][:k]) and bool((pix[b, k:] == -7).all()), (sel, b)
    outs = [torch.full((B, cap, 3), -5.0, device=DEV) for _ in range(3)]
    counts = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    for srcs in ((None, gN, rgb), (gV, None, rgb), (gV, gN, None)):
        with pytest.raises(RuntimeError) as e:
            _raw_downsample(nv, depth, *srcs, ds, cap, outs, None, counts)
        assert "gs_downsample_frame" in str(e.value) and "without its source" in str(e.value), str(e.value)
    with pytest.raises(RuntimeError) as e:
        _raw_downsample(nv, depth, gV, gN, rgb, ds, cap - 1, outs, None, counts)
    assert "gs_downsample_frame: cap (11)" in str(e.value) and "(12)" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert all(bool((o == -5.0).all()) for o in outs) and bool((counts == -1).all())


# ---------------------------------------------------------------------------------------------- c) raw frames
RAW_SHAPES = [((6, 8), (6, 8)), ((12, 16), (6, 8)), ((7, 9), (5, 4)), ((3, 4), (7, 9)), ((1, 5), (3, 5)), ((5, 1), (5, 3)),
              ((48, 64), (30, 40))]
# The ABI takes depth_scale as a C float: the scales are float32-representable numbers, so the kernel divides by the very
# number the restatement divides by.
SCALES = (5000.0, 1000.0, 1.0)
assert all(float(np.float32(s)) == s for s in SCALES)


@functools.lru_cache(maxsize=None)
def _raw_case(B, Hs, Ws):
    """(depth (B,Hs,Ws) int64 values in [0, 65535] with 0, 1 and 65535 among them, rgb (B,Hs,Ws,3) uint8)."""
    g = torch.Generator().manual_seed(Hs * 100 + Ws + B)
    depth = torch.randint(0, 65536, (B, Hs, Ws), generator=g)
    flat = depth.view(B, -1)
    flat[:, -1] = 65535
    for k, v in enumerate((0, 65535, 1)):
        flat[:, (2 * k) % flat.shape[1]] = v
    rgb = torch.randint(0, 256, (B, Hs, Ws, 3), generator=g, dtype=torch.uint8)
    rgb.view(B, -1)[:, :2] = torch.tensor([0, 255], dtype=torch.uint8)
    return depth, rgb


def _taps(n_out, n_in):
    f = (torch.arange(n_out, dtype=torch.float64) + 0.5) * (n_in / n_out) - 0.5
    i0 = torch.floor(f).to(torch.int64)
    f = f - i0
    f[i0 < 0] = 0.0
    i0 = i0.clamp_min(0)
    f[i0 >= n_in - 1] = 0.0
    i0 = i0.clamp_max(n_in - 1)
    return i0, (i0 + 1).clamp_max(n_in - 1), f


def _restate(depth, rgb, Hd, Wd, scale, normalise):
    """float64 (depth (B,Hd,Wd,1), rgb (B,Hd,Wd,3)) of the rule stated in the module docstring."""
    B, Hs, Ws = depth.shape
    ys = torch.floor(torch.arange(Hd, dtype=torch.float64) * (Hs / Hd)).to(torch.int64).clamp_max(Hs - 1)
    xs = torch.floor(torch.arange(Wd, dtype=torch.float64) * (Ws / Wd)).to(torch.int64).clamp_max(Ws - 1)
    d = (depth.double()[:, ys][:, :, xs] / scale).unsqueeze(-1)
    a = rgb.double()
    y0, y1, fy = _taps(Hd, Hs)
    x0, x1, fx = _taps(Wd, Ws)
    fx, fy = fx[None, None, :, None], fy[None, :, None, None]
    top = a[:, y0][:, :, x0] * (1.0 - fx) + a[:, y0][:, :, x1] * fx
    bot = a[:, y1][:, :, x0] * (1.0 - fx) + a[:, y1][:, :, x1] * fx
    c = top * (1.0 - fy) + bot * fy
    return d, (c / 255.0 if normalise else c)


def test_restatement_is_the_datasets_host_path():
    """_restate agrees with SequenceDataset's host conversion (resize_nearest / resize_bilinear and the datasets' scaling)
    to the last bit of float64, and its nearest-neighbour indices are floor(y Hs / Hd) in exact integer arithmetic: the
    host path and this file state one rule."""
    from gradslam_amd.datasets._base import SequenceDataset

    for (Hs, Ws), (Hd, Wd) in RAW_SHAPES:
        depth, rgb = _raw_case(3, Hs, Ws)
        ys = torch.floor(torch.arange(Hd, dtype=torch.float64) * (Hs / Hd)).to(torch.int64)
        xs = torch.floor(torch.arange(Wd, dtype=torch.float64) * (Ws / Wd)).to(torch.int64)
        assert ys.tolist() == [y * Hs // Hd for y in range(Hd)] and xs.tolist() == [x * Ws // Wd for x in range(Wd)]
        for scale, normalise in itertools.product(SCALES, (False, True)):
            host = SequenceDataset.__new__(SequenceDataset)
            host.height, host.width, host.channels_first = Hd, Wd, False
            host.normalize_color, host.scaling_factor = normalise, scale
            d, c = _restate(depth, rgb, Hd, Wd, scale, normalise)
            for b in range(3):
                hd = host._preprocess_depth(depth[b].numpy().astype(np.int64))
                hc = host._preprocess_color(rgb[b].numpy().astype(float))
                assert hd.dtype == np.float64 and np.array_equal(hd, d[b].numpy()), (Hs, Ws, Hd, Wd, scale)
                assert hc.dtype == np.float64 and np.array_equal(hc, c[b].numpy()), (Hs, Ws, Hd, Wd, normalise)
        if (Hs, Ws) == (Hd, Wd):
            assert torch.equal(_restate(depth, rgb, Hd, Wd, 1.0, False)[1], rgb.double())


def _storage(depth):
    """uint16 values as the int16 storage the datasets hand over."""
    return torch.from_numpy(depth.numpy().astype(np.uint16).view(np.int16))


def _ulp32(x):
    """Spacing of float32 at |x| (float64 tensor of normal float32 magnitudes, or zero)."""
    _, e = torch.frexp(x.abs())
    return torch.where(x == 0, torch.zeros_like(x), torch.ldexp(torch.ones_like(x), e - 24))


@pytest.mark.gpu
@pytest.mark.parametrize("src,dst", RAW_SHAPES)
@pytest.mark.parametrize("B", [1, 3])
def test_frames_from_raw_against_float64(gs, B, src, dst):
    """Depth is float32(float64(u16) / scale) bit for bit; colour is a float32 neighbour of the float64 value, and exact
    for a same-size frame without normalisation; depth only, colour only and both give the same tensors."""
    from gradslam_amd import ops

    (Hs, Ws), (Hd, Wd) = src, dst
    depth, rgb = _raw_case(B, Hs, Ws)
    d16, rgb_dev = _storage(depth).to(DEV), rgb.to(DEV)
    assert {0, 1, 65535} <= set(depth.unique().tolist())
    for scale, normalise in itertools.product(SCALES, (False, True)):
        rd, rc = _restate(depth, rgb, Hd, Wd, scale, normalise)
        for with_d, with_c in ((True, False), (False, True), (True, True)):
            tag = (scale, normalise, with_d, with_c)
            gd, gc = ops.frames_from_raw(d16 if with_d else None, rgb_dev if with_c else None, Hd, Wd, scale, normalise)
            assert (gd is None) == (not with_d) and (gc is None) == (not with_c), tag
            if with_d:
                assert gd.shape == (B, Hd, Wd, 1) and gd.dtype == torch.float32
                assert torch.equal(_bits(gd).cpu(), _bits(rd.float())), tag
            if with_c:
                assert gc.shape == (B, Hd, Wd, 3) and gc.dtype == torch.float32
                err = (gc.cpu().double() - rc).abs()
                assert bool((err <= (0.5 + 2.0 ** -20) * _ulp32(rc)).all()), (tag, float(err.max()))
                if (Hs, Ws) == (Hd, Wd) and not normalise:
                    assert torch.equal(gc.cpu(), rgb.float()), tag


@pytest.mark.gpu
def test_frames_from_raw_refusals(gs):
    """B = 0, a non-positive scale with depth given, an input with a NULL output and both inputs NULL are refused by name;
    the wrapper raises ValueError for a non-contiguous depth and for a colour tensor that is not uint8."""
    from gradslam_amd import _native as nv
    from gradslam_amd import ops

    depth, rgb = _raw_case(1, 6, 8)
    d16, rgb_dev = _storage(depth).to(DEV), rgb.to(DEV)
    od, oc = torch.full((1, 6, 8, 1), -5.0, device=DEV), torch.full((1, 6, 8, 3), -5.0, device=DEV)

    def refused(d_in, c_in, B, scale, d_out, c_out):
        with pytest.raises(RuntimeError) as e:
            nv.call("gs_frames_from_raw", nv.ptr(d_in), nv.ptr(c_in), B, 6, 8, 6, 8, scale, 0, nv.ptr(d_out), nv.ptr(c_out), nv.stream())
        assert "gs_frames_from_raw:" in str(e.value) and "code -1" in str(e.value), str(e.value)
        return str(e.value)

    assert "bad shape" in refused(d16, rgb_dev, 0, 5000.0, od, oc)
    for scale in (0.0, -1.0):
        assert "depth_scale" in refused(d16, rgb_dev, 1, scale, od, oc)
    assert "NULL output" in refused(d16, rgb_dev, 1, 5000.0, None, oc)
    assert "NULL output" in refused(d16, rgb_dev, 1, 5000.0, od, None)
    refused(None, None, 1, 5000.0, od, oc)
    torch.cuda.synchronize()
    assert bool((od == -5.0).all()) and bool((oc == -5.0).all())
    # a non-positive scale is no obstacle without depth
    nv.call("gs_frames_from_raw", None, nv.ptr(rgb_dev), 1, 6, 8, 6, 8, 0.0, 0, None, nv.ptr(oc), nv.stream())
    assert torch.equal(oc.cpu(), rgb.float().view(1, 6, 8, 3))
    with pytest.raises(ValueError):
        ops.frames_from_raw(d16.transpose(1, 2), None, 6, 8, 5000.0, False)
    with pytest.raises(ValueError):
        ops.frames_from_raw(d16.to(torch.int32), None, 6, 8, 5000.0, False)
    with pytest.raises(ValueError):
        ops.frames_from_raw(None, rgb_dev.float(), 6, 8, 5000.0, False)
    with pytest.raises(ValueError):
        ops.frames_from_raw(None, rgb_dev.transpose(1, 2), 6, 8, 5000.0, False)
