"""The harness of tests/test_workspace_exact.py and tests/test_workspace_exact_families.py (not a test file): an entry point
whose workspace comes from one `*_layout` function runs in a workspace of EXACTLY the queried size, whatever the bytes held.

A case makes its call the way the package does -- through `ops`, whose `call` / `ptr` / `workspace` are watched, or, for the
entries `ops` has no wrapper for, in `ops`' words.  `check_exact` then issues the recorded call again through `_native.call`,
argument for argument:
  * the reference run: the cached, roomy workspace of `ops` (rounded up to a power of two) -- after `dirty()`, a call of the same
    kind at a larger shape on the same workspace tag, so that it starts from what a real neighbouring call left there;
  * twice at exactly the queried size, GUARD bytes into a buffer of 0xA5 (a tiny negative float, a large negative integer) and
    of 0xFF (a NaN, -1) with GUARD more behind it: every guard byte survives, every compared output carries the reference's
    bits (whole buffers: what a kernel leaves unwritten keeps the fill in all runs).  An entry whose kernels add floats
    atomically into its outputs (`bitwise=False`) is held to this instead: finite wherever the reference is, and no word
    still the fill where the reference wrote;
  * a queried size of 0: the pointer at the guard boundary with ws_bytes = 0, guards checked, nothing else;
  * one byte less: RuntimeError "workspace too small", code -2, outputs untouched;
  * `tape=`: the tape argument gets the same treatment at exactly its queried size -- a guarded buffer of its own, compared
    whole where the entry writes it (its inside starts from the outputs' fill), copied in where the entry reads it, and, where
    the entry is told its size, one byte less refused with "tape too small".
An overrun of less than GUARD bytes is caught without leaving the allocation."""
import contextlib
import os
import re

import pytest
import torch

DEV = "cuda:0"
GUARD = 4096
POISONS = (0xA5, 0xFF)

REGISTRY = {}  # test module -> the entry points its cases cover


def covers(module, *entries):
    """Decorator of a case: registers the entry points it hands to check_exact (at import: the CPU test of the list reads it)."""
    REGISTRY.setdefault(module, set()).update(entries)
    return lambda fn: fn


HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gradslam_hip.h")


def header_params(header_text):
    """name -> [parameter names] of every gs_* declaration of the header, in header order."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*|^[ \t]*#[^\n]*", "", header_text, flags=re.S | re.M)
    return {name: [p.replace("*", " ").split()[-1] for p in params.split(",") if p.split() not in ([], ["void"])]
            for name, params in re.findall(r"\b(gs_\w+)\s*\(([^()]*)\)\s*;", text)}


def header_entries(header_text):
    """Every gs_* declaration of the header that takes a workspace or a sized tape (the size queries take neither)."""
    return {name for name, params in header_params(header_text).items() if {"ws_bytes", "tape_bytes", "tape_size"} & set(params)}


with open(HEADER) as _f:
    PARAMS = header_params(_f.read())


def at(entry, *names):
    """The argument positions of the named parameters of `entry`, as the header declares them."""
    return [PARAMS[entry].index(n) for n in names]


class Watch:
    """ops.call / ops.ptr / ops.workspace while a case runs: the calls made, the tensors behind their pointers (kept alive),
    the size each workspace was asked for."""

    def __init__(self, monkeypatch, gs):
        self.nv, self.calls, self.tensors, self.asked = gs._native, [], {}, {}
        monkeypatch.setattr(gs.ops, "call", self.call)
        monkeypatch.setattr(gs.ops, "ptr", self.ptr)
        monkeypatch.setattr(gs.ops, "workspace", self.workspace)

    def call(self, name, *args):
        self.calls.append((name, args, dict(self.asked)))  # (asked: two calls of a case may share one cached workspace)
        return self.nv.call(name, *args)

    def ptr(self, t):
        if t is not None:
            self.tensors[t.data_ptr()] = t
        return self.nv.ptr(t)

    def workspace(self, nbytes, device, tag="default"):
        ws = self.nv.workspace(nbytes, device, tag)
        self.asked[ws.data_ptr()] = int(nbytes)
        return ws


def _bytes(t):
    return t.reshape(-1).view(torch.uint8)


def _words(b):
    return b[: b.numel() // 4 * 4].view(torch.int32)


def check_exact(gs, monkeypatch, entry, run, outs, bitwise=True, fill=0x5A, compare=None, dirty=None, tape=None, tape_out=False,
                tape_sized=True, inout=(), ws_at=-3):
    """`run()` makes one call of `entry` (see the module docstring); `outs` are the positions of its output arguments, or the
    output tensors themselves (or a callable that gives them once `run()` has made them); `compare` the subset that is compared
    (default: all); `fill` what the outputs hold before a run (0 for entries that add into them); `inout`: tensors the entry updates in place, put back to what they held before
    `run()` in front of every run and compared like outputs; `dirty()`: see the module docstring; `tape`: the position of the
    tape argument (`tape_out`: the entry writes it; `tape_sized`: its size in bytes is the next argument); `ws_at`: the
    position of the workspace pointer (its size follows it)."""
    assert any(entry in names for names in REGISTRY.values()), entry + " is not registered: decorate the case with covers()"
    nv = gs._native
    before = [(t, t.clone()) for t in inout]
    if dirty is not None:
        dirty()
    w = Watch(monkeypatch, gs)
    run()
    made = [(args, asked) for name, args, asked in w.calls if name == entry]
    assert len(made) == 1, (entry, [name for name, _, _ in w.calls])
    args, asked = list(made[0][0]), made[0][1]
    ws_at = ws_at % len(args)
    ws_ptr, ws_have = args[ws_at], args[ws_at + 1]
    need = 0 if ws_ptr is None else asked[ws_ptr]
    outs = outs() if callable(outs) else outs
    assert need <= ws_have
    resolve = lambda which: [w.tensors[args[o]] if isinstance(o, int) else o for o in which if not isinstance(o, int) or args[o] is not None]
    tensors = resolve(outs)
    compared = (tensors if compare is None else resolve(compare)) + [t for t, _ in before]
    assert (tensors or before) and all(t.is_contiguous() for t in tensors + [t for t, _ in before])
    the_tape = tape_need = None
    if tape is not None:
        tape = tape % len(args)
        the_tape = w.tensors[args[tape]]
        tape_need = the_tape.numel() * the_tape.element_size()
        assert tape_need > 0 and (not tape_sized or args[tape + 1] == tape_need)
        tape_ref = _bytes(the_tape).clone()

    def again(ws, nbytes, value, tape_ptr=None, tape_bytes=None):
        for t in tensors:
            _bytes(t).fill_(value)
        for t, held in before:
            t.copy_(held)
        a = list(args)
        a[ws_at], a[ws_at + 1] = ws, nbytes
        if tape is not None:
            a[tape] = args[tape] if tape_ptr is None else tape_ptr
            if tape_sized:
                a[tape + 1] = tape_need if tape_bytes is None else tape_bytes
            if tape_out and tape_ptr is None:
                _bytes(the_tape).fill_(value)
        nv.call(entry, *a)
        torch.cuda.synchronize()
        return [_bytes(t).clone() for t in compared]

    if dirty is not None:
        dirty()  # (again: `run()` has since left its own bytes there)
    ref = again(ws_ptr, ws_have, fill)
    if tape_out:
        tape_ref = _bytes(the_tape).clone()
    buf = None
    for poison in POISONS:
        buf = torch.full((need + 2 * GUARD,), poison, dtype=torch.uint8, device=DEV)
        tbuf = None
        if tape is not None:
            tbuf = torch.full((tape_need + 2 * GUARD,), poison, dtype=torch.uint8, device=DEV)
            inside = tbuf[GUARD:GUARD + tape_need]
            inside.fill_(fill) if tape_out else inside.copy_(tape_ref)
        got = again(buf.data_ptr() + GUARD, need, fill, None if tbuf is None else tbuf.data_ptr() + GUARD)
        where = "{} on 0x{:02X}".format(entry, poison)
        assert bool((buf[:GUARD] == poison).all()), where + ": wrote in front of its workspace"
        assert bool((buf[GUARD + need:] == poison).all()), where + ": wrote behind its workspace"
        if tbuf is not None:
            assert bool((tbuf[:GUARD] == poison).all()), where + ": wrote in front of its tape"
            assert bool((tbuf[GUARD + tape_need:] == poison).all()), where + ": wrote behind its tape"
            assert torch.equal(tbuf[GUARD:GUARD + tape_need], tape_ref), where + (": the tape differs" if tape_out else ": wrote to the tape it reads")
        for k, (r, g) in enumerate(zip(ref, got)):
            if bitwise:
                assert torch.equal(r, g), (where, "output", k)
                assert fill != 0x5A or k >= len(compared) - len(before) or not bool((g == 0x5A).all()), (where, "output", k, "was never written")
            else:
                rw, gw = _words(r), _words(g)
                finite = torch.isfinite(rw.view(torch.float32))
                assert bool(torch.isfinite(gw.view(torch.float32))[finite].all()), (where, "output", k, "is not finite where the reference is")
                fill_word = _words(torch.full((4,), fill, dtype=torch.uint8, device=DEV))[0]
                assert bool((gw[rw != fill_word] != fill_word).all()), (where, "output", k, "holds the fill where the reference wrote")
        if bitwise:
            assert any(bool((g != fill).any()) for g in got), (where, "wrote nothing")
    held = lambda: (all(bool((_bytes(t) == 0x5A).all()) for t in tensors) and all(torch.equal(t, h) for t, h in before))
    if need > 0:
        with pytest.raises(RuntimeError) as e:
            again(buf.data_ptr() + GUARD, need - 1, 0x5A)
        assert "workspace too small" in str(e.value) and "code -2" in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert held(), entry + ": a refused call wrote to its outputs"
    if tape is not None and tape_sized:
        with pytest.raises(RuntimeError) as e:
            again(buf.data_ptr() + GUARD, need, 0x5A, tbuf.data_ptr() + GUARD, tape_need - 1)
        assert "tape too small" in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert held(), entry + ": a call refused for its tape wrote to its outputs"


@contextlib.contextmanager
def deterministic(on):
    before = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(before)


def frames(gs, B, L, H, W):
    """depth (B,L,H,W,1), rgb (B,L,H,W,3), K (B,1,4,4), poses (B,L,4,4) and the maps of all frames, on the device."""
    from gradslam_amd.synthetic import make_sequence

    c, d, K, P = (x.to(DEV).contiguous() for x in make_sequence(B, L, H, W, seed=0))
    V, N, gV, gN = gs.ops.vertex_normal_maps_raw(d, K, P)
    return dict(rgb=c, depth=d, K=K, P=P, V=V, N=N, gV=gV, gN=gN)


def valid_points(f, b, l):
    """(points, normals) of frame l of sequence b in world coordinates: the pixels with a depth and a normal."""
    ok = (f["depth"][b, l, ..., 0] > 0) & (f["gN"][b, l].abs().sum(-1) > 0)
    return f["gV"][b, l][ok].contiguous(), f["gN"][b, l][ok].contiguous()


def make_clouds(gs, n_src, n_tgt):
    """(src (n_src,3), tgt (n_tgt,3), its normals, T0): the valid points of two neighbouring 24 x 32 frames and a start pose."""
    f = frames(gs, 1, 2, 24, 32)
    tgt, nrm = valid_points(f, 0, 0)
    src, _ = valid_points(f, 0, 1)
    assert tgt.shape[0] >= n_tgt and src.shape[0] >= n_src
    T0 = torch.eye(4, device=DEV)
    T0[0, 3] = 0.004
    return src[:n_src].contiguous(), tgt[:n_tgt].contiguous(), nrm[:n_tgt].contiguous(), T0


def make_table(gs, H, W, Nmax, counts, every=1):
    """Two frames of B = len(counts) sequences with their maps, and a map of the first counts[b] of every `every`-th valid point
    of the first frame in arrays of Nmax rows (mp, mn; cc: ones)."""
    B = len(counts)
    f = frames(gs, B, 2, H, W)
    mp, mn = torch.zeros(B, Nmax, 3, device=DEV), torch.zeros(B, Nmax, 3, device=DEV)
    for b in range(B):
        p, n = (x[::every] for x in valid_points(f, b, 0))
        assert p.shape[0] >= counts[b] and counts[b] <= Nmax, (p.shape[0], counts[b])
        mp[b, :counts[b]], mn[b, :counts[b]] = p[:counts[b]], n[:counts[b]]
    f.update(B=B, H=H, W=W, Nmax=Nmax, mp=mp, mn=mn, counts=torch.tensor(counts, dtype=torch.int32, device=DEV),
             cc=torch.ones(B, Nmax, 1, device=DEV))
    return f
