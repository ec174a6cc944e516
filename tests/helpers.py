"""Shared helpers for the parity tests."""
import math

import numpy as np
import torch


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def cloud_from_golden(g, prefix, nb, feats=True):
    from oracle.cloud import Cloud

    return Cloud([t(g[f"{prefix}_points_{b}"]) for b in range(nb)],
                 [t(g[f"{prefix}_normals_{b}"]) for b in range(nb)],
                 [t(g[f"{prefix}_colors_{b}"]) for b in range(nb)],
                 [t(g[f"{prefix}_feats_{b}"]) for b in range(nb)] if feats else None)


def rel_err(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ------------------------------------------------------------------ the fixed-order fp32 sums (gs_rowsum.hpp), restated
def block_rows_f32(terms, waves):
    """terms (nblocks, waves, 64 lanes, N) float32 -> (nblocks, N): the butterfly (offsets 32 .. 1), then the waves in order
    starting from wave 0's sum."""
    x = terms
    assert x.dtype == np.float32 and x.shape[1:3] == (waves, 64)
    for half in (32, 16, 8, 4, 2, 1):
        x = x[:, :, :half] + x[:, :, half:2 * half]
    x = x[:, :, 0]
    out = x[:, 0]
    for w in range(1, waves):
        out = out + x[:, w]
    assert out.dtype == np.float32
    return out


def fold_rows_f32(rows, groups):
    """rows (nrow, N) float32 -> (N,): rows g, g + groups, .. in ascending order onto +0, then the partial sums g = 0, 1, ..
    in ascending order (onto +0: the first of them is never -0)."""
    nrow, N = rows.shape
    pad = -nrow % groups
    x = np.concatenate([rows, np.zeros((pad, N), np.float32)]).reshape(-1, groups, N)
    acc = np.zeros((groups, N), np.float32)
    for it in range(x.shape[0]):
        acc = acc + x[it]
    t = acc[0]
    for g in range(1, groups):
        t = t + acc[g]
    assert t.dtype == np.float32
    return t


# ------------------------------------------------------------------ exact sums of fp32 values (the references of the folds)
def f32_to_int(bits):
    """fp32 bit patterns (finite) -> Python integers in units of 2^-149 (exact)."""
    bits = np.asarray(bits, dtype=np.uint32).astype(np.int64)
    e, m = (bits >> 23) & 0xFF, bits & 0x7FFFFF
    mant = np.where(e > 0, m | 0x800000, m)
    shift = np.maximum(e, 1) - 1
    sign = np.where(bits >> 31, -1, 1)
    return [int(s) * (int(a) << int(k)) for s, a, k in zip(sign.ravel(), mant.ravel(), shift.ravel())]


def int_to_f32(t, unit=-149):
    """A Python integer in units of 2^unit (default 2^-149) -> the nearest fp32 (ties to even), rounded once: to 24 bits, or
    to the subnormal quantum 2^-149 where that is coarser."""
    if t == 0:
        return np.float32(0.0)
    a = abs(t)
    nb = a.bit_length()
    mant, sh = a, max(nb - 24, -149 - unit, 0)
    if sh > 0:
        mant = a >> sh
        rem, half = a & ((1 << sh) - 1), 1 << (sh - 1)
        if rem > half or (rem == half and (mant & 1)):
            mant += 1
    val = math.ldexp(mant, sh + unit) if sh + unit + mant.bit_length() <= 128 else math.inf  # (exact in float64 below 2^128)
    with np.errstate(over="ignore"):
        return np.float32(-val if t < 0 else val)


def exact_sum_f32(values):
    """The exact sum of fp32 values rounded once to fp32; non-finite members give what a float sum gives."""
    values = np.asarray(values, dtype=np.float32).ravel()
    fin = np.isfinite(values)
    if not fin.all():
        bad = values[~fin]
        if np.isnan(bad).any() or (np.isposinf(bad).any() and np.isneginf(bad).any()):
            return np.float32(np.nan)
        return np.float32(np.inf if np.isposinf(bad).any() else -np.inf)
    return int_to_f32(sum(f32_to_int(values.view(np.uint32))))


# ------------------------------------------------------------------ the exact fold's rule (gs_fixed128.hpp), restated
def _finite_max_bits(call_terms):
    """The float bits of the largest finite |x| of a call's terms (0 for none)."""
    u = np.asarray(call_terms, dtype=np.float32).ravel().view(np.uint32) & np.uint32(0x7FFFFFFF)
    u = u[u < 0x7F800000]
    return int(u.max()) if u.size else 0


def fold_rule_int(values, lg, call_terms=None):
    """The fold's 128-bit sum of finite fp32 `values` as a Python integer, and its scale -> (total, E): total 2^-E is the sum
    of the terms, each truncated toward zero to a multiple of 2^-E.  E = 252 - eb - lg with eb the biased exponent (at least 1)
    of the largest finite |x| of `call_terms` (the maximum itself, or all terms of the call; default: `values`)."""
    values = np.asarray(values, dtype=np.float32).ravel()
    assert np.isfinite(values).all()
    eb = max(_finite_max_bits(values if call_terms is None else call_terms) >> 23, 1)
    E = 252 - eb - int(lg)
    total = 0
    for b in values.view(np.uint32).tolist():
        e, m = (b >> 23) & 0xFF, b & 0x7FFFFF
        mant = (m | 0x800000) if e else m
        s = max(e, 1) - 150 + E  # x = mant 2^(s - E)
        u = mant << s if s >= 0 else mant >> -s
        total += -u if b >> 31 else u
    return total, E


def fold_rule_f32(values, lg, call_terms=None):
    """What the exact fold gives for one sum of fp32 `values` with at most 2^lg terms per sum: non-finite members give what
    exact_sum_f32 gives; otherwise every term is truncated toward zero to a multiple of 2^-E (fold_rule_int: E follows from the
    largest finite |x| of the whole CALL, `call_terms`), the integers are added exactly and the sum is rounded once to fp32,
    ties to even.  Equal to exact_sum_f32 while every term of the call lies within 102 - lg binary places of the largest."""
    values = np.asarray(values, dtype=np.float32).ravel()
    if not np.isfinite(values).all():
        return exact_sum_f32(values)
    total, E = fold_rule_int(values, lg, call_terms)
    return int_to_f32(total, unit=-E)
