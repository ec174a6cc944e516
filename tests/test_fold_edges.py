"""The exact 128-bit fold (gs_fixed128.hpp) at its edges, through gs_voxel_reduce.

The rule is restated once in tests/helpers.py (fold_rule_f32, Python integers): the call's largest finite |x| fixes the scale
E = 252 - eb - lg, every term is truncated toward zero to a multiple of 2^-E, the integers are added exactly and the sum is
rounded once to fp32.  ops.voxel_reduce_raw takes the assignment as an input, so a hand-made voxel_of puts any multiset of fp32
values into any sum: every case below builds its own sums, says which edge it is (and asserts that it is that edge), and
compares bit for bit with the rule, in both modes (with and without the pre-aggregation of neighbouring lanes).
"""
import numpy as np
import pytest
import torch

from tests.helpers import exact_sum_f32, fold_rule_f32, fold_rule_int, int_to_f32

DEV = "cuda:0"
FLT_MAX = np.array([0x7F7FFFFF], np.uint32).view(np.float32)[0]


def f32(*xs):
    return np.array(xs, dtype=np.float32)


def from_bits(*bs):
    return np.array(bs, dtype=np.uint32).view(np.float32)


def bits_of(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def lg_of(n):
    return int(n - 1).bit_length()  # ceil(log2 n), n >= 1


# ------------------------------------------------------------------ CPU: the rule itself
def test_rule_equals_the_exact_sum_within_its_range():
    """Spread within 102 - lg binary places of the largest term: nothing is truncated, the rule is the exact sum."""
    rng = np.random.RandomState(0)
    for lg in (0, 3, 12):
        span = 102 - lg - 24  # exponents: the lowest mantissa bit of the smallest term is still carried
        for _ in range(20):
            n = rng.randint(1, min(1 << lg, 40) + 1)
            x = (rng.choice([-1.0, 1.0], n) * (1.0 + rng.rand(n)) * np.exp2(rng.randint(-span, 1, n) + rng.randint(-40, 40))).astype(np.float32)
            assert fold_rule_f32(x, lg).view(np.uint32) == exact_sum_f32(x).view(np.uint32), (lg, x)
    sub = from_bits(1, 1, 3, 0x7FFFFF, 0x80000002)  # subnormals only: eb clamps to 1
    assert fold_rule_int(sub, 4)[1] == 251 - 4
    assert fold_rule_f32(sub, 4).view(np.uint32) == exact_sum_f32(sub).view(np.uint32) == 0x800002
    top = from_bits(0x7F7FFFFF, 0xFF7FFFFF, 0x7F000001, 0x7F7FFFFE)  # top binade
    assert fold_rule_int(top, 2)[1] == -2 - 2
    assert fold_rule_f32(top, 2).view(np.uint32) == exact_sum_f32(top).view(np.uint32)
    assert fold_rule_f32(f32(), 3) == 0 and fold_rule_f32(f32(-0.0, -0.0), 3).view(np.uint32) == 0
    assert np.isnan(fold_rule_f32(f32(1.0, np.nan), 3)) and np.isnan(fold_rule_f32(f32(np.inf, -np.inf), 3))
    assert fold_rule_f32(f32(1.0, -np.inf), 3) == -np.inf


def test_rule_truncates_toward_zero_below_the_call_global_unit():
    lg = 5
    M = f32(2.0 ** 100)
    E = fold_rule_int(M, lg)[1]
    assert E == 252 - 227 - lg == 20
    small = f32(*[(2 ** 23 + 1) * 2.0 ** (-E - 35)] * 4)  # each wholly below the unit 2^-E
    assert fold_rule_f32(small, lg, M) == 0 and exact_sum_f32(small) == np.float32((2 ** 23 + 1) * 2.0 ** (-E - 33))
    assert fold_rule_f32(small, lg) == exact_sum_f32(small)  # on their own they are carried in full
    x = f32(1.0 + 7 * 2.0 ** -23)  # three bits below the unit 2^-20
    assert fold_rule_f32(x, lg, M) == np.float32(1.0) and fold_rule_f32(-x, lg, M) == np.float32(-1.0)  # toward zero, not floor
    assert fold_rule_f32(np.concatenate([x, x]), lg, np.concatenate([M, x])) == np.float32(2.0)  # (all the call's terms)


def test_rule_rounds_once_ties_to_even_and_out_of_range():
    r = lambda *xs: fold_rule_f32(f32(*xs), 4)
    assert r(2.0 ** 24, 1.0) == np.float32(2.0 ** 24)
    assert r(2.0 ** 24, 2.0, 1.0) == np.float32(2.0 ** 24 + 4)
    assert r(2.0 ** 25 - 2, 1.0) == np.float32(2.0 ** 25)
    assert r(2.0 ** 24, 1.0, 2.0 ** -36) == np.float32(2.0 ** 24 + 2)  # a tie broken from 60 places below
    assert r(FLT_MAX, 2.0 ** 103) == np.inf and r(FLT_MAX, 2.0 ** 102) == FLT_MAX  # the tie rounds up out of range
    assert r(-FLT_MAX, -2.0 ** 103) == -np.inf
    assert r(FLT_MAX, FLT_MAX, -FLT_MAX) == FLT_MAX and r(FLT_MAX, FLT_MAX) == np.inf
    # int_to_f32 in other units, subnormal results included: 3 2^-150 is a tie -> 2 2^-149; 5 2^-151 is above 2^-149
    assert int_to_f32(3, unit=-150).view(np.uint32) == 2 and int_to_f32(5, unit=-151).view(np.uint32) == 1
    assert int_to_f32(-(2 ** 24 + 1) << 100, unit=-249).view(np.uint32) == np.float32(-(2.0 ** -125)).view(np.uint32)


# ------------------------------------------------------------------ GPU helpers
class Call:
    """One gs_voxel_reduce call of hand-made sums: x (B, N, C) fp32, voxel_of (B, N), n_voxels (B,), counts (B,)."""

    def __init__(self, x, voxel_of, n_voxels=None, counts=None):
        self.x = np.ascontiguousarray(x, dtype=np.float32)
        self.B, self.N, self.C = self.x.shape
        self.vof = np.ascontiguousarray(voxel_of, dtype=np.int32).reshape(self.B, self.N)
        self.nvox = np.asarray([int(v.max()) + 1 for v in self.vof] if n_voxels is None else n_voxels, dtype=np.int32)
        self.counts = np.asarray([self.N] * self.B if counts is None else counts, dtype=np.int32)
        self.M = max(int(self.nvox.max()), 1)
        self.lg = lg_of(self.N)
        assert self.N <= 4097 and self.M <= 600

    def members(self, b, m):
        i = np.arange(self.N)
        return (i < self.counts[b]) & (self.vof[b] == m) & (m < self.nvox[b])

    def call_terms(self):
        """Every term that belongs to a sum of the call: the maximum is taken over these (non-finite ones never count)."""
        keep = np.stack([(np.arange(self.N) < self.counts[b]) & (self.vof[b] >= 0) & (self.vof[b] < self.nvox[b]) for b in range(self.B)])
        return self.x[keep]

    def voxel_count(self):
        cnt = np.zeros((self.B, self.N), np.int32)
        for b in range(self.B):
            for m in range(int(self.nvox[b])):
                cnt[b, m] = self.members(b, m).sum()
        return cnt

    def rule(self, mean=False, fn=None):
        """(B, M, C) by fold_rule_f32 (or fn(values) per sum); rows beyond n_voxels are zero."""
        terms = self.call_terms()
        mx = np.abs(terms[np.isfinite(terms)]).max(initial=0.0)
        out = np.zeros((self.B, self.M, self.C), np.float32)
        cnt = self.voxel_count()
        for b in range(self.B):
            for m in range(int(self.nvox[b])):
                rows = self.x[b, self.members(b, m)]
                for c in range(self.C):
                    out[b, m, c] = fold_rule_f32(rows[:, c], self.lg, mx) if fn is None else fn(rows[:, c])
                if mean:
                    with np.errstate(all="ignore"):
                        out[b, m] = out[b, m] / np.float32(cnt[b, m])
        return out

    def gpu(self, mean=False):
        """The device's result, the same bits required of both modes -> (B, M, C) float32."""
        from gradslam_amd import ops

        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        args = (t(self.x), t(self.counts), t(self.vof), t(self.nvox), t(self.voxel_count()), self.M)
        got = [ops.voxel_reduce_raw(*args, (1 if mean else 0) | mode).cpu().numpy() for mode in (0, ops.VOXEL_NO_PREAGG)]
        assert np.array_equal(bits_of(got[0]), bits_of(got[1])), "pre-aggregated and plain accumulation differ"
        return got[0]

    def check(self, mean=False):
        got, want = self.gpu(mean), self.rule(mean)
        bad = np.argwhere((bits_of(got) != bits_of(want)) & ~(np.isnan(got) & np.isnan(want)))  # (NaN compares as NaN)
        assert bad.size == 0, [(tuple(i), hex(bits_of(got)[tuple(i)]), hex(bits_of(want)[tuple(i)])) for i in bad[:8]]
        return got


def sums_call(sums, N=None, C=1):
    """One batch element, one channel: voxel m holds the values sums[m] (adjacent rows); N pads with rows beyond the count."""
    vals = np.concatenate([np.asarray(s, np.float32) for s in sums])
    vof = np.concatenate([np.full(len(s), m, np.int32) for m, s in enumerate(sums)])
    n = len(vals)
    N = n if N is None else N
    x = np.zeros((1, N, 1), np.float32)
    x[0, :n, 0] = vals
    v = np.full((1, N), -1, np.int32)
    v[0, :n] = vof
    return Call(x, v, n_voxels=[len(sums)], counts=[n])


def full_mantissa(rng, lo, hi, exp):
    """A random fp32 in [lo, hi) 2^exp (lo, hi within one binade) whose last mantissa bit is set."""
    v = np.float32(rng.uniform(lo, hi) * 2.0 ** int(exp))
    return from_bits(int(v.view(np.uint32)) | 1)[0]


# ------------------------------------------------------------------ GPU 1: the sums' leading bit at every accumulator position
@pytest.mark.gpu
def test_leading_bit_sweep_over_every_accumulator_position():
    """Voxel 0 holds 1.0 (M = 1, E = 125 - lg = 115 for N = 1024); then one voxel per sign and leading-bit position p = 0 .. E
    of three full-mantissa terms of both signs: the p <= 23 branch, the seam between the accumulator's words at bits 63 / 64,
    rounding positions on either side of it, and for small p terms that are partly or wholly truncated."""
    rng = np.random.RandomState(3)
    N, lg = 1024, 10
    E = 125 - lg
    sums = [f32(1.0)]
    for p in range(E + 1):
        k = p - E
        if p <= E - 2:
            terms = [full_mantissa(rng, 1.5, 1.75, k), -full_mantissa(rng, 0.25, 0.5, k), full_mantissa(rng, 1.0, 2.0, k - 24)]
        else:  # every term stays below M = 1
            terms = [full_mantissa(rng, 0.75, 1.0, k), full_mantissa(rng, 0.5, 0.75, k), -full_mantissa(rng, 0.125, 0.25, k)]
        sums += [f32(*terms), -f32(*terms)]
    call = sums_call(sums, N=N)
    assert call.lg == lg and fold_rule_int(call.call_terms(), lg)[1] == E and np.abs(call.call_terms()).max() == 1.0
    lead = {1: set(), -1: set()}
    truncated = 0
    for s in sums[1:]:
        total = fold_rule_int(s, lg, f32(1.0))[0]
        lead[1 if total > 0 else -1].add(abs(total).bit_length() - 1)
        truncated += fold_rule_f32(s, lg, f32(1.0)).view(np.uint32) != exact_sum_f32(s).view(np.uint32)
    for sign in (1, -1):  # both sides of 23 and of 63 / 64 among them
        assert lead[sign] >= set(range(E + 1)), sorted(set(range(E + 1)) - lead[sign])
    assert {22, 23, 24, 62, 63, 64, 65, 86, 87, 88} <= lead[1] and truncated >= 10
    got = call.check()
    assert np.isfinite(got).all() and (got[0, 1:len(sums), 0] != 0).all()


# ------------------------------------------------------------------ GPU 2: the final rounding
@pytest.mark.gpu
def test_final_rounding_ties_carry_and_zero():
    cases = [  # (members, expected sum)
        ((2.0 ** 24, 1.0), 2.0 ** 24),                           # tie, kept mantissa even: down
        ((2.0 ** 24, 2.0, 1.0), 2.0 ** 24 + 4),                  # tie, kept mantissa odd: up
        ((2.0 ** 24, 1.0, 2.0 ** -36), 2.0 ** 24 + 2),           # the tie broken upward by a term 60 binary places below
        ((2.0 ** 24, 2.0, 1.0, -(2.0 ** -36)), 2.0 ** 24 + 2),   # and downward
        ((2.0 ** 25 - 2, 1.0), 2.0 ** 25),                       # the mantissa carries to 2^24
        ((2.0 ** 24 - 1, 0.5), 2.0 ** 24),                       # tie at the top of a binade, odd: carries
        ((2.0 ** 24 - 2, 0.5), 2.0 ** 24 - 2),                   # the same tie, even: stays
    ]
    sums, want = [], []
    for members, w in cases:
        for sign in (1.0, -1.0):
            sums.append(sign * f32(*members))
            want.append(sign * w)
    sums += [f32(3.25, -3.25, 1e-3, -1e-3, 2.0 ** 24, -(2.0 ** 24)), f32(-0.0, -0.0, -0.0)]  # cancellation; -0 members only
    want += [0.0, 0.0]
    call = sums_call(sums)
    for s, w in zip(sums, want):  # the cases are the edges they claim to be, by the test's own exact sum
        assert exact_sum_f32(s).view(np.uint32) == np.float32(w).view(np.uint32), (s, w)
    got = call.check()[0, :, 0]
    assert np.array_equal(bits_of(got), bits_of(f32(*want)))
    assert bits_of(got)[-2] == 0 and bits_of(got)[-1] == 0  # +0.0 both


# ------------------------------------------------------------------ GPU 3: subnormals
@pytest.mark.gpu
def test_subnormal_members_and_results():
    """Every member of the call is subnormal: eb clamps to 1, E = 251 - lg."""
    sums = [from_bits(1, 1, 3),                              # stays subnormal: 5 2^-149
            from_bits(0x7FFFFF, 0x80000001),                 # mixed signs, stays subnormal
            from_bits(0x7FFFFF, 1),                          # crosses into the normal range: 2^-126
            from_bits(0x7FFFFF, 0x7FFFFF, 0x7FFFFF, 0x7FFFFF, 0x7FFFFF),  # a normal result that needs no rounding
            from_bits(*([0x7FFFFF] * 9)),                    # 9 (2^23 - 1): 27 bits, rounded
            from_bits(0x807FFFFF, 0x807FFFFF, 0x80000003),   # negative, normal
            from_bits(0x123456, 0x80123456, 7, 0x80000007),  # cancels to zero
            from_bits(0, 0x80000000)]
    want = [5, 0x7FFFFE, 0x800000, None, None, None, 0, 0]
    call = sums_call(sums)
    assert (bits_of(call.call_terms()) & 0x7F800000).max() == 0 and fold_rule_int(call.call_terms(), call.lg)[1] == 251 - call.lg
    got = call.check()[0, :, 0]
    for g, s, w in zip(bits_of(got), sums, want):
        assert g == exact_sum_f32(s).view(np.uint32) and (w is None or g == w), (s, hex(g))
    assert (bits_of(got)[:2] < 0x800000).all() and (bits_of(got)[2:6] & 0x7F800000 != 0).all()


@pytest.mark.gpu
def test_a_call_of_zeros_only():
    x = np.zeros((1, 70, 2), np.float32)
    x[0, ::3, 1] = -0.0
    call = Call(x, (np.arange(70) % 7)[None])
    assert fold_rule_int(call.call_terms(), call.lg)[1] == 251 - call.lg  # M = 0
    assert not bits_of(call.check()).any() and not bits_of(call.check(mean=True)).any()


# ------------------------------------------------------------------ GPU 4: the top binade
@pytest.mark.gpu
def test_top_binade_members_and_sums_out_of_range():
    mx = FLT_MAX
    sums = [f32(mx, mx), f32(-mx, -mx), f32(mx, mx, -mx), f32(-mx, -mx, mx), f32(mx, 2.0 ** 103), f32(mx, 2.0 ** 102),
            f32(-mx, -(2.0 ** 103)), f32(mx, -mx), f32(mx)]
    want = f32(np.inf, -np.inf, mx, -mx, np.inf, mx, -np.inf, 0.0, mx)  # infinities by rounding: no flag is set for them
    call = sums_call(sums)
    assert fold_rule_int(call.call_terms(), call.lg)[1] == -2 - call.lg
    got = call.check()[0, :, 0]
    assert np.array_equal(bits_of(got), bits_of(want))


@pytest.mark.gpu
@pytest.mark.parametrize("N", [4096, 4097])
def test_one_voxel_of_n_same_sign_members_at_the_bound(N):
    """N members just below 2 in ONE voxel (lg = 12 and 13): the sum is just below 2^(lg + 1), in the accumulator just below
    2^126 -- the stated bound.  Channels 0 and 1 hold them with either sign (all in the high word); channels 2 and 3 hold
    same-sign members whose leading bit sits at accumulator bits 61 .. 63, so nearly every add wraps the low word."""
    rng = np.random.RandomState(N)
    lg = 12 if N == 4096 else 13
    x = from_bits(*(0x3FFFFFFF - rng.randint(0, 4, N)).tolist())
    low = np.array([full_mantissa(rng, 1.0, 2.0, e - (102 - lg)) for e in rng.randint(38, 41, N)], np.float32)
    call = Call(np.stack([x, -x, low, -low], axis=1)[None], np.zeros((1, N), np.int32))
    assert call.lg == lg
    total, E = fold_rule_int(x, lg, call.call_terms())
    assert E == 125 - lg and 2 ** 125 <= total < 2 ** 126
    total_low = fold_rule_int(low, lg, call.call_terms())[0]
    assert total_low >= 2 ** 72 and max(fold_rule_int(low[i:i + 1], lg, call.call_terms())[0] for i in range(N)) < 2 ** 64
    got = call.check()
    assert np.isfinite(got).all() and got[0, 0, 0] == -got[0, 0, 1] and got[0, 0, 2] == -got[0, 0, 3]
    assert np.array_equal(bits_of(got), bits_of(call.rule(fn=exact_sum_f32)))


# ------------------------------------------------------------------ GPU 5: truncation and the call-global maximum
def _truncation_sums(rng, E):
    """Sums whose terms carry bits below 2^-E (the unit of a call whose maximum is 2^100), of both signs."""
    unit = -E
    sums = [f32(*[(2 ** 23 + 1) * 2.0 ** (unit - 35)] * 4),                # wholly below the unit: vanish
            f32(*[-(2 ** 23 + 1) * 2.0 ** (unit - 35)] * 4),
            f32((1 + 7 * 2.0 ** -23) * 2.0 ** (unit + 20)),                  # one term, its last three bits below the unit
            f32(-(1 + 7 * 2.0 ** -23) * 2.0 ** (unit + 20)),                 # toward zero, where floor would give one unit more
            f32(*[-(1 + 2.0 ** -23) * 2.0 ** (unit + 22)] * 3)]
    for _ in range(6):
        sums.append(f32(*[s * full_mantissa(rng, 1.0, 2.0, unit + e) for s, e in zip(rng.choice([-1.0, 1.0], 5), rng.randint(-3, 23, 5))]))
    return sums


def _assert_truncation_shows(call, lg, M):
    """At least one sum differs from its exact sum, and at least one from the sum of floors (truncation is toward zero)."""
    n_exact = n_floor = 0
    for b in range(call.B):
        for m in range(int(call.nvox[b])):
            for c in range(call.C):
                v = call.x[b, call.members(b, m), c]
                r = fold_rule_f32(v, lg, M).view(np.uint32)
                n_exact += r != exact_sum_f32(v).view(np.uint32)
                E = fold_rule_int(v, lg, M)[1]
                floor_total = sum(int(np.floor(np.float64(t) * 2.0 ** E)) for t in v)  # (exact in float64: 24 bits times 2^E)
                n_floor += r != int_to_f32(floor_total, unit=-E).view(np.uint32)
    assert n_exact >= 3 and n_floor >= 1, (n_exact, n_floor)


@pytest.mark.gpu
def test_truncation_below_the_unit_of_the_call():
    """M = 2^100 in one voxel: with N = 62, E = 252 - 227 - 6 = 19, and every other sum loses what lies below 2^-19."""
    N, lg, E = 62, 6, 19
    sums = [f32(2.0 ** 100)] + _truncation_sums(np.random.RandomState(1), E)
    call = sums_call(sums, N=N)
    assert call.lg == lg and fold_rule_int(call.call_terms(), lg)[1] == E
    _assert_truncation_shows(call, lg, f32(2.0 ** 100))
    got = call.check()[0, :, 0]
    assert got[0] == np.float32(2.0 ** 100) and got[1] == 0 and got[2] == 0 and bits_of(got)[2] == 0
    assert got[3] == np.float32(2.0 ** (-E + 20)) and got[4] == -got[3]  # toward zero for both signs
    # the same small sums in a call of their own are exact
    alone = sums_call(sums[1:], N=N)
    assert np.array_equal(bits_of(alone.check()), bits_of(alone.rule(fn=exact_sum_f32)))


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["batch", "channel"])
def test_the_maximum_is_taken_over_the_whole_call(where):
    """The large value sits in batch element 0 (B = 2) or in channel 0 (C = 2), the small data in the other: truncated alike."""
    N, lg, E = 64, 6, 19
    small = sums_call(_truncation_sums(np.random.RandomState(2), E), N=N)
    r = int(small.counts[0])  # the first row the small data leaves free
    big = np.zeros((1, N, 1), np.float32)
    big[0, r, 0] = -(2.0 ** 100)
    if where == "batch":
        call = Call(np.concatenate([big, small.x]), np.concatenate([np.where(np.arange(N) == r, 0, -1)[None], small.vof]),
                    n_voxels=[1, small.nvox[0]], counts=[N, r])
    else:
        vof = small.vof.copy()
        vof[0, r] = 0
        call = Call(np.concatenate([big, small.x], axis=2), vof, n_voxels=small.nvox, counts=[r + 1])
    assert r < N and fold_rule_int(call.call_terms(), lg)[1] == E
    _assert_truncation_shows(call, lg, f32(2.0 ** 100))
    call.check()


@pytest.mark.gpu
def test_rows_that_stay_out_of_the_maximum():
    """A NaN and an inf member, a row at and one beyond counts[b], a row with voxel_of = -1 and one with voxel_of >= n_voxels,
    the last four holding 3e38: none of them may enter M.  The sums are of full-mantissa values near 1 and near 2^-60: had
    any of these rows entered M, the small terms (with 3e38: every term) would be truncated away."""
    rng = np.random.RandomState(5)
    N, C, n, nvox = 96, 2, 90, 6
    x = np.array([[s * full_mantissa(rng, 1.0, 2.0, e) for s, e in zip(rng.choice([-1.0, 1.0], C), rng.choice([0, -60], C))]
                  for _ in range(N)], np.float32)[None]
    vof = (np.arange(N) % nvox).astype(np.int32)[None]
    out_rows = {"at_count": n, "beyond_count": n + 3, "no_voxel": 17, "voxel_beyond_n": 40}
    vof[0, out_rows["no_voxel"]], vof[0, out_rows["voxel_beyond_n"]] = -1, nvox
    for r in out_rows.values():
        x[0, r] = 3e38
    x[0, 8, 0], x[0, 21, 1] = np.nan, -np.inf  # members of voxels 2 and 3
    call = Call(x, vof, n_voxels=[nvox], counts=[n])
    assert np.abs(call.call_terms()[np.isfinite(call.call_terms())]).max() < 2.0
    assert fold_rule_int(call.call_terms()[np.isfinite(call.call_terms())], call.lg)[1] == 125 - call.lg
    got = call.check()
    flagged = np.zeros((1, nvox, C), bool)
    flagged[0, 2, 0] = flagged[0, 3, 1] = True
    assert np.isnan(got[0, 2, 0]) and got[0, 3, 1] == -np.inf and np.isfinite(got[~flagged]).all()
    assert np.array_equal(bits_of(got[~flagged]), bits_of(call.rule(fn=exact_sum_f32)[~flagged]))  # nothing was truncated
    zeroed = x.copy()
    for r in out_rows.values():
        zeroed[0, r] = 0.0
    zeroed[0, 8, 0] = zeroed[0, 21, 1] = 0.0
    ref = Call(zeroed, vof, n_voxels=[nvox], counts=[n]).check()
    assert np.isfinite(ref).all() and np.array_equal(bits_of(got[~flagged]), bits_of(ref[~flagged]))


# ------------------------------------------------------------------ GPU 6: the flag words
FLAG_CHANNELS = (0, 9, 10, 19, 20, 29, 30, 63)
FLAG_KINDS = ((np.nan,), (np.inf,), (-np.inf,), (np.inf, -np.inf))


def _flag_call(C):
    rng = np.random.RandomState(C)
    nvox, per = 12, 6
    N = nvox * per
    x = (rng.choice([-1.0, 1.0], (1, N, C)) * (1.0 + rng.rand(1, N, C)) * np.exp2(rng.randint(-30, 1, (1, N, C)))).astype(np.float32)
    vof = rng.permutation(np.arange(N) % nvox).astype(np.int32)[None]
    rows = lambda m: np.nonzero(vof[0] == m)[0]
    flagged = {}
    for k, ch in enumerate(c for c in FLAG_CHANNELS if c < C):  # one kind per (voxel k, channel ch), the kinds in turn
        for r, val in zip(rows(k), FLAG_KINDS[k % 4]):
            x[0, r, ch] = val
        flagged[(k, ch)] = FLAG_KINDS[k % 4]
    pairs = [p for p in ((8, 9), (9, 10), (19, 20), (39, 40), (49, 50), (59, 60), (62, 63)) if p[1] < C]
    for k, (c0, c1) in enumerate(pairs):  # two different flags in neighbouring channels of one voxel
        m = 8 + k % 4
        kinds = (FLAG_KINDS[(k + 1) % 4], FLAG_KINDS[(k + 2) % 4])
        for ch, kind in zip((c0, c1), kinds):
            for r, val in zip(rows(m)[2 * (ch == c1):], kind):
                x[0, r, ch] = val
            flagged[(m, ch)] = kind
    return Call(x, vof), flagged


@pytest.mark.gpu
@pytest.mark.parametrize("C,mean", [(10, False), (11, False), (21, False), (21, True), (64, False)])
def test_flags_in_every_flag_word(C, mean):
    """Ten channels share a flag word (3 bits each): NaN, +inf, -inf and both infinities in the first and last channel of
    every word, different flags in neighbours within a word (8, 9) and across a word boundary (9, 10; 19, 20; 59, 60); every
    other sum keeps its finite bits.  mean: the division comes after the flag rule."""
    call, flagged = _flag_call(C)
    words = -(-C // 10)
    assert words == {10: 1, 11: 2, 21: 3, 64: 7}[C] and (C == 10 or words > 1)
    assert {ch // 10 for _, ch in flagged} == set(range(words))  # every flag word of a row is used
    got = call.check(mean)
    isflag = np.zeros(got.shape, bool)
    for (m, ch), kind in flagged.items():
        isflag[0, m, ch] = True
        if len(kind) == 2 or np.isnan(kind[0]):
            assert np.isnan(got[0, m, ch]), (m, ch, kind, got[0, m, ch])
        else:
            assert got[0, m, ch] == kind[0], (m, ch, kind, got[0, m, ch])
    assert np.isfinite(got[~isflag]).all() and (got[~isflag] != 0).all()
    want = call.rule(mean, fn=exact_sum_f32)  # the finite sums are within range: exact
    assert np.array_equal(bits_of(got[~isflag]), bits_of(want[~isflag]))


# ------------------------------------------------------------------ GPU 7: pre-aggregated runs
@pytest.mark.gpu
def test_preaggregated_runs_across_waves_and_blocks():
    """Members of one voxel adjacent in runs of 1, 2, 63, 64, 65 and 130 lanes, the runs crossing wave boundaries and the
    256-thread block; channel 0 holds same-sign members near the maximum, so the segmented shuffle sum wraps its low word
    inside the wave.  The same bits with and without pre-aggregation (Call.gpu) and as the rule."""
    runs = [1, 2, 63, 64, 65, 130, 2, 130, 65, 1, 64, 63, 130, 1, 1, 2, 64, 65, 63]
    nvox = 5
    vof = np.concatenate([np.full(r, k % nvox, np.int32) for k, r in enumerate(runs)])
    N = len(vof)
    starts = np.cumsum([0] + runs[:-1])
    crosses = lambda period: any(s // period != (s + r - 1) // period for s, r in zip(starts, runs) if r > 1)
    assert N <= 4097 and N > 3 * 256 and crosses(64) and crosses(256)
    rng = np.random.RandomState(11)
    lg = lg_of(N)
    s = 102 - lg  # the shift of a term of [1, 2) in a call whose maximum lies there
    low = np.array([full_mantissa(rng, 1.0, 2.0, e - s) for e in rng.randint(38, 41, N)])  # leading bit at 61 .. 63: two wrap
    x = np.stack([low, -low, np.array([full_mantissa(rng, 1.0, 2.0, 0) for _ in range(N)]),
                  rng.choice([-1.0, 1.0], N) * np.array([full_mantissa(rng, 1.0, 2.0, e) for e in rng.randint(-60, 1, N)])], axis=1)
    call = Call(x.astype(np.float32)[None], vof[None])
    assert call.lg == lg and fold_rule_int(call.call_terms(), lg)[1] == 125 - lg
    assert all(2 ** 61 <= fold_rule_int(low[i:i + 1], lg, call.call_terms())[0] < 2 ** 64 for i in range(N))
    got = call.check()
    assert np.array_equal(bits_of(got), bits_of(call.rule(fn=exact_sum_f32)))
