"""The slab kernel's LDS capacity rule and the trimming estimate (csrc/host/fa_slab.h)
through libfa_host.so's exports: Python holds no copy of either, so the copies here
are the oracle -- the rule as ops/primitives.py used to write it out, and the exact
binomial tail in integer arithmetic."""
import itertools
from fractions import Fraction
from math import comb

import numpy as np
import pytest

LDS = 163328          # TUNING.slab_lds_bytes' default
K_RANGE = range(3, 42)
TOL = 1e-12           # per unit of histogram mass: <= 41 recurrence steps of a few ulp give ~1e-13


def _map_lds(F1):
    return ((F1 * 2 + 15) & ~15) if F1 <= 8192 else 0


def _rule(n_used, C, lds, accb):
    """(SW, capacity) as ops.primitives.slab_capacity / dl_slab_width computed it."""
    for sw in (16, 32, 8, 4):
        cap = int((lds - n_used * (sw + 2) * 8) // accb)
        if cap >= min(C, 8192) or (sw == 4 and cap >= 1024):
            return sw, cap
    return 0, 0


N_USED = (0, 1, 50, 300, 974, 2000, 3000, 5000, 20000)
CANDS = (1, 1000, 1023, 1024, 8191, 8192, 8193, 40000, 1 << 20)
BUDGETS = (24 << 10, 48 << 10, LDS, LDS - _map_lds(974), LDS - _map_lds(8192))


def test_slab_width_matches_the_restated_rule(native):
    from fastapriori_amd.ops import primitives as Pm
    seen = set()
    for n, C, lds, accb in itertools.product(N_USED, CANDS, BUDGETS, (2, 4)):
        got = Pm.slab_width(n, C, lds, accb)
        assert got == _rule(n, C, lds, accb), (n, C, lds, accb)
        seen.add(got[0])
    # every outcome the rule has.  32 is not among them: (sw + 2) * 8 grows with sw, so
    # width 32's capacity is below width 16's, which the order asks first -- the rule as
    # it stands (and as it stood in every copy) cannot return 32, on this grid or off it.
    assert seen == {16, 8, 4, 0}
    assert all(_rule(n, C, lds, accb)[0] != 32
               for n, C, lds, accb in itertools.product(range(0, 4000, 37), (1, 5000, 8192, 1 << 20),
                                                        BUDGETS, (2, 4)))


def test_slab_total_limit_is_the_largest_total_that_fits(native):
    from fastapriori_amd.ops import primitives as Pm
    for n, lds, accb in itertools.product(N_USED, BUDGETS, (2, 4)):
        t = Pm.slab_total_limit(n, lds, accb)
        assert 0 <= t <= _rule(n, t, lds, accb)[1], (n, lds, accb, t)
        assert t + 1 > _rule(n, t + 1, lds, accb)[1], (n, lds, accb, t)


def test_slab_map_lds(native):
    from fastapriori_amd.ops import primitives as Pm
    assert [Pm.slab_map_lds(F1) for F1 in (1, 8, 8192, 8193)] == [16, 16, 16384, 0]
    assert all(Pm.slab_map_lds(F1) == _map_lds(F1) for F1 in (1, 7, 8, 9, 974, 2000, 8191, 8192, 8193, 30000))


def test_slab_workgroups_matches_the_restated_footprint(native, tune):
    from fastapriori_amd.ops import primitives as Pm
    for budget in (LDS, 48 << 10, 100000):
        tune(slab_lds_bytes=budget)
        for nslabs, n, sw, nacc, rnd, mp in itertools.product((1, 3, 300, 5000), (1, 300, 974), (4, 8, 16, 32),
                                                               (1, 1001, 8192, 21352), (False, True), (0, 1952)):
            lds = n * (sw + 2) * 8 + (((nacc + 3) & ~3) if rnd else nacc) * 4 + mp
            want = max(1, min(nslabs, 256 * min(max(1, budget // lds), 2)))
            assert Pm._slab_workgroups(nslabs, n, sw, nacc, rnd, mp) == want


# ---- trimming estimate ---------------------------------------------------------------

P_GRID = [float(x) for x in (1e-6, 1e-4, 1e-3, 0.01, 0.05, 0.1, 0.25, 1 / 3, 0.5, 2 / 3, 0.75, 0.9, 0.99,
                             1 - 1e-6)]
L_MAX = 255


def _exact_tails(pf: float, L: int) -> list:
    """[P[Binom(L, p) >= k] for k in 0..41] at the double p's exact rational value."""
    p = Fraction(pf)
    a, b = p.numerator, p.denominator
    c, den = b - a, b ** L
    out, below, term = [], 0, (b - a) ** L          # term = C(L, k) a^k c^(L-k), an integer
    for k in range(42):
        # (den - below) / den, truncated at 2^-64 and rounded once to a double
        out.append(float(((den - below) << 64) // den) / 2.0 ** 64)
        below += term
        term = term * (L - k) * a // ((k + 1) * c)
    return out


def test_exact_tail_oracle():
    # the integer recurrence above against the definition, in rationals
    for pf, L in ((0.25, 7), (1 / 3, 40), (0.9, 45)):
        p = Fraction(pf)
        for k in (0, 3, 7, 41):
            want = sum(comb(L, i) * p ** i * (1 - p) ** (L - i) for i in range(k, L + 1))
            assert abs(_exact_tails(pf, L)[k] - float(want)) <= 2.0 ** -52


@pytest.fixture(scope="module")
def exact():
    """tails[(p, L)][k], computed once for the module."""
    return {(pf, L): _exact_tails(pf, L) for pf in P_GRID for L in range(3, L_MAX + 1)}


def _tail(Pm, hist, L, pf, k):
    hist[L] = 1
    rows, nnz = Pm.trim_estimate(hist, pf, k)
    hist[L] = 0
    assert nnz == L * pf
    return rows


def test_trim_estimate_against_the_exact_binomial_tail(native, exact):
    from fastapriori_amd.ops import primitives as Pm
    hist = np.zeros(L_MAX + 1, np.int64)
    worst = 0.0
    for pf in P_GRID:
        for k in K_RANGE:
            for L in range(3, L_MAX + 1):
                got = _tail(Pm, hist, L, pf, k)
                want = exact[pf, L][k] if L >= k else 0.0
                worst = max(worst, abs(got - want))
    print(f"largest |estimate - exact tail| = {worst:.3e}")
    assert worst <= TOL
    # a whole histogram: the sum of its bins' tails, and the occurrences kept
    rng = np.random.default_rng(5)
    hist = rng.integers(0, 1000, L_MAX + 1).astype(np.int64)
    for pf, k in ((0.1, 3), (0.5, 17), (0.9, 41)):
        rows, nnz = Pm.trim_estimate(hist, pf, k)
        want = sum(int(hist[L]) * exact[pf, L][k] for L in range(k, L_MAX + 1))
        assert abs(rows - want) <= TOL * int(hist.sum())
        assert nnz == pytest.approx(float((hist * np.arange(L_MAX + 1)).sum()) * pf, rel=1e-12)


def test_trim_estimate_against_betainc(native):
    betainc = pytest.importorskip("scipy.special").betainc
    from fastapriori_amd.ops import primitives as Pm
    hist = np.zeros(L_MAX + 1, np.int64)
    worst = 0.0
    for pf in P_GRID:
        for k in K_RANGE:
            L = np.arange(k, L_MAX + 1)
            want = betainc(k, L - k + 1, pf)
            got = np.array([_tail(Pm, hist, int(x), pf, k) for x in L])
            worst = max(worst, float(np.abs(got - want).max()))
    print(f"largest |estimate - betainc| = {worst:.3e}")
    assert worst <= TOL


def test_trim_estimate_histogram_sizes(native):
    from fastapriori_amd.ops import primitives as Pm
    assert Pm.trim_estimate(np.array([7], np.int64), 0.5, 3) == (0.0, 0.0)
    hist = np.zeros(300, np.int64)
    hist[[2, 40, 299]] = (5, 3, 2)
    rows, nnz = Pm.trim_estimate(hist, 0.25, 3)
    want = 3 * _exact_tails(0.25, 40)[3] + 2 * _exact_tails(0.25, 299)[3]
    assert abs(rows - want) <= TOL * 10
    assert nnz == pytest.approx((5 * 2 + 3 * 40 + 2 * 299) * 0.25, rel=1e-12)
    # edge probabilities: nothing survives at 0, every row of >= k items at 1
    assert Pm.trim_estimate(hist, 0.0, 3)[0] == 0.0
    assert Pm.trim_estimate(hist, 1.0, 3)[0] == 5.0
