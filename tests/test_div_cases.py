"""tests/div_cases.py holds what it says: the admission verdicts, the planted
operands' properties (conditions on the inputs, checked with the reference
arithmetic alone) and div_rcp(x, d) == x / d on every planted operand, in exact
arithmetic.  No GPU."""
import math

import numpy as np
import pytest

import div_cases as dc


def test_admission_verdicts():
    assert len(dc.ADMITTED) == 11 and len(dc.REFUSED) == 6
    for d in dc.ADMITTED:
        assert dc.admitted(d), d
    for d in dc.REFUSED:
        assert not dc.admitted(d), d
    # the window is [2^-40, 2^40): the frexp exponent of 2^40 is 41
    assert dc.admitted(2.0 ** -40) and not dc.admitted(2.0 ** 40) and dc.admitted(2.0 ** 40 - 2.0 ** 11)
    assert dc.admitted(1.5 * 2.0 ** 39) and dc.admitted(2.0 ** 39) and not dc.admitted(math.nextafter(2.0 ** -40, 0.0))
    # the odd part: 2^30 - 1 is the largest admitted, 2^30 + 1 the smallest refused
    assert dc.odd_part(dc.M30 * 2.0 ** -69) == 2 ** 30 - 1 and dc.odd_part(6.0) == 3 and dc.odd_part(2.0 ** -40) == 1
    for bad in (0.0, -0.0, math.inf, -math.inf, math.nan, 2.0 ** -1030, 5e-324):
        assert not dc.admitted(bad), bad
    assert dc.admitted(-3.0) and dc.admitted(-0.75)


def test_operand_range_rule():
    for x in (dc.X_LO, -dc.X_LO, 2.0 ** 959, math.nextafter(dc.X_HI, 0.0), 0.0, 1.0):
        assert dc.in_range(x), x
    for x in (-0.0, dc.X_HI, -dc.X_HI, math.nextafter(dc.X_LO, 0.0), math.inf, math.nan, 5e-324):
        assert not dc.in_range(x), x


@pytest.mark.parametrize("d", dc.ADMITTED, ids=[float(d).hex() for d in dc.ADMITTED])
def test_planted_operands_of_an_admitted_divisor(d):
    xs = dc.operands(d)
    assert xs.shape == (dc.N_ADMITTED,) and np.unique(xs).size >= dc.N_ADMITTED - 2
    assert xs[0] == 2.0 ** -960 and xs[1] == 2.0 ** 959
    assert all(dc.in_range(x) for x in xs) and not np.any(xs == 0.0)
    assert np.count_nonzero(xs < 0) >= 900 and np.count_nonzero(xs > 0) >= 900
    ex = np.frexp(np.abs(xs))[1] - 1  # floor(log2 |x|)
    assert np.count_nonzero(np.abs(ex) <= 8) >= 1024
    wide = ex[np.abs(ex) > 8]
    assert wide.min() == -960 and wide.max() == 959
    assert np.count_nonzero(wide < -480) >= 200 and np.count_nonzero(wide > 480) >= 200
    differ = sum(dc.product_differs(float(x), d) for x in xs)
    print(f"d = {d!r}: {differ} of {xs.size} operands have RN(x RN(1/d)) != RN(x / d)")
    assert differ >= dc.need_diff(d)
    assert dc.need_diff(d) == (0 if dc.is_pow2(d) else 32 if dc.odd_part(d) == 2 ** 30 - 1 else 512)
    if dc.is_pow2(d):
        assert differ == 0
    # the claim itself: the corrected reciprocal quotient is the division's, bit for bit
    bad = [float(x) for x in xs if dc.div_rcp(float(x), d) != float(x) / d]
    assert not bad, (d, bad[:5])


@pytest.mark.parametrize("d", dc.REFUSED, ids=[float(d).hex() for d in dc.REFUSED])
def test_planted_operands_of_a_refused_divisor(d):
    xs = dc.operands(d)
    assert xs.shape == (dc.N_REFUSED,) and xs[0] == 2.0 ** -960 and xs[1] == 2.0 ** 959
    assert all(dc.in_range(x) for x in xs)
    ex = np.frexp(np.abs(xs))[1] - 1
    assert np.count_nonzero(np.abs(ex) <= 8) >= 128 and np.count_nonzero(ex < -480) >= 20 and np.count_nonzero(ex > 480) >= 20


def test_refused_divisors_outside_the_window_break_the_reciprocal():
    """why the window is there: at 2^959 the reciprocal form overflows for 2^-100, and at the
    low end it lands in the subnormals for 3 * 2^100 (true quotients inf and subnormal)"""
    assert 2.0 ** 959 * (1.0 / 2.0 ** -100) == math.inf  # q0; then r = -inf and q1 = inf - inf
    d = 3.0 * 2.0 ** 100
    xs = dc.beyond_window(d)
    assert len(xs) == 4 and list(dc.operands(d)[2:6]) == xs
    for x in xs:
        assert dc.in_range(x) and 0.0 < abs(x / d) < 2.0 ** -1022 and dc.div_rcp(x, d) != x / d, x
    for d in dc.REFUSED:
        assert (len(dc.beyond_window(d)) == 4) == (d == 3.0 * 2.0 ** 100), d


def test_fallback_operands():
    for d in dc.ADMITTED:
        fb = dc.fallback(d)
        assert [dc.in_range(x) for x in fb[:6]] == [False, True, False, False, False, False]
        assert math.copysign(1.0, fb[0]) < 0 and fb[0] == 0.0 and fb[4] == 2.0 ** 960 and 0.0 < fb[5] < 2.0 ** -960
        t = dc.tiny(d)
        assert (t is None) == (d in dc.NO_TINY), (d, t)
        if t is not None:
            assert len(fb) == 7 and fb[6] == t and not dc.in_range(t)
            q = t / d
            assert q != 0.0 and abs(q) < 2.0 ** -1022, (d, t, q)
            assert dc.div_rcp(t, d) != q, (d, t)
    assert sum(dc.tiny(d) is not None for d in dc.ADMITTED) == 5  # 6, -6, 0.75, (2^30 - 1) 2^10, 1.5 2^39
    # what NO_TINY rests on: odd integers, a power of two, and a divisor whose every candidate was tried
    for d in dc.NO_TINY:
        m, e = dc.odd_exp(d)
        assert e == 0 or m == 1 or (d == dc.M30 * 2.0 ** -69 and math.frexp(d)[1] - 1022 + 1074 <= 14), d
