"""Case table for the Jacobi epilogues' division by a uniform diagonal
(csrc/amg_kernels.hip: fast_div_of, div_rcp, div_rcp_ok, jac_div1, jac_div2).
Host arithmetic only: no GPU, no library.

The kernels replace x / d by q0 = x y, r = fma(-q0, d, x), q1 = fma(r, y, q0)
with y = RN(1 / d) when the host admits d (admitted below) and every lane of
the wave holds that divisor and an operand in range (in_range below).  This
module restates both rules and the arithmetic, and builds the operands that
can tell a right division from a wrong one:

  operands(d)   in range, x = RN(d (q + ulp(q) / 2)) for random 53-bit q, so
                that x / d lies next to a rounding midpoint.  Half have an
                exponent near 0, half are spread over [2^-960, 2^960) with the
                two boundary operands 2^-960 and 2^959 among them.  A share of
                them (NEED_DIFF) is searched so that the uncorrected product
                RN(x RN(1 / d)) is not the quotient: a kernel without the
                correction step, or with a wrong one, fails there.
  fallback(d)   operands out of range: -0.0, +0.0 (in range, listed beside its
                twin), inf, NaN, 2^960, the largest double below 2^-960 and
                tiny(d).  A wave that holds one of them must divide truly.
  tiny(d)       an operand whose quotient is subnormal and where
                div_rcp(x, d) != x / d, found by search.  The zeros, inf and
                NaN cannot show by themselves which division ran; this one can.

tiny(d) is None where no such operand exists (NO_TINY).  Every double is a
multiple of u = 2^-1074, and so is a subnormal quotient q0.  For an odd integer
d (3, 5, 7, 2^30 - 1) the remainder x - q0 d is then a whole multiple of u of
at most d / 2 units, hence exact, and the quotient lies j / d units off a grid
point, never within 1 / (2 d) of one half: far more than the error of r y, so
q1 is the correctly rounded quotient.  For a power of two the reciprocal only
scales.  For (2^30 - 1) 2^-69 only operands below 2^13 u have a subnormal
quotient: tiny() tries every one of them (the quotient is again a multiple of
1 / (2^30 - 1) units, and the reciprocal's relative error is 2^-60).  Every
other divisor of the table has one: an even d = m 2^e (e >= 1) has exact ties
x = d (k + 1/2) u, which the division rounds to even and the reciprocal to
wherever its error points; 0.75 loses the bits of r below u.
"""
import math
from fractions import Fraction
from functools import lru_cache

import numpy as np

X_LO, X_HI = 2.0 ** -960, 2.0 ** 960  # div_rcp_ok: |x| in [X_LO, X_HI), or +0.0


def _fma(a, b, c):
    """fma(a, b, c) in exact arithmetic, rounded once (int / int is correctly rounded)."""
    v = Fraction(a) * Fraction(b) + Fraction(c)
    return v.numerator / v.denominator if v else 0.0


def div_rcp(x, d):
    """csrc/amg_kernels.hip div_rcp: the quotient by the reciprocal with one correction step."""
    y = 1.0 / d
    q0 = x * y
    return _fma(_fma(-q0, d, x), y, q0)


def odd_exp(d):
    """(m, e) with |d| = m 2^e and m odd (d finite and not zero)"""
    f, e = math.frexp(abs(d))
    m, e = int(math.ldexp(f, 53)), e - 53
    while not m & 1:
        m, e = m >> 1, e + 1
    return m, e


def odd_part(d):
    """the odd part of d's 53-bit significand"""
    return odd_exp(d)[0]


def admitted(d):
    """fast_div_of's rule: d normal, its frexp exponent in [-39, 40] (2^-40 <= |d| < 2^40) and
    the odd part of its significand below 2^30."""
    d = float(d)
    if not math.isfinite(d) or abs(d) < 2.0 ** -1022:
        return False
    e = math.frexp(abs(d))[1]
    return -39 <= e <= 40 and odd_part(d) < 2 ** 30


def in_range(x):
    """div_rcp_ok: |x| in [2^-960, 2^960), or the bits of +0.0"""
    x = float(x)
    return X_LO <= abs(x) < X_HI or (x == 0.0 and math.copysign(1.0, x) > 0)


M30 = float(2 ** 30 - 1)
ADMITTED = [3.0, 5.0, 6.0, 7.0, -6.0, 0.75, M30, M30 * 2.0 ** -69, M30 * 2.0 ** 10, 2.0 ** -40, 1.5 * 2.0 ** 39]
REFUSED = [float(2 ** 30 + 1), 0.1, 2.0 ** -41, 2.0 ** 40, 3.0 * 2.0 ** 100, 2.0 ** -100]
N_ADMITTED, N_REFUSED = 2048, 256
NO_TINY = [3.0, 5.0, 7.0, M30, M30 * 2.0 ** -69, 2.0 ** -40]  # tiny(d) is None: the module docstring says why


def is_pow2(d):
    return odd_part(d) == 1


def need_diff(d):
    """NEED_DIFF: how many of operands(d) must have RN(x RN(1/d)) != RN(x / d)"""
    return 0 if is_pow2(d) else 32 if odd_part(d) == 2 ** 30 - 1 else 512


def product_differs(x, d):
    """the uncorrected product is not the quotient (both correctly rounded host operations)"""
    return x * (1.0 / d) != x / d


def _near_midpoint(g, d, ex):
    """x = RN(d (q + ulp(q) / 2)), q a random 53-bit significand scaled so that x's exponent is
    about ex: d = md 2^ed and q + ulp / 2 = (2 mq + 1) 2^k, the product an exact integer that
    float() rounds to nearest even and ldexp scales exactly"""
    fd, e = math.frexp(abs(d))
    md, ed = int(math.ldexp(fd, 53)), e - 53
    mq = int(g.integers(2 ** 52, 2 ** 53))
    x = float(md * (2 * mq + 1))
    return math.ldexp(x, ex - math.frexp(x)[1] + 1)


def _planted(d, seed, n, forced, edges):
    """n in-range operands for d: the edges, then near-midpoint operands, half with exponents
    in [-8, 8] and half over [-960, 959]; the first `forced` / 2 of each half are drawn until
    product_differs.  Signs alternate."""
    g = np.random.default_rng(seed)
    out = list(edges)
    half = n // 2
    for lo, hi, cnt in ((-8, 8, half), (-960, 959, n - half - len(edges))):
        for k in range(cnt):
            while True:
                x = _near_midpoint(g, d, int(g.integers(lo, hi + 1)))
                if not in_range(x):
                    continue
                if k >= forced // 2 or product_differs(x, d):
                    break
            out.append(-x if k & 1 else x)
    return np.array(out, dtype=np.float64)


def beyond_window(d):
    """For a divisor above the exponent window: four operands in range whose quotients are
    subnormal ties, x = d (k + 1/2) 2^-1074, and where div_rcp(x, d) is not the division's
    (ties to even there, here wherever the reciprocal's error points).  The window keeps the
    kernels from ever forming them; below it 2^959 does the same by overflowing x (1 / d)."""
    if math.frexp(abs(d))[1] <= 40 or is_pow2(d):  # a power of two only scales: nothing to find
        return []
    g = np.random.default_rng(3000 + REFUSED.index(d))
    m, ed = odd_exp(d)
    out = []
    while len(out) < 4:
        k = int(g.integers(2 ** 20, 2 ** 40))
        x = math.ldexp(float(m * (2 * k + 1)), ed - 1075)
        assert in_range(x) and x / d == math.ldexp(k + (k & 1), -1074), (x, k)
        if div_rcp(x, d) != x / d:
            out.append(x if len(out) & 1 else -x)
    return out


@lru_cache(maxsize=None)
def operands(d):
    """the planted in-range operands of a divisor: N_ADMITTED for an admitted one (with
    need_diff(d) of them searched), N_REFUSED for a refused one; 2^-960 and 2^959 first"""
    adm = d in ADMITTED
    assert adm or d in REFUSED
    idx = (ADMITTED + REFUSED).index(d)
    edges = [X_LO, 2.0 ** 959] + ([] if adm else beyond_window(d))
    out = _planted(d, 1000 + idx, N_ADMITTED if adm else N_REFUSED, need_diff(d) if adm else 0, edges)
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def tiny(d):
    """an operand whose quotient by d is subnormal and whose reciprocal-path quotient is not
    the division's, or None (see the module docstring) when the search finds none"""
    g = np.random.default_rng(2000 + ADMITTED.index(d))
    top = math.frexp(abs(d))[1] - 1022  # |x| < 2^top: the quotient is subnormal

    def hit(x):
        q = x / d
        return q != 0.0 and abs(q) < 2.0 ** -1022 and div_rcp(x, d) != q

    m, ed = odd_exp(d)
    if ed >= 1:
        # an even divisor has exact ties x = d (k + 1/2) 2^-1074: the division rounds them to
        # even, the reciprocal to wherever its error points, so every other k differs
        for _ in range(64):
            k = int(g.integers(1, min(2 ** 51, 2 ** 52 // m)))
            x = math.ldexp(float(m * (2 * k + 1)), ed - 1075)
            if hit(x):
                return x
    if top + 1074 <= 14:
        # a few thousand subnormal operands in all: every one, from the top, where the quotient
        # has the most bits (r rounds to 0 there, so only a wrong product can give a wrong q1)
        for X in range(2 ** (top + 1074) - 1, 0, -1):
            x = math.ldexp(float(X), -1074)
            if product_differs(x, d) and hit(x):
                return x
        return None
    for _ in range(3000):
        ex = top - int(g.integers(1, 12))
        if ex >= -1022:
            x = math.ldexp(1.0 + float(g.integers(0, 2 ** 52)) * 2.0 ** -52, ex)
        else:  # a subnormal operand with as many bits as fit
            x = math.ldexp(float(g.integers(2 ** (ex + 1074), 2 ** (ex + 1075))), -1074)
        if hit(x):
            return x
    return None


def fallback(d):
    """the operands that must send a wave to the division itself (and +0.0 beside -0.0);
    d None or refused: without a tiny operand"""
    out = [-0.0, 0.0, math.inf, math.nan, X_HI, math.nextafter(X_LO, 0.0)]
    if d in ADMITTED and tiny(d) is not None:
        out.append(tiny(d))
    return out
