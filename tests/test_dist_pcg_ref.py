"""CPU: the rank-ordered dot product of the distributed PCG model (dist_pcg_ref.dist_dot)."""
import numpy as np
import pytest

import dist_pcg_ref
import pcg_ref


def bits(v):
    return np.float64(v).view(np.uint64)


@pytest.mark.parametrize("n", [1, 257, 2306, 5000])
def test_one_range_is_dev_dot(n):
    g = np.random.default_rng(n)
    x, y = g.uniform(-1, 1, n), g.uniform(-1, 1, n)
    assert bits(dist_pcg_ref.dist_dot([0, n])(x, y)) == bits(pcg_ref.dev_dot(x, y))


@pytest.mark.parametrize("n,cuts", [(2306, [2049]), (513, [1, 256]), (5000, [1200, 1200, 4999])])
def test_split_differs_by_a_few_ulps(n, cuts):
    """Positive data, so that the sum of |x_i y_i| is the result itself.  Either order adds every
    product through at most d rounded additions: a lane's chain (at most 8 at these sizes: 2048
    rows per workgroup), the 64-lane tree (6), the four waves (3), the same again over the
    workgroup partials (1 + 6 + 3), and one addition per rank (at most 4 here): d <= 31.  Each
    result is within d u sum|x_i y_i| of the exact sum (u = 2^-53, first order), the two within
    2 d u = 31 ulps of each other; an empty range adds 0.0 and changes nothing."""
    g = np.random.default_rng(n)
    x, y = g.uniform(0.5, 1, n), g.uniform(0.5, 1, n)
    one = pcg_ref.dev_dot(x, y)
    split = dist_pcg_ref.dist_dot([0] + cuts + [n])(x, y)
    ulps = abs(split - one) / np.spacing(one)
    print(f"n={n} cuts={cuts}: {ulps:.1f} ulps")
    assert ulps <= 31


@pytest.mark.parametrize("n,cuts", [(2306, [2049]), (513, [1, 256]), (5000, [1200, 1200, 4999])])
def test_split_is_exact_on_dyadic_data(n, cuts):
    """small integers: every product and every partial sum is exact in fp64, so the order cannot show"""
    g = np.random.default_rng(n + 1)
    x = g.integers(-8, 9, n).astype(np.float64)
    y = g.integers(-8, 9, n).astype(np.float64) / 4.0
    exact = float(np.sum(x * y))
    assert bits(pcg_ref.dev_dot(x, y)) == bits(exact)
    assert bits(dist_pcg_ref.dist_dot([0] + cuts + [n])(x, y)) == bits(exact)


def test_same_split_same_bits():
    """the sum depends on the values and the split only: not on the call, the container of the
    row starts, or the memory layout of the operands"""
    n = 3001
    g = np.random.default_rng(3)
    x, y = g.uniform(-1, 1, n), g.uniform(-1, 1, n)
    rs = [0, 700, 700, 2900, n]
    a = dist_pcg_ref.dist_dot(rs)(x, y)
    b = dist_pcg_ref.dist_dot(np.array(rs, dtype=np.int64))(x, y)
    wide = np.zeros((n, 2))
    wide[:, 0], wide[:, 1] = x, y
    c = dist_pcg_ref.dist_dot(tuple(rs))(wide[:, 0], wide[:, 1])  # strided views
    d = dist_pcg_ref.dist_dot(rs)(x, y)
    assert bits(a) == bits(b) == bits(c) == bits(d)
    # ... at a rounding-level distance from the one-range order
    assert np.isfinite(a) and abs(a - pcg_ref.dev_dot(x, y)) <= 64 * np.spacing(np.sum(np.abs(x * y)))
