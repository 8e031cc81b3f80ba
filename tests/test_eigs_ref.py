"""CPU: the host parts of the CG-Lanczos eigenvalue estimate -- amg_lanczos_extremes and
amg_lehmer_stream -- against their Python restatements (tests/eigs_ref.py), numpy and the dense
spectrum.  No GPU: the alpha / beta histories come from the host model of the recurrence.
"""
import ctypes as C

import numpy as np
import pytest

import eigs_ref

EPS = np.finfo(np.float64).eps
ITERS = 20

_cache = {}


def case(oracle, n, scaled):
    """(A, alpha, beta, gamma) of the model on the n^3 7-pt operator, plain or S A S, built once"""
    key = (n, scaled)
    if key not in _cache:
        A = oracle.laplace_7pt(n)
        if scaled:
            A = eigs_ref.sym_scaled(oracle, A)
        _cache[key] = (A,) + eigs_ref.eigs_model(oracle, A, ITERS)
    return _cache[key]


CASES = [(6, False), (6, True), (8, False), (8, True)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_bitwise(amg, alpha, beta):
    emax, emin, td, to = amg.lanczos_extremes(alpha, beta, full=True)
    rmax, rmin, rtd, rto = eigs_ref.lanczos_extremes(alpha, beta)
    assert np.array_equal(bits(td), bits(rtd)), "tridiag"
    assert np.array_equal(bits(to), bits(rto)), "trioffd"
    assert bits([emax])[0] == bits([rmax])[0], (emax, rmax)
    assert bits([emin])[0] == bits([rmin])[0], (emin, rmin)
    return emax, emin, td, to


@pytest.mark.parametrize("n,scaled", CASES)
@pytest.mark.parametrize("k", [1, 2, ITERS])
def test_extremes_bit_identical_to_the_restatement(amg, oracle, n, scaled, k):
    A, alpha, beta, gamma = case(oracle, n, scaled)
    assert eigs_ref.valid_iterations(alpha, gamma) == ITERS
    emax, emin, td, to = check_bitwise(amg, alpha[:k], beta[:k])
    assert 0.0 < emin <= emax
    if k == 1:
        assert emax == emin == 1.0 / alpha[0]


@pytest.mark.parametrize("n,scaled", CASES)
def test_extremes_against_numpy(amg, oracle, n, scaled):
    """against numpy.linalg.eigvalsh of the same T.  Measured with this rule on the four cases
    (k = 20), in units of eps ||T||_inf, (emax, emin): 6^3 (0.995, 1.088), 6^3 scaled (0.990,
    1.144), 8^3 (2.937, 1.484), 8^3 scaled (0.490, 0.261).  The worst ratio is 2.94; the bound
    is 8 x that -- the margin is for LAPACK's own backward error, which grows with k"""
    A, alpha, beta, gamma = case(oracle, n, scaled)
    emax, emin, td, to = amg.lanczos_extremes(alpha, beta, full=True)
    T = eigs_ref.tridiag_matrix(td, to)
    w = np.linalg.eigvalsh(T)
    norm = np.abs(T).sum(axis=1).max()
    ratios = (abs(emax - w[-1]) / (EPS * norm), abs(emin - w[0]) / (EPS * norm))
    print(f"{n}^3 scaled={scaled}: |emax - numpy| = {ratios[0]:.3f}, |emin - numpy| = {ratios[1]:.3f} eps ||T||inf")
    assert max(ratios) <= 8 * 2.94


@pytest.mark.parametrize("n,scaled", CASES)
def test_ritz_values_inside_the_spectrum_and_close_to_its_top(amg, oracle, n, scaled):
    A, alpha, beta, gamma = case(oracle, n, scaled)
    emax, emin = amg.lanczos_extremes(alpha, beta)
    lam = eigs_ref.dense_scaled_spectrum(A)
    slack = ITERS * A.nrows * EPS * lam[-1]
    assert lam[0] - slack <= emin <= emax <= lam[-1] + slack, (lam[0], emin, emax, lam[-1])
    print(f"{n}^3 scaled={scaled}: emax / lambda_max = {emax / lam[-1]:.8f}")
    assert emax >= 0.999 * lam[-1]


def test_scaling_leaves_the_estimate_nearly_unchanged(amg, oracle):
    """D^-1/2 A D^-1/2 of S A S is that of A: the two estimates differ by the start vector's scaling only"""
    e_plain = amg.lanczos_extremes(*case(oracle, 8, False)[1:3])
    e_scaled = amg.lanczos_extremes(*case(oracle, 8, True)[1:3])
    assert abs(e_plain[0] - e_scaled[0]) <= 1e-3 * e_plain[0]


def test_lehmer_stream(amg):
    ref = eigs_ref.lehmer_stream(3000)
    full = amg.lehmer_stream(3000)
    assert np.array_equal(bits(full), bits(ref))
    assert full[0] == 16807 / 2147483647.0 and np.all((full > 0.0) & (full < 1.0))
    # the 10000th value of the minimal standard generator from seed 1 (Park & Miller 1988)
    assert amg.lehmer_stream(1, skip=9999)[0] == 1043618065 / 2147483647.0
    for skip in (0, 1, 255, 1234, 2999):
        assert np.array_equal(bits(amg.lehmer_stream(3000 - skip, skip=skip)), bits(full[skip:])), skip
    assert amg.lehmer_stream(0, skip=5).size == 0
    big = 5 * 2147483646 + 17  # the stream's period is 2^31 - 2
    assert np.array_equal(bits(amg.lehmer_stream(4, skip=big)), bits(full[17:21]))
    other = amg.lehmer_stream(10, seed=12345)
    assert np.array_equal(bits(other), bits(eigs_ref.lehmer_stream(10, seed=12345)))


def test_statuses(amg):
    dp = C.POINTER(C.c_double)
    a, b = np.array([0.25, 0.2]), np.array([0.5, 0.1])
    td, to = np.zeros(2), np.zeros(2)
    emax, emin = C.c_double(), C.c_double()

    def call(k, al, be, tdp=None):
        return amg.lib.amg_lanczos_extremes(k, al.ctypes.data_as(dp), be.ctypes.data_as(dp),
                                            td.ctypes.data_as(dp) if tdp is None else tdp, to.ctypes.data_as(dp),
                                            C.byref(emax), C.byref(emin))

    assert call(2, a, b) == 0
    for k in (0, -3):
        assert call(k, a, b) == -5  # AMG_ERR_UNSUPPORTED
        assert b"no iteration" in amg.lib.amg_last_error()
    assert call(2, a, b, tdp=dp()) == -1  # AMG_ERR_ARG
    for bad in (0.0, np.nan, np.inf):
        assert call(2, np.array([0.25, bad]), b) == -1
    assert call(2, a, np.array([-0.5, 0.1])) == -1
    assert call(2, a, np.array([np.nan, 0.1])) == -1
    assert call(2, a, np.array([0.5, np.nan])) == 0  # the last beta is not read
    with pytest.raises(amg.AmgError):
        amg.lanczos_extremes([], [])
    out = np.zeros(4)
    for seed, skip, n in ((0, 0, 4), (2147483647, 0, 4), (1, -1, 4), (1, 0, -1)):
        assert amg.lib.amg_lehmer_stream(seed, skip, n, out.ctypes.data_as(dp)) == -1
    assert eigs_ref.estimate(np.array([0.0]), np.array([0.0]), np.array([0.0, 0.0])) == (None, None, 0)
