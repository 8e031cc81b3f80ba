"""Host model of the CG-Lanczos eigenvalue estimate (amg_eigs_cg, amg_dist_eigs_cg,
amg_lanczos_extremes, amg_lehmer_stream).

Test infrastructure only.  eigs_model restates csrc/amg_eig.h's recurrence statement by
statement with the device's dot product (pcg_ref.dev_dot, or dist_pcg_ref.dist_dot of a row
partition) and the oracle's sequential product, so with every numpy operation one rounded fp64
operation its alpha / beta / gamma history has the device's bits.  lanczos_extremes restates the
header comment of amg_lanczos_extremes in Python floats.
"""
import math
import sys

import numpy as np

import pcg_ref

EPS = sys.float_info.epsilon
DBL_MIN = sys.float_info.min
LEHMER_M = 2147483647


# ---- the start vector -----------------------------------------------------------
def lehmer_stream(n, seed=1, skip=0):
    """u[j] = w_{skip + j + 1} / (2^31 - 1), w_0 = seed, w <- 16807 w mod (2^31 - 1), one step at a time"""
    w = seed
    for _ in range(skip):
        w = 16807 * w % LEHMER_M
    out = np.empty(n)
    for j in range(n):
        w = 16807 * w % LEHMER_M
        out[j] = w / 2147483647.0
    return out


def default_start(n, row0=0):
    """2 u_g - 1 by global row g"""
    return 2.0 * lehmer_stream(n, 1, row0) - 1.0


# ---- the recurrence -------------------------------------------------------------
def diag_of(A):
    """a_ii as the library reads it: the first entry of every row"""
    return np.array(A.val[np.asarray(A.rowptr[:-1])], dtype=np.float64)


def eigs_model(oracle, A, iters, scale=1, r0=None, dot=pcg_ref.dev_dot):
    """(alpha[iters], beta[iters], gamma[iters + 1]) of amg_eigs_cg on the host"""
    n = A.nrows
    r = default_start(n) if r0 is None else np.array(r0, dtype=np.float64)
    d = diag_of(A) if scale else None
    z = r / d if scale else r
    gam = dot(r, z)
    alpha, beta, gamma = [], [], [gam]
    p = None
    for i in range(iters):
        z = r / d if scale else r
        p = z.copy() if i == 0 else z + beta[-1] * p
        q = oracle.seq_matvec(A, p)
        pq = dot(p, q)
        a = gam / pq if pq != 0.0 else 0.0
        r = r - a * q
        z = r / d if scale else r
        gnew = dot(r, z)
        b = gnew / gam if gam != 0.0 else 0.0
        gam = gnew
        alpha.append(a)
        beta.append(b)
        gamma.append(gam)
    return np.array(alpha), np.array(beta), np.array(gamma)


def valid_iterations(alpha, gamma):
    """the leading iterations with gamma_i >= DBL_EPSILON and alpha_i finite and positive"""
    k = 0
    while k < len(alpha) and gamma[k] >= EPS and math.isfinite(alpha[k]) and alpha[k] > 0.0:
        k += 1
    return k


# ---- the tridiagonal and its extremes -------------------------------------------
def tridiagonal(alpha, beta):
    k = len(alpha)
    td, to = [0.0] * k, [0.0] * k
    td[0] = 1.0 / float(alpha[0])
    for i in range(1, k):
        ia = 1.0 / float(alpha[i - 1])
        td[i] = ia * float(beta[i - 1]) + 1.0 / float(alpha[i])
        to[i] = ia * math.sqrt(float(beta[i - 1]))
    return td, to


def sturm_count(td, to, x):
    cnt = 0
    q = td[0] - x
    if q == 0.0:
        q = -DBL_MIN
    if q < 0.0:
        cnt += 1
    for i in range(1, len(td)):
        q = (td[i] - x) - (to[i] * to[i]) / q  # a float division overflows to inf, as IEEE does
        if q == 0.0:
            q = -DBL_MIN
        if q < 0.0:
            cnt += 1
    return cnt


def lanczos_extremes(alpha, beta):
    """(emax, emin, tridiag, trioffd) by amg_lanczos_extremes' rule"""
    td, to = tridiagonal(alpha, beta)
    k = len(td)
    lo = hi = None
    for i in range(k):
        rad = abs(to[i]) + (abs(to[i + 1]) if i + 1 < k else 0.0)
        a, b = td[i] - rad, td[i] + rad
        lo = a if lo is None or a < lo else lo
        hi = b if hi is None or b > hi else hi
    l, h = lo, hi
    m = 0.5 * (l + h)
    while l < m < h:
        if sturm_count(td, to, m) == k:
            h = m
        else:
            l = m
        m = 0.5 * (l + h)
    emax = h
    l, h = lo, hi
    m = 0.5 * (l + h)
    while l < m < h:
        if sturm_count(td, to, m) >= 1:
            h = m
        else:
            l = m
        m = 0.5 * (l + h)
    return emax, l, np.array(td), np.array(to)


def tridiag_matrix(td, to):
    k = len(td)
    T = np.diag(np.asarray(td, dtype=np.float64))
    for i in range(1, k):
        T[i, i - 1] = T[i - 1, i] = to[i]
    return T


def estimate(alpha, beta, gamma):
    """(emax, emin, k) as the entries return them; k = 0: (None, None, 0)"""
    k = valid_iterations(alpha, gamma)
    if k == 0:
        return None, None, 0
    emax, emin, _, _ = lanczos_extremes(alpha[:k], beta[:k])
    return emax, emin, k


# ---- operators ------------------------------------------------------------------
def tridiag_varied(oracle, n):
    """tridiag(-1, 4 + 0.25 (i % 5), -1), the diagonal first in every row"""
    rp, col, val = [0], [], []
    for i in range(n):
        col.append(i)
        val.append(4.0 + 0.25 * (i % 5))
        for j in (i - 1, i + 1):
            if 0 <= j < n:
                col.append(j)
                val.append(-1.0)
        rp.append(len(col))
    return oracle.Csr(n, n, np.array(rp), np.array(col, dtype=np.int32), np.array(val))


def sym_scaled(oracle, A, seed=3):
    """S A S with S = diag(s), s in [0.5, 2): symmetric, a non-uniform diagonal, the same D^-1/2 A D^-1/2"""
    s = np.random.default_rng(seed).uniform(0.5, 2.0, A.nrows)
    rows = np.repeat(np.arange(A.nrows), np.diff(A.rowptr))
    return oracle.Csr(A.nrows, A.ncols, A.rowptr, A.col, A.val * (s[rows] * s[A.col]))


def dense_scaled_spectrum(A):
    """eigenvalues of D^-1/2 A D^-1/2, ascending"""
    M = np.zeros((A.nrows, A.ncols))
    M[np.repeat(np.arange(A.nrows), np.diff(A.rowptr)), A.col] = A.val
    ds = 1.0 / np.sqrt(diag_of(A))
    return np.linalg.eigvalsh(ds[:, None] * M * ds[None, :])
