"""Several right-hand sides at once on the MI355X (amg_mvec_*, amg_mrhs_*).

The oracle is the library's own single-vector path: column j of every multi-vector
result must carry the bits of the single-vector entry point applied to column j,
whatever storage form (marched, geometric, fused, 3x3 blocks, long-row kernel) that
one picks.  Columns are drawn with different seeds, so a column mix-up shows.  Norm
histories of the stationary solve pass through another summation order on the single
path (tile partials) and are held to rtol 1e-12, the project's bar for norms.
"""
import ctypes as C

import numpy as np
import pytest

import pcg_ref
from conftest import random_csr
from test_gpu_kernels import assert_bitwise

pytestmark = pytest.mark.gpu

AMG_ERR_ARG, AMG_ERR_UNSUPPORTED = -1, -5
WIDTHS = (2, 4, 8)
# every (alpha, beta) of test_gpu_kernels.py::test_spgemv_branches
AB = [(1, 0), (-1, 0), (2.5, 0), (1, -1), (-1, 1), (0.5, -0.5), (1, 1), (-1, -1), (3, 3), (1, 0.3), (-1, 0.7),
      (1.7, -0.4)]

_CACHE = {}


def cached(key, make):
    """a reference computed once and shared (never modified by its users)"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def draw(n, count, seed):
    """count vectors of n entries, each from its own seed"""
    return [np.random.default_rng(1000 * seed + j).uniform(-1, 1, n) for j in range(count)]


def mvec_of(ctx, cols, k):
    return ctx.mvec(np.ascontiguousarray(np.stack(cols[:k], axis=1)))


def dev_csr(ctx, M):
    return ctx.csr(M.nrows, M.ncols, M.rowptr, M.col, M.val)


# ---- 1. reductions and column moves ---------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2049, 262145])
def test_reductions_axpy_and_columns(amg, ctx, n):
    xs, ys = draw(n, 8, 1), draw(n, 8, 2)
    alpha = np.random.default_rng(3).uniform(-2, 2, 8)
    xv = [ctx.vec(x) for x in xs]
    yv = [ctx.vec(y) for y in ys]
    dots, norms, axpys = [], [], []
    out = C.c_double()
    for j in range(8):
        amg.check(amg.lib.amg_vec_dot(ctx.h, xv[j].h, yv[j].h, C.byref(out)))
        dots.append(out.value)
        norms.append(xv[j].norm2())
    for j in range(8):
        amg.check(amg.lib.amg_vec_axpy(ctx.h, float(alpha[j]), xv[j].h, yv[j].h))
        axpys.append(yv[j].download())
    for k in WIDTHS:
        X, Y = mvec_of(ctx, xs, k), mvec_of(ctx, ys, k)
        assert_bitwise(X.dot(Y), np.array(dots[:k]), f"dot n={n} k={k}")
        assert_bitwise(X.norm2(), np.array(norms[:k]), f"norm2 n={n} k={k}")
        Y.axpy(alpha[:k], X)
        got = Y.download()
        for j in range(k):
            assert_bitwise(got[:, j], axpys[j], f"axpy n={n} k={k} column {j}")
        # device-side pack and unpack
        Z = ctx.mvec((n, k))
        for j in range(k):
            Z.set_col(j, xv[k - 1 - j])
        got = Z.download()
        for j in range(k):
            assert_bitwise(got[:, j], xs[k - 1 - j], f"set_col n={n} k={k} column {j}")
            c = Z.col(j)
            assert_bitwise(c.download(), xs[k - 1 - j], f"get_col n={n} k={k} column {j}")
            c.free()
        Z.set(0.25)
        assert np.all(Z.download() == 0.25)
        for m in (X, Y, Z):
            m.free()
    for v in xv + yv:
        v.free()


# ---- 2. SpGEMV ---------------------------------------------------------------------------
def check_spgemv(amg, ctx, A, dA, pairs, ranges, seed, what, widths=WIDTHS):
    """every (alpha, beta), row range and b-aliases-y choice: the k-column result against
    amg_spgemv on each column, rows outside the range left as they were"""
    n, m = A.nrows, A.ncols
    xs, bs, y0 = draw(m, 8, seed), draw(n, 8, seed + 1), draw(n, 8, seed + 2)
    xv = [ctx.vec(x) for x in xs]
    bv = [ctx.vec(b) for b in bs]
    yv = ctx.vec(n)
    X = {k: mvec_of(ctx, xs, k) for k in widths}
    B = {k: mvec_of(ctx, bs, k) for k in widths}
    Y = {k: ctx.mvec((n, k)) for k in widths}
    y0k = {k: np.ascontiguousarray(np.stack(y0[:k], axis=1)) for k in widths}
    bk = {k: np.ascontiguousarray(np.stack(bs[:k], axis=1)) for k in widths}
    for alpha, beta in pairs:
        for rb, re in ranges:
            for alias in (False, True):
                ref = []
                for j in range(max(widths)):
                    yv.upload(bs[j] if alias else y0[j])
                    amg.check(amg.lib.amg_spgemv(ctx.h, dA.h, xv[j].h, yv.h if alias else bv[j].h, alpha, beta,
                                                 yv.h, rb, re))
                    ref.append(yv.download())
                for k in widths:
                    Y[k].upload(bk[k] if alias else y0k[k])
                    amg.check(amg.lib.amg_mrhs_spgemv(ctx.h, dA.h, X[k].h, Y[k].h if alias else B[k].h, alpha, beta,
                                                      Y[k].h, rb, re))
                    got = Y[k].download()
                    for j in range(k):
                        assert_bitwise(got[:, j], ref[j],
                                       f"{what} ab={(alpha, beta)} rows [{rb},{re}) alias={alias} k={k} column {j}")
    for v in xv + bv + [yv] + list(X.values()) + list(B.values()) + list(Y.values()):
        v.free()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1031])
def test_spgemv(amg, oracle, ctx, n):
    """rows of 0-14 entries, empty ones among them; square diagonal-first and rectangular
    n x (n/2 + 1) and n x 2n, and square with rows of up to 120 entries.  The row range (3, n - 2)
    exists from n = 5 on, so n = 1 runs the full range alone."""
    ranges = [(0, n)] + ([(3, n - 2)] if n >= 5 else [])
    mats = [("square", random_csr(oracle, n, n, 7, seed=10 + n)),
            ("rect_half", random_csr(oracle, n, n // 2 + 1, 7, seed=20 + n, diag_first=False)),
            ("rect_2n", random_csr(oracle, n, 2 * n, 7, seed=30 + n, diag_first=False)),
            # 32 or more entries per row on average (from n = 63 on): the long-row kernel
            ("square_60", random_csr(oracle, n, n, 60, seed=35 + n))]
    for name, A in mats:
        dA = dev_csr(ctx, A)
        check_spgemv(amg, ctx, A, dA, AB, ranges, 40 + n, f"{name} n={n}")
        X = mvec_of(ctx, draw(A.ncols, 2, 50), 2)
        Y, Y2 = ctx.mvec((n, 2)), ctx.mvec((n, 2))
        amg.check(amg.lib.amg_mrhs_matvec(ctx.h, dA.h, X.h, Y.h))
        amg.check(amg.lib.amg_mrhs_spgemv(ctx.h, dA.h, X.h, None, 1.0, 0.0, Y2.h, 0, n))
        assert_bitwise(Y.download().ravel(), Y2.download().ravel(), f"matvec {name} n={n}")
        for v in (X, Y, Y2):
            v.free()
        dA.free()


# ---- 3. long rows --------------------------------------------------------------------------
def long_row_matrix(oracle, n, m, long_row, seed):
    """short random rows and one row of 5000 entries: longer than any LDS chunk"""
    g = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        others = np.delete(np.arange(m), i)
        k = 4999 if i == long_row else int(g.integers(0, 12))
        rows.append([i] + sorted(g.choice(others, size=k, replace=False).tolist()))
    rp = np.cumsum([0] + [len(r) for r in rows])
    cj = np.concatenate([np.array(r, dtype=np.int32) for r in rows])
    cv = g.uniform(-1, 1, size=cj.size)
    cv[rp[:-1]] = 50.0
    return oracle.Csr(n, m, rp, cj, cv)


def check_one_sweep(amg, ctx, A, dA, seed, what):
    n = A.nrows
    fs, us = draw(n, 8, seed), draw(n, 8, seed + 1)
    ref = []
    for j in range(8):
        f, u, up = ctx.vec(fs[j]), ctx.vec(us[j]), ctx.vec(n)
        amg.check(amg.lib.amg_jacobi(ctx.h, dA.h, f.h, u.h, up.h, 0.8, 1, 0, 0, n, 0))
        ref.append(u.download())
        for v in (f, u, up):
            v.free()
    for k in WIDTHS:
        F, U, UP = mvec_of(ctx, fs, k), mvec_of(ctx, us, k), ctx.mvec((n, k))
        amg.check(amg.lib.amg_mrhs_jacobi(ctx.h, dA.h, F.h, U.h, UP.h, 0.8, 1, 0))
        got = U.download()
        for j in range(k):
            assert_bitwise(got[:, j], ref[j], f"{what}: Jacobi sweep k={k} column {j}")
        for v in (F, U, UP):
            v.free()


def test_long_rows(amg, oracle, ctx):
    """a 5000-entry row among short ones (130 x 6000, and square 5200 x 5200 for the sweep),
    and 100 entries in every row (300 x 300: the single path's long-row kernel)"""
    pairs = [(1, 0), (-1, 1), (1.7, -0.4)]
    wide = long_row_matrix(oracle, 130, 6000, 77, 5)
    assert np.diff(wide.rowptr).max() == 5000
    dA = dev_csr(ctx, wide)
    check_spgemv(amg, ctx, wide, dA, pairs, [(0, 130), (3, 128)], 60, "130 x 6000")
    dA.free()
    sq = long_row_matrix(oracle, 5200, 5200, 300, 6)
    assert np.diff(sq.rowptr).max() == 5000
    dA = dev_csr(ctx, sq)
    check_spgemv(amg, ctx, sq, dA, pairs[:2], [(0, 5200)], 63, "5200 x 5200")
    check_one_sweep(amg, ctx, sq, dA, 66, "5200 x 5200")
    dA.free()
    g = np.random.default_rng(8)
    rows = [[i] + sorted(g.choice(np.delete(np.arange(300), i), size=99, replace=False).tolist()) for i in range(300)]
    cj = np.array(rows, dtype=np.int32).ravel()
    cv = g.uniform(-1, 1, cj.size)
    cv[::100] = 60.0
    dense = oracle.Csr(300, 300, np.arange(0, 30001, 100), cj, cv)
    dA = dev_csr(ctx, dense)
    check_spgemv(amg, ctx, dense, dA, pairs, [(0, 300), (3, 298)], 70, "300 x 300 dense")
    check_one_sweep(amg, ctx, dense, dA, 73, "300 x 300 dense")
    dA.free()


# ---- 4. Jacobi and L1 Jacobi ------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 1031])
@pytest.mark.parametrize("l1", [False, True])
@pytest.mark.parametrize("density", [7, 60])
def test_jacobi_sweeps(amg, oracle, ctx, n, l1, density):
    """zero diagonals among the rows: the zero-guess sweep leaves those rows' u as it was;
    density 60 (32 or more entries per row on average) takes the long-row kernel"""
    A = random_csr(oracle, n, n, density, seed=80 + n, with_zero_diag=True)
    assert (A.rowptr[-1] // n >= 32) == (density == 60)
    dA = dev_csr(ctx, A)
    fs, us = draw(n, 8, 81), draw(n, 8, 82)
    lv = ctx.vec(n)
    amg.check(amg.lib.amg_l1_norms(ctx.h, dA.h, lv.h))  # 0 on the empty rows: inf / NaN there on both paths

    def single(f, u, up, sweeps, zf):
        if l1:
            return amg.lib.amg_l1_jacobi(ctx.h, dA.h, f.h, u.h, up.h, lv.h, sweeps, zf, 0, n, 0)
        return amg.lib.amg_jacobi(ctx.h, dA.h, f.h, u.h, up.h, 0.7, sweeps, zf, 0, n, 0)

    def multi(F, U, UP, sweeps, zf):
        if l1:
            return amg.lib.amg_mrhs_l1_jacobi(ctx.h, dA.h, F.h, U.h, UP.h, lv.h, sweeps, zf)
        return amg.lib.amg_mrhs_jacobi(ctx.h, dA.h, F.h, U.h, UP.h, 0.7, sweeps, zf)

    fv = [ctx.vec(f) for f in fs]
    u, up = ctx.vec(n), ctx.vec(n)
    for sweeps in (1, 2, 3):
        for zf in (0, 1):
            ref = []
            for j in range(8):
                u.upload(us[j])
                amg.check(single(fv[j], u, up, sweeps, zf))
                ref.append(u.download())
            for k in WIDTHS:
                F, U, UP = mvec_of(ctx, fs, k), mvec_of(ctx, us, k), ctx.mvec((n, k))
                amg.check(multi(F, U, UP, sweeps, zf))
                got = U.download()
                for j in range(k):
                    assert_bitwise(got[:, j], ref[j], f"l1={l1} n={n} sweeps={sweeps} zero_first={zf} k={k} column {j}")
                for v in (F, U, UP):
                    v.free()
    for v in fv + [u, up, lv]:
        v.free()
    dA.free()


# ---- hierarchies -------------------------------------------------------------------------------
def smoother_opts(amg, smoother, **kw):
    sm = {"jacobi": amg.AMG_JACOBI, "l1": amg.AMG_L1_JACOBI}[smoother]
    return amg.default_opts(**{"tol": 0.0, "smoother": sm, "smooth_weight": 0.8, **kw})


def linear_host(amg, oracle, n):
    return cached(("lin", n), lambda: pcg_ref.host_hierarchy(amg, oracle, n))


def elasticity_setup(amg):
    def make():
        n, rp, cj, v, b = amg.classical.elasticity(2)[:5]
        return n, b, amg.classical.ClassicalAMG(n, rp, cj, v, coarsen_type=9, strong_threshold=0.5, num_functions=3)
    return cached("elast2", make)


def make_hier(amg, oracle, ctx, which, opts):
    """(Hier, n0): the 16^3 linear hierarchy with default settings (the single path runs its
    marched, geometric and fused kernels) or the classical hierarchy of elasticity at refine 2
    (3x3 blocks on level 0)"""
    if which == "lin16":
        L, host = linear_host(amg, oracle, 16)
        assert L >= 3
        return pcg_ref.device_hier(amg, ctx, host, opts), 16 ** 3
    n, _, cl = elasticity_setup(amg)
    assert cl.L >= 3
    H = cl.hierarchy(ctx, opts)
    assert H._keep[0][0].bsr3 != 0
    return H, n


CASES = [("lin16", "jacobi"), ("lin16", "l1"), ("elast2", "jacobi"), ("elast2", "l1")]


# ---- 5. the cycle across storage forms --------------------------------------------------------
@pytest.mark.parametrize("which,smoother", CASES)
def test_precond_apply(amg, oracle, ctx, which, smoother):
    H, n = make_hier(amg, oracle, ctx, which, smoother_opts(amg, smoother, num_cycles=1))
    rs = draw(n, 8, 90)
    ref = [H.precond_apply(r) for r in rs]
    for count in (2, 3, 8):
        z = H.mrhs_precond_apply(rs[:count])
        z2 = H.mrhs_precond_apply(rs[:count])  # no state carried from one application to the next
        assert len(z) == count
        for j in range(count):
            assert_bitwise(z[j], ref[j], f"{which} {smoother}: M^-1 r, {count} vectors, column {j}")
            assert_bitwise(z2[j], ref[j], f"{which} {smoother}: second application, column {j}")
    H.free()


# ---- 6. stationary solve ----------------------------------------------------------------------
@pytest.mark.parametrize("which,smoother", CASES)
def test_stationary_solve(amg, oracle, ctx, which, smoother):
    """amg_solve fills its history only under check_resnorm 1, so the reference norms come from
    a second single solve with check_resnorm 1 and tol 0 (which never stops early)"""
    opts = smoother_opts(amg, smoother, num_cycles=5, check_resnorm=0)
    H, n = make_hier(amg, oracle, ctx, which, smoother_opts(amg, smoother, num_cycles=5, check_resnorm=1))
    fs, u0 = draw(n, 8, 91), [0.25 * v for v in draw(n, 8, 92)]
    norms = [H.solve(fs[j], u0[j])[1] for j in range(8)]
    H.set_opts(opts)
    ref = []
    for j in range(8):
        u, _, k = H.solve(fs[j], u0[j])
        assert len(norms[j]) == 6
        ref.append((u, norms[j], k))
    for count in (2, 4, 8):
        us, hist, done = H.mrhs_solve(fs[:count], u0[:count])
        assert done == 5 and hist.shape == (6, count)
        for j in range(count):
            assert ref[j][2] == 5
            assert_bitwise(us[j], ref[j][0], f"{which} {smoother}: iterate, {count} vectors, column {j}")
            np.testing.assert_allclose(hist[:, j], ref[j][1], rtol=1e-12, atol=0)
    H.free()


# ---- 7. PCG -------------------------------------------------------------------------------------
def check_pcg(amg, ctx, H, n, iters, count, seed, what):
    """x and the alpha / beta / rho history of every column bitwise the single solve's"""
    fs, x0 = draw(n, count, seed), [0.25 * v for v in draw(n, count, seed + 1)]
    ref = []
    for j in range(count):
        x, hist, k = H.pcg_solve(fs[j], x0[j])
        ref.append((x, hist, k, H.pcg_scalars()))
    xs, hist, done = H.mrhs_pcg_solve(fs, x0)
    assert done == iters and hist.shape == (iters + 1, count)
    for j in range(count):
        assert ref[j][2] == iters
        assert_bitwise(xs[j], ref[j][0], f"{what}: x, column {j}")
        got = H.mrhs_pcg_scalars(j)
        for name, a, b in zip(("alpha", "beta", "rho"), got, ref[j][3]):
            assert len(a) == iters
            assert_bitwise(a, b, f"{what}: {name}, column {j}")
        np.testing.assert_allclose(hist[:, j], ref[j][1], rtol=1e-12, atol=0)


@pytest.mark.parametrize("n", [16, 24])
def test_pcg_multi_level(amg, oracle, ctx, n):
    L, host = linear_host(amg, oracle, n)
    H = pcg_ref.device_hier(amg, ctx, host, smoother_opts(amg, "jacobi", num_cycles=10, check_resnorm=0))
    check_pcg(amg, ctx, H, n ** 3, 10, 4, 100 + n, f"{n}^3")
    H.free()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2049])
def test_pcg_one_level(amg, oracle, ctx, n):
    """L = 1, A = tridiag(-1, 4, -1): the tails and the single-workgroup reductions"""
    L, host = pcg_ref.tridiag_hierarchy(oracle, n)
    H = pcg_ref.device_hier(amg, ctx, host, smoother_opts(amg, "jacobi", num_cycles=10, check_resnorm=0))
    check_pcg(amg, ctx, H, n, 10, 4, 110, f"tridiag n={n}")
    H.free()


# ---- 8. the stop rule ------------------------------------------------------------------------
def test_stop_rule(amg, oracle, ctx):
    n = 16 ** 3
    L, host = linear_host(amg, oracle, 16)
    stop = smoother_opts(amg, "jacobi", num_cycles=50, check_resnorm=1, tol=1e-6)
    H = pcg_ref.device_hier(amg, ctx, host, stop)
    t = np.linspace(0.0, 1.0, n)
    smooth = np.sin(np.pi * t) + 0.5
    fs = [draw(n, 1, 120)[0], np.zeros(n), oracle.seq_matvec(host["A"][0], smooth), draw(n, 1, 121)[0]]
    singles = [H.pcg_solve(fs[j])[2] for j in (0, 2, 3)]
    xs, hist, done = H.mrhs_pcg_solve(fs)
    assert done == max(singles) and 0 < done < 50
    assert hist.shape == (done + 1, 4)
    # every column done at the last iteration, some column not done one before it
    assert all(hist[0, j] == 0 or hist[done, j] / hist[0, j] < 1e-6 for j in range(4))
    assert any(hist[0, j] != 0 and not hist[done - 1, j] / hist[0, j] < 1e-6 for j in range(4))
    H.set_opts(smoother_opts(amg, "jacobi", num_cycles=done, check_resnorm=0))
    for j in (0, 2, 3):
        x, h, k = H.pcg_solve(fs[j])
        assert k == done
        assert_bitwise(xs[j], x, f"column {j} after {done} iterations")
        np.testing.assert_allclose(hist[:, j], h, rtol=1e-12, atol=0)
    assert np.all(xs[1].view(np.uint64) == 0), "the zero column keeps x0 = 0"
    assert np.all(hist[:, 1] == 0.0)
    H.free()


# ---- 9. past one grid of lanes -------------------------------------------------------------
def test_past_one_grid_of_lanes(amg, oracle, ctx):
    """66^3 = 287 496 rows > 262 144: the grid-stride loops of the vector kernels wrap"""
    n = 66
    L, host = pcg_ref.host_hierarchy(amg, oracle, n, interp=amg.AMG_INTERP_AGGREGATE, levels=2)
    assert L == 2 and host["A"][0].nrows > 262144
    H = pcg_ref.device_hier(amg, ctx, host, smoother_opts(amg, "jacobi", num_cycles=2, check_resnorm=0))
    check_pcg(amg, ctx, H, n ** 3, 2, 2, 130, "66^3")
    H.free()


# ---- 10. isolation and refusals ------------------------------------------------------------
def test_single_vector_pcg_is_not_disturbed(amg, oracle, ctx):
    n = 16 ** 3
    L, host = linear_host(amg, oracle, 16)
    H = pcg_ref.device_hier(amg, ctx, host, smoother_opts(amg, "jacobi", num_cycles=4, check_resnorm=0))
    f, x0 = ctx.vec(draw(n, 1, 140)[0]), ctx.vec(n)
    out = ctx.vec(n)
    H.pcg_start(f, x0)
    H.pcg_iterate(5)
    H.pcg_get_x(out)
    ref = out.download()
    H.pcg_start(f, x0)
    H.pcg_iterate(3)
    H.mrhs_pcg_solve(draw(n, 3, 141))
    H.mrhs_solve(draw(n, 2, 142))
    H.mrhs_precond_apply(draw(n, 8, 143))
    H.pcg_iterate(2)
    H.pcg_get_x(out)
    assert_bitwise(out.download(), ref, "3 + 2 iterations around multi-vector calls")
    for v in (f, x0, out):
        v.free()
    H.free()


def last_error(amg):
    return amg.lib.amg_last_error() or b""


def test_refusals(amg, oracle, ctx):
    n = 16 ** 3
    L, host = linear_host(amg, oracle, 16)
    lib = amg.lib
    assert ctx.device_errors() == 0
    # widths other than 2, 4, 8
    h = C.c_void_p()
    assert lib.amg_mvec_create(ctx.h, 10, 3, C.byref(h)) == AMG_ERR_ARG
    assert b"amg_mvec_create" in last_error(amg)
    H = pcg_ref.device_hier(amg, ctx, host, smoother_opts(amg, "jacobi", num_cycles=2, check_resnorm=0))
    A0 = H._keep[0][0]
    a2, b4, c4, short4 = ctx.mvec((n, 2)), ctx.mvec((n, 4)), ctx.mvec((n, 4)), ctx.mvec((n - 1, 4))
    hist, k = np.zeros(3 * 8), C.c_int()
    hp = hist.ctypes.data_as(C.POINTER(C.c_double))
    calls = {
        "amg_mrhs_spgemv": lambda x, y: lib.amg_mrhs_spgemv(ctx.h, A0.h, x.h, None, 1.0, 0.0, y.h, 0, n),
        "amg_mrhs_matvec": lambda x, y: lib.amg_mrhs_matvec(ctx.h, A0.h, x.h, y.h),
        "amg_mrhs_jacobi": lambda x, y: lib.amg_mrhs_jacobi(ctx.h, A0.h, x.h, y.h, c4.h, 0.8, 1, 0),
        "amg_mrhs_precond_apply": lambda x, y: lib.amg_mrhs_precond_apply(H.h, x.h, y.h),
        "amg_mrhs_solve": lambda x, y: lib.amg_mrhs_solve(H.h, x.h, y.h, hp, C.byref(k)),
        "amg_mrhs_pcg_solve": lambda x, y: lib.amg_mrhs_pcg_solve(H.h, x.h, y.h, hp, C.byref(k)),
    }
    for name, call in calls.items():
        assert call(a2, b4) == AMG_ERR_ARG, f"{name}: widths that differ"
        assert name.encode() in last_error(amg) or b"amg_mrhs_spgemv" in last_error(amg)
        assert call(short4, b4) == AMG_ERR_ARG, f"{name}: wrong row count"
        assert last_error(amg)
    H.free()
    # hierarchies the multi-vector cycle does not restate
    unsupported = {
        "hybrid JGS": amg.default_opts(smoother=amg.AMG_HYBRID_JGS, tol=0.0, num_cycles=2),
        "BPX": amg.default_opts(solver=amg.AMG_BPX, smoother=amg.AMG_JACOBI, smooth_weight=0.6, tol=0.0, num_cycles=2),
        "Chebyshev": amg.default_opts(smoother=amg.AMG_JACOBI, smooth_weight=0.8, cheby_flag=1, cheby_mu=1.5,
                                      cheby_delta=1.0, tol=0.0, num_cycles=2),
    }
    for what, opts in unsupported.items():
        H = pcg_ref.device_hier(amg, ctx, host, opts)
        assert lib.amg_mrhs_precond_apply(H.h, b4.h, c4.h) == AMG_ERR_UNSUPPORTED, what
        assert b"amg_mrhs_precond_apply" in last_error(amg)
        assert lib.amg_mrhs_solve(H.h, b4.h, c4.h, hp, C.byref(k)) == AMG_ERR_UNSUPPORTED, what
        assert b"amg_mrhs_solve" in last_error(amg)
        assert lib.amg_mrhs_pcg_solve(H.h, b4.h, c4.h, hp, C.byref(k)) == AMG_ERR_UNSUPPORTED, what
        assert b"amg_mrhs_pcg_solve" in last_error(amg)
        H.free()
    assert np.all(c4.download() == 0.0), "a refused call writes nothing"
    assert ctx.device_errors() == 0
    for v in (a2, b4, c4, short4):
        v.free()
