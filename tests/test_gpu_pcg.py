"""AMG-preconditioned conjugate gradients on the MI355X against the host model.

The recurrence is pinned statement by statement (one rounded fp64 operation
each, the dot products in amg_vec_dot's order), so the iterate, the residual
and the alpha / beta / rho history are compared bit for bit with
pcg_ref.pcg_model (the oracle's cycle as M^-1, pcg_ref.dev_dot as the dot
product).  Norms pass through a square root and are held to rtol 1e-12, the
project's bar for norms.
"""
import ctypes as C

import numpy as np
import pytest

import pcg_ref
from test_gpu_kernels import assert_bitwise

pytestmark = pytest.mark.gpu

_CACHE = {}


def cached(key, make):
    """a reference computed once and shared (never modified by its users)"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def case_opts(amg, name, **kw):
    base = {
        "mult_jacobi": dict(smoother=amg.AMG_JACOBI, smooth_weight=0.8),
        "mult_l1": dict(smoother=amg.AMG_L1_JACOBI, smooth_weight=0.8),
        "bpx": dict(solver=amg.AMG_BPX, smoother=amg.AMG_JACOBI, smooth_weight=0.6),
        "multadd": dict(solver=amg.AMG_MULTADD, smoother=amg.AMG_JACOBI, smooth_weight=0.8, smooth_transfer=1),
        "afacx": dict(solver=amg.AMG_AFACX, smoother=amg.AMG_JACOBI, smooth_weight=0.8),
    }[name]
    return amg.default_opts(**{"tol": 0.0, **base, **kw})


def linear_host(amg, oracle, n):
    return cached(("host", n), lambda: pcg_ref.host_hierarchy(amg, oracle, n))


def check_run(amg, H, ctx, f, run, iters, what):
    """drive H one iteration at a time; x after every iteration, r at the end and the
    scalar history bitwise the model's; the norm history within rtol 1e-12"""
    fv, xv = ctx.vec(f), ctx.vec(run.xs[0])
    out = ctx.vec(len(f))
    r0 = H.pcg_start(fv, xv)
    hist = [r0]
    for k in range(1, iters + 1):
        H.pcg_iterate(1)
        H.pcg_get_x(out)
        assert_bitwise(out.download(), run.xs[k], f"{what}: x after iteration {k}")
        hist.append(H.pcg_resnorm())
    assert_bitwise(H.vec(amg.AMG_VEC_R, 0).download(), run.rs[iters], f"{what}: recurrence residual")
    a, b, rho = H.pcg_scalars()
    assert len(a) == iters
    assert_bitwise(a, np.array(run.alpha), f"{what}: alpha")
    assert_bitwise(b, np.array(run.beta), f"{what}: beta")
    assert_bitwise(rho, np.array(run.rho), f"{what}: rho")
    np.testing.assert_allclose(hist, run.hist, rtol=1e-12, atol=0)
    for v in (fv, xv, out):
        v.free()
    return np.array(hist)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2049, 262145])
def test_dev_dot_is_amg_vec_dot(amg, ctx, n):
    """the reduction order as it stands: pins the helper, not the feature"""
    g = np.random.default_rng(n)
    x, y = g.uniform(-1, 1, n), g.uniform(-1, 1, n)
    xv, yv = ctx.vec(x), ctx.vec(y)
    out = C.c_double()
    amg.check(amg.lib.amg_vec_dot(ctx.h, xv.h, yv.h, C.byref(out)))
    xv.free()
    yv.free()
    assert np.float64(out.value).view(np.uint64) == np.float64(pcg_ref.dev_dot(x, y)).view(np.uint64)


@pytest.mark.parametrize("name", ["mult_jacobi", "mult_l1", "bpx", "multadd", "afacx"])
def test_precond_apply_is_the_oracles(amg, oracle, ctx, name):
    L, host = linear_host(amg, oracle, 16)
    opts = case_opts(amg, name, num_cycles=1)
    r = amg.rhs_rand(0, 16 ** 3)
    H = pcg_ref.device_hier(amg, ctx, host, opts)
    z = H.precond_apply(r)
    z2 = H.precond_apply(r)  # no state carried from one application to the next
    H.free()
    assert_bitwise(z, pcg_ref.oracle_precond(oracle, host, opts)(r), f"M^-1 r ({name})")
    assert_bitwise(z2, z, "second application")


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2049])
def test_one_level(amg, oracle, ctx, n):
    """L = 1, A = tridiag(-1, 4, -1): M^-1 is two Jacobi sweeps from zero; the tails of the
    fused kernels and the single-workgroup reductions"""
    L, host = pcg_ref.tridiag_hierarchy(oracle, n)
    iters = 6
    opts = case_opts(amg, "mult_jacobi", num_cycles=iters)
    f = amg.rhs_rand(0, n)
    run = pcg_ref.pcg_model(oracle, host, opts, f, iters, pcg_ref.dev_dot)
    H = pcg_ref.device_hier(amg, ctx, host, opts)
    check_run(amg, H, ctx, f, run, iters, f"tridiag n={n}")
    H.free()


@pytest.mark.parametrize("name,n", [("mult_jacobi", 24), ("mult_l1", 24), ("bpx", 16), ("multadd", 16)])
def test_multi_level(amg, oracle, ctx, name, n):
    L, host = linear_host(amg, oracle, n)
    assert L >= (4 if n == 24 else 3)
    iters = 10
    opts = case_opts(amg, name, num_cycles=iters)
    f = amg.rhs_rand(0, n ** 3)
    run = pcg_ref.pcg_model(oracle, host, opts, f, iters, pcg_ref.dev_dot)
    H = pcg_ref.device_hier(amg, ctx, host, opts)
    hist = check_run(amg, H, ctx, f, run, iters, name)
    _, h_stat, k = H.solve(f)
    H.free()
    assert k == iters
    print(f"{name}: relres after {iters}: PCG {hist[-1] / hist[0]:.3e}, stationary {h_stat[-1] / h_stat[0]:.3e}")
    assert hist[-1] / hist[0] < h_stat[-1] / h_stat[0]


def test_past_one_grid_of_lanes(amg, oracle, ctx):
    """66^3 = 287 496 rows > 262 144: the grid-stride loops of the vector kernels wrap"""
    n = 66
    L, host = pcg_ref.host_hierarchy(amg, oracle, n, interp=amg.AMG_INTERP_AGGREGATE, levels=2)
    assert L == 2 and host["A"][0].nrows > 262144
    iters = 3
    opts = case_opts(amg, "mult_jacobi", num_cycles=iters)
    f = amg.rhs_rand(0, n ** 3)
    run = pcg_ref.pcg_model(oracle, host, opts, f, iters, pcg_ref.dev_dot)
    H = pcg_ref.device_hier(amg, ctx, host, opts)
    check_run(amg, H, ctx, f, run, iters, "66^3")
    H.free()


@pytest.mark.parametrize("name", ["mult_jacobi", "mult_l1"])
def test_nonuniform_and_zero_diagonal(amg, oracle, ctx, name):
    """the zero-guess sweep folded into the residual update reads a_ii per row where the diagonal is
    not one value, and leaves 0 where a_ii = 0 (the cleared u that jacobi_zero does not touch): 16^3,
    2-level aggregation, A_0 + diag(d) with d in [0, 2) and two rows' diagonals set to 0"""
    n = 16
    L, host = cached(("host_agg", n), lambda: pcg_ref.host_hierarchy(amg, oracle, n, interp=amg.AMG_INTERP_AGGREGATE,
                                                                     levels=2))
    A = host["A"][0]
    val = A.val.copy()
    val[A.rowptr[:-1]] += np.random.default_rng(5).uniform(0.0, 2.0, A.nrows)
    val[A.rowptr[[7, 2049]]] = 0.0
    host = {"A": [oracle.Csr(A.nrows, A.ncols, A.rowptr, A.col, val), host["A"][1]], "P": host["P"], "R": host["R"]}
    iters = 3
    opts = case_opts(amg, name, num_cycles=iters)
    f = amg.rhs_rand(0, n ** 3)
    run = pcg_ref.pcg_model(oracle, host, opts, f, iters, pcg_ref.dev_dot)
    assert np.all(np.isfinite(run.xs[-1]))
    H = pcg_ref.device_hier(amg, ctx, host, opts)
    check_run(amg, H, ctx, f, run, iters, f"non-uniform diagonal ({name})")
    H.free()


def test_split_and_one_shot_agree(amg, oracle, ctx):
    L, host = linear_host(amg, oracle, 16)
    opts = case_opts(amg, "mult_jacobi", num_cycles=5, check_resnorm=0)
    f = amg.rhs_rand(0, 16 ** 3)
    x0 = 0.25 * amg.rhs_rand(7, 7 + 16 ** 3)
    H = pcg_ref.device_hier(amg, ctx, host, opts)
    x_one, h_one, k = H.pcg_solve(f, x0)
    assert k == 5 and len(h_one) == 6
    fv, xv, out = ctx.vec(f), ctx.vec(x0), ctx.vec(16 ** 3)

    def split(parts):
        r0 = H.pcg_start(fv, xv)
        for p in parts:
            H.pcg_iterate(p)
        H.pcg_get_x(out)
        return out.download(), r0, H.pcg_resnorm(), H.pcg_scalars()

    x5, r0, rn5, sc5 = split([5])
    x32, _, rn32, sc32 = split([3, 2])
    H.free()
    assert_bitwise(x5, x_one, "start + iterate(5) + get_x against pcg_solve")
    assert_bitwise(x32, x5, "iterate(3) + iterate(2) against iterate(5)")
    assert r0 == h_one[0] and rn5 == h_one[-1] and rn32 == rn5
    for a, b in zip(sc5, sc32):
        assert_bitwise(a, b, "scalar history")
    assert np.all(h_one[1:] > 0) and h_one[-1] < h_one[0]


def test_stops_on_tolerance(amg, oracle, ctx):
    L, host = linear_host(amg, oracle, 16)
    cap = 30
    opts = case_opts(amg, "mult_jacobi", num_cycles=cap, tol=1e-6, check_resnorm=1)
    f = amg.rhs_rand(0, 16 ** 3)
    run = pcg_ref.pcg_model(oracle, host, opts, f, cap, pcg_ref.dev_dot)
    rel = run.hist / run.hist[0]
    k_model = int(np.argmax(rel < 1e-6))
    assert 0 < k_model < cap
    H = pcg_ref.device_hier(amg, ctx, host, opts)
    x, hist, k = H.pcg_solve(f)
    H.free()
    assert k == k_model and len(hist) == k + 1
    assert hist[-1] / hist[0] < 1e-6 <= hist[-2] / hist[0]
    assert_bitwise(x, run.xs[k], "iterate at the stop")
    np.testing.assert_allclose(hist, run.hist[:k + 1], rtol=1e-12, atol=0)


def test_zero_right_hand_side(amg, oracle, ctx):
    L, host = linear_host(amg, oracle, 16)
    opts = case_opts(amg, "mult_jacobi", num_cycles=4, check_resnorm=1)
    H = pcg_ref.device_hier(amg, ctx, host, opts)
    x, hist, k = H.pcg_solve(np.zeros(16 ** 3))
    a, b, rho = H.pcg_scalars()
    H.free()
    assert k == 4 and len(a) == 4
    assert np.array_equal(x, np.zeros(16 ** 3))
    assert np.array_equal(hist, np.zeros(5))
    for s in (a, b, rho):
        assert np.all(np.isfinite(s)) and np.all(s == 0.0)


def test_async_hierarchies_are_refused(amg, oracle, ctx):
    L, host = linear_host(amg, oracle, 16)
    opts = amg.default_opts(solver=amg.AMG_ASYNC_MULTADD, smooth_weight=0.8, num_cycles=3, tol=0.0)
    H = pcg_ref.device_hier(amg, ctx, host, opts)
    fv, xv = ctx.vec(amg.rhs_rand(0, 16 ** 3)), ctx.vec(16 ** 3)
    for call in (lambda: amg.lib.amg_pcg_start(H.h, fv.h, xv.h, None),
                 lambda: amg.lib.amg_pcg_solve(H.h, fv.h, xv.h, None, None),
                 lambda: amg.lib.amg_precond_apply(H.h, fv.h, xv.h)):
        assert call() < 0
        assert b"cannot precondition CG" in amg.lib.amg_last_error()
    assert amg.lib.amg_pcg_iterate(H.h, 1) < 0  # no state was created
    with pytest.raises(amg.AmgError):
        H.pcg_solve(amg.rhs_rand(0, 16 ** 3))
    H.free()
