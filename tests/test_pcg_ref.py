"""The preconditioned-CG interface and its host model (no GPU needed).

The exported symbols; the numpy restatement of the device dot product
(pcg_ref.dev_dot) against an exact sum; the model recurrence (pcg_ref.pcg_model,
the oracle's cycle as M^-1) against the stationary iteration.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import pcg_ref

PCG_SYMBOLS = ["amg_pcg_solve", "amg_pcg_start", "amg_pcg_iterate", "amg_pcg_resnorm", "amg_pcg_get_x",
               "amg_pcg_scalars", "amg_precond_apply"]


def test_pcg_symbols_exported(amg):
    """every PCG entry is declared in the header, has a ctypes prototype and is in the library"""
    from async_multigrid_amd import abi
    declared = abi.header_symbols()
    assert os.path.exists(abi.LIB_PATH)
    lib = C.CDLL(abi.LIB_PATH)
    for name in PCG_SYMBOLS:
        assert name in declared, f"{name} not declared in the header"
        assert name in abi.PROTOTYPES, f"{name} has no prototype in abi.py"
        assert hasattr(lib, name), f"{name} not exported by the library"
    for name in ("precond_apply", "pcg_solve", "pcg_start", "pcg_iterate", "pcg_resnorm", "pcg_get_x",
                 "pcg_scalars"):
        assert hasattr(amg.Hier, name)


@pytest.mark.parametrize("n", [1, 255, 257, 2049, 70000])
def test_dev_dot_against_exact_sum(n):
    """the standard bound of a length-n summation in any order: n 2^-53 sum |x_i y_i|
    (each product's own rounding, 2^-53 |x_i y_i|, is inside it for n >= 2; n = 1 is exact
    against the rounded product)"""
    g = np.random.default_rng(n)
    x = g.uniform(-1, 1, n) * 10.0 ** g.integers(-3, 4, n)
    y = g.uniform(-1, 1, n)
    prods = x * y
    exact = math.fsum(prods.tolist())
    bound = n * 2.0 ** -53 * math.fsum(np.abs(prods).tolist())
    got = pcg_ref.dev_dot(x, y)
    assert abs(got - exact) <= bound, (got, exact, bound)
    if n == 1:
        assert got == prods[0]


def test_model_converges_faster_than_stationary(amg, oracle):
    """16^3 7-pt, 2-level linear hierarchy, Jacobi w = 0.8 V(1,1): after 8 iterations the model's
    recurrence residual is below the stationary cycle's after 8 cycles, with either dot product"""
    L, host = pcg_ref.host_hierarchy(amg, oracle, 16, levels=2)
    assert L == 2
    iters = 8
    opts = amg.default_opts(smooth_weight=0.8, num_cycles=iters, tol=0.0)
    f = amg.rhs_rand(0, 16 ** 3)
    _, h_stat, k = pcg_ref.oracle_hier(oracle, host, opts).solve(f)
    assert k == iters
    A = host["A"][0]
    for dot in (pcg_ref.dev_dot, lambda a, b: float(np.dot(a, b))):
        run = pcg_ref.pcg_model(oracle, host, opts, f, iters, dot)
        assert np.all(np.isfinite(run.hist))
        assert run.hist[-1] / run.hist[0] < h_stat[-1] / h_stat[0], (run.hist, h_stat)
        # the recurrence residual is the true residual up to rounding
        true = f - oracle.seq_matvec(A, run.xs[-1])
        assert np.linalg.norm(true - run.rs[-1]) <= 1e-12 * run.hist[0]
