"""GPU: interpolation truncation (amg_trunc.hip) and the smoothed-transfer setup
on the device, bit-identical to the host path (tests/test_truncation.py pins the
host path against the numpy restatement and the oracle), and the solve phase on
the hierarchies they produce, bit-identical to the oracle."""
import numpy as np
import pytest

from test_gpu_solve import compare_solve, oracle_opts
from test_gpu_kernels import assert_bitwise
from test_truncation import (PAIRS, assert_csr_bitwise, assert_levels_bitwise, crafted_rows, levels_of, problem)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def elast2_P1(amg, oracle):
    """level-1 P of elasticity r = 2 (rows of up to 52 entries)"""
    n, rp, cj, v, kw, nfun = problem(amg, oracle, "elast2")
    H = amg.classical.ClassicalAMG(n, rp, cj, v, num_functions=nfun, **kw)
    P = H.get(amg.AMG_GEN_P, 1)
    assert np.diff(P[2]).max() >= 40
    return P


@pytest.mark.parametrize("tf,mx", PAIRS)
def test_device_rule_matches_host(amg, elast2_P1, tf, mx):
    n, rp, cj, v = crafted_rows()
    assert_csr_bitwise(amg.classical.truncate_rows(n, rp, cj, v, tf, mx, device=0),
                       amg.classical.truncate_rows(n, rp, cj, v, tf, mx, device=-1), "crafted")
    pn, _, prp, pcj, pv = elast2_P1
    assert_csr_bitwise(amg.classical.truncate_rows(pn, prp, pcj, pv, tf, mx, device=0),
                       amg.classical.truncate_rows(pn, prp, pcj, pv, tf, mx, device=-1), "elasticity P1")


def test_device_noop_is_bitwise(amg):
    n, rp, cj, v = crafted_rows()
    for tf, mx in ((0.0, 0), (0.0, int(np.diff(rp).max()))):
        assert_csr_bitwise(amg.classical.truncate_rows(n, rp, cj, v, tf, mx, device=0), (rp, cj, v), (tf, mx))


@pytest.mark.parametrize("name", ["lap12", "elast2"])
def test_device_setup_matches_host(amg, oracle, name):
    n, rp, cj, v, kw, nfun = problem(amg, oracle, name)
    kw = dict(kw, num_functions=nfun, P_max_elmts=4, trunc_factor=0.2)
    Hh = amg.classical.ClassicalAMG(n, rp, cj, v, **kw)
    Hd = amg.classical.ClassicalAMG(n, rp, cj, v, device=0, **kw)
    assert Hh.L >= 3
    assert_levels_bitwise(levels_of(amg, Hd), levels_of(amg, Hh))


def smoothed_of(amg, H):
    return [(H.get(amg.AMG_GEN_PS, l), H.get(amg.AMG_GEN_RS, l)) for l in range(H.L - 1)]


def test_device_smoothed_transfers(amg, oracle):
    n, rp, cj, v, kw, _ = problem(amg, oracle, "lap12")
    H = amg.classical.ClassicalAMG(n, rp, cj, v, **kw)
    lv = levels_of(amg, H)
    H.smooth_transfers(0.8, device=0)
    for l, (ps, rs) in enumerate(smoothed_of(amg, H)):
        ops, ors = oracle.smooth_transfer(oracle.Csr(*lv["A"][l]), oracle.Csr(*lv["P"][l]), 0.8)
        assert (ps[0], ps[1], rs[0], rs[1]) == (ops.nrows, ops.ncols, ors.nrows, ors.ncols)
        assert_csr_bitwise(ps[2:], (ops.rowptr, ops.col, ops.val), f"PS{l}")
        assert_csr_bitwise(rs[2:], (ors.rowptr, ors.col, ors.val), f"RS{l}")
    H.smooth_transfers(0.8, add_P_max_elmts=8, add_trunc_factor=0.1, device=0)
    dev = smoothed_of(amg, H)
    H.smooth_transfers(0.8, add_P_max_elmts=8, add_trunc_factor=0.1, device=-1)
    for l, ((dp, dr), (hp, hr)) in enumerate(zip(dev, smoothed_of(amg, H))):
        assert dp[:2] == hp[:2] and dr[:2] == hr[:2]
        assert np.diff(dp[2]).max() <= 8
        assert_csr_bitwise(dp[2:], hp[2:], f"truncated PS{l}")
        assert_csr_bitwise(dr[2:], hr[2:], f"truncated RS{l}")


def test_vcycle_on_truncated_laplacian(amg, oracle, ctx):
    n, rp, cj, v, kw, _ = problem(amg, oracle, "lap16")
    H = amg.classical.ClassicalAMG(n, rp, cj, v, P_max_elmts=4, trunc_factor=0.2, device=0, **kw)
    host = {k: [oracle.Csr(*m) for m in ms] for k, ms in levels_of(amg, H).items()}
    opts = amg.default_opts(smooth_weight=0.8, num_cycles=12, tol=0.0)
    u, hist = compare_solve(amg, oracle, ctx, host, opts, amg.rhs_rand(0, n))
    print(f"truncated 16^3 V-cycle: relres {hist[-1] / hist[0]:.3e}")
    assert hist[-1] < 1e-3 * hist[0]


def test_vcycle_on_truncated_elasticity(amg, oracle, ctx):
    n, rp, cj, v, b = amg.classical.elasticity(2)
    H = amg.classical.ClassicalAMG(n, rp, cj, v, coarsen_type=9, strong_threshold=0.5, num_functions=3,
                                   P_max_elmts=4, trunc_factor=0.2, device=0)
    host = {k: [oracle.Csr(*m) for m in ms] for k, ms in levels_of(amg, H).items()}
    opts = amg.default_opts(smooth_weight=0.6, num_cycles=10, tol=0.0)
    u, hist = compare_solve(amg, oracle, ctx, host, opts, b)
    print(f"truncated elasticity r=2 V-cycle: history {hist / hist[0]}")
    assert np.all(np.diff(hist) < 0)


def test_multadd_on_truncated_smoothed_transfers(amg, oracle, ctx):
    n, rp, cj, v, kw, _ = problem(amg, oracle, "lap12")
    H = amg.classical.ClassicalAMG(n, rp, cj, v, **kw)
    H.smooth_transfers(0.8, add_P_max_elmts=8, device=0)
    opts = amg.default_opts(solver=amg.AMG_MULTADD, smooth_weight=0.8, num_cycles=10, tol=0.0)
    Hd = H.hierarchy(ctx, opts, smoothed=True)
    f = amg.rhs_rand(0, n)
    u_g, h_g, k_g = Hd.solve(f)
    Hd.free()
    As = [oracle.Csr(*H.get(amg.AMG_GEN_A, l)) for l in range(H.L)]
    Ps = [oracle.Csr(*H.get(amg.AMG_GEN_PS, l)) for l in range(H.L - 1)]
    Rs = [oracle.Csr(*H.get(amg.AMG_GEN_RS, l)) for l in range(H.L - 1)]
    OH = oracle.Hier(As, Ps, Rs, oracle_opts(oracle, opts))
    u_c, h_c, k_c = OH.solve(f)
    assert k_g == k_c == 10
    assert_bitwise(u_g, u_c, "iterate u")
    np.testing.assert_allclose(h_g, h_c, rtol=1e-12, atol=0)
    print(f"MULTADD on truncated smoothed transfers: relres {h_g[-1] / h_g[0]:.3e}")
    assert h_g[-1] < 1e-3 * h_g[0]
