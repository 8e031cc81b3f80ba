"""GPU: the classical setup's strength, transposes, PMIS and interpolation on the
device (amg_setup_dev.hip) and the device-resident level loop
(setup_on_device=1), every result bit for bit against the host path (device -1),
which tests/test_setup_phases.py pins against its restatements."""
import numpy as np
import pytest

from test_classical import aniso
from test_setup_phases import EDGE_THETA, edge_operator, pmis_np
from test_spgemm import crafted_operator
from test_truncation import DEFAULT_SEED, assert_csr_bitwise, assert_levels_bitwise, levels_of, problem

pytestmark = pytest.mark.gpu

INPUTS = ["lap12", "aniso", "elast2", "crafted", "edge1", "edge3"]
SEEDS = [DEFAULT_SEED, 1, 2 ** 63 + 12345]
_cache = {}


def operand(amg, oracle, name):
    """name -> dict(n, rp, cj, v, theta, nfun, srp, scj, cf: the host PMIS marker,
    cf0: the crafted marker of the edge operators); built once"""
    if name in _cache:
        return _cache[name]
    cf0 = None
    if name == "aniso":
        A = aniso(oracle, 40, 0.01)
        n, rp, cj, v, theta, nfun = A.nrows, A.rowptr, A.col, A.val, 0.25, 1
    elif name == "crafted":
        n, rp, cj, v = crafted_operator()
        theta, nfun = 0.25, 1
    elif name.startswith("edge"):
        nfun = int(name[4:])
        n, rp, cj, v, cf0 = edge_operator(nfun)
        theta = EDGE_THETA
    else:
        n, rp, cj, v, kw, nfun = problem(amg, oracle, name)
        theta = kw["strong_threshold"]
    srp, scj = amg.classical.strength(n, rp, cj, v, theta, num_functions=nfun)
    cf = amg.classical.pmis(n, srp, scj, DEFAULT_SEED)
    _cache[name] = dict(n=n, rp=rp, cj=cj, v=v, theta=theta, nfun=nfun, srp=srp, scj=scj, cf=cf, cf0=cf0)
    return _cache[name]


@pytest.mark.parametrize("name", INPUTS)
def test_strength(amg, oracle, name):
    o = operand(amg, oracle, name)
    cl = amg.classical
    got = cl.strength(o["n"], o["rp"], o["cj"], o["v"], o["theta"], num_functions=o["nfun"], device=0)
    assert np.array_equal(got[0], o["srp"]) and np.array_equal(got[1], o["scj"])
    # the row-sum test (a serial sum in storage order on the device)
    for mrs in (0.9, 0.1):
        host = cl.strength(o["n"], o["rp"], o["cj"], o["v"], o["theta"], mrs, o["nfun"])
        got = cl.strength(o["n"], o["rp"], o["cj"], o["v"], o["theta"], mrs, o["nfun"], device=0)
        assert np.array_equal(got[0], host[0]) and np.array_equal(got[1], host[1]), mrs


@pytest.mark.parametrize("values", [True, False])
@pytest.mark.parametrize("name", INPUTS)
def test_transpose(amg, oracle, name, values):
    o = operand(amg, oracle, name)
    cl = amg.classical
    v = o["v"] if values else None
    host = cl.transpose(o["n"], o["n"], o["rp"], o["cj"], v)
    got = cl.transpose(o["n"], o["n"], o["rp"], o["cj"], v, device=0)
    assert (got[2] is None) == (not values)
    assert_csr_bitwise(got[:2 + values], host[:2 + values], "A^T")
    # S^T (long rows at the hubs' neighbours) and a rectangular P
    host = cl.transpose(o["n"], o["n"], o["srp"], o["scj"])
    got = cl.transpose(o["n"], o["n"], o["srp"], o["scj"], device=0)
    assert_csr_bitwise(got[:2], host[:2], "S^T")
    P = cl.interp(o["n"], o["rp"], o["cj"], o["v"], o["srp"], o["scj"], o["cf"], 6, o["nfun"])
    pv = P[4] if values else None
    host = cl.transpose(P[0], P[1], P[2], P[3], pv)
    got = cl.transpose(P[0], P[1], P[2], P[3], pv, device=0)
    assert_csr_bitwise(got[:2 + values], host[:2 + values], "P^T")


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", INPUTS)
def test_pmis(amg, oracle, name, seed):
    o = operand(amg, oracle, name)
    host = amg.classical.pmis(o["n"], o["srp"], o["scj"], seed)
    got = amg.classical.pmis(o["n"], o["srp"], o["scj"], seed, device=0)
    assert set(np.unique(got)) <= {-1, 1}
    assert np.array_equal(got, host)


def pattern_of(rows):
    srp = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)
    return len(rows), srp, np.array([j for r in rows for j in r], dtype=np.int32)


def test_pmis_on_a_path(amg):
    """a path of 2000 points, every neighbour strong: the integer parts of the
    measures are equal, so the random parts alone order the rounds (3 or 4 of
    them for these seeds)"""
    n, srp, scj = pattern_of([[j for j in (i - 1, i + 1) if 0 <= j < 2000] for i in range(2000)])
    for seed in SEEDS:
        ref, rounds = pmis_np(n, srp, scj, seed)
        print(f"PMIS on a path of {n}, seed {seed}: {rounds} rounds, {int((ref == 1).sum())} C points")
        assert rounds >= 3
        assert np.array_equal(amg.classical.pmis(n, srp, scj, seed, device=0), ref)


def test_pmis_of_many_rounds(amg):
    """a chain of 60 points where point i also has i leaves that depend on it:
    |S^T_i| grows along the chain, so a round can only take the undecided end"""
    m = 60
    rows = [[j for j in (i - 1, i + 1) if 0 <= j < m] for i in range(m)]
    for i in range(m):
        rows += [[i]] * i
    n, srp, scj = pattern_of(rows)
    ref, rounds = pmis_np(n, srp, scj, DEFAULT_SEED)
    print(f"PMIS on the staircase chain ({n} points): {rounds} rounds")
    assert rounds >= m // 2
    assert np.array_equal(amg.classical.pmis(n, srp, scj, DEFAULT_SEED, device=0), ref)


def markers(o):
    return [("pmis", o["cf"])] + ([("crafted", o["cf0"])] if o["cf0"] is not None else [])


@pytest.mark.parametrize("itype", [6, 3])
@pytest.mark.parametrize("name", INPUTS)
def test_interp(amg, oracle, name, itype):
    o = operand(amg, oracle, name)
    for what, cf in markers(o):
        args = (o["n"], o["rp"], o["cj"], o["v"], o["srp"], o["scj"], cf, itype, o["nfun"])
        host = amg.classical.interp(*args)
        got = amg.classical.interp(*args, device=0)
        assert got[:2] == host[:2]
        assert_csr_bitwise(got[2:], host[2:], f"P ({what} marker)")


@pytest.mark.parametrize("nfun", [1, 3])
def test_interp_in_batches(amg, oracle, nfun):
    """the edge operator's extended+i rows under a scratch budget of a quarter of
    the whole (several batches) and under one below its largest row (that row a
    batch of its own); the result does not depend on the budget"""
    o = operand(amg, oracle, f"edge{nfun}")
    cf, sl = o["cf0"], np.diff(o["srp"])
    # the bound of include/amg_mi355x.h: |S_i| + |S_k| over the strong F neighbours
    ub = np.array([0 if cf[i] == 1 else sl[i] + sum(sl[k] for k in o["scj"][o["srp"][i]:o["srp"][i + 1]]
                                                     if cf[k] == -1) for i in range(o["n"])])
    assert ub.max() > 256
    args = (o["n"], o["rp"], o["cj"], o["v"], o["srp"], o["scj"], cf, 6, o["nfun"])
    host = amg.classical.interp(*args)
    try:
        for budget in (int(ub.sum()) // 4, int(ub.max()) - 1):
            amg.classical.set_setup_scratch(budget)
            got = amg.classical.interp(*args, device=0)
            assert_csr_bitwise(got[2:], host[2:], f"budget {budget}")
    finally:
        amg.classical.set_setup_scratch(0)


def setup_problem(amg, oracle, name):
    if name == "elast3":
        n, rp, cj, v, _ = amg.classical.elasticity(3)
        assert n == 15795
        return n, rp, cj, v, 0.5, 3
    n, rp, cj, v, kw, nfun = problem(amg, oracle, name)
    return n, rp, cj, v, kw["strong_threshold"], nfun


def assert_same_hierarchy(amg, Hd, Hh):
    assert Hd.L == Hh.L
    assert_levels_bitwise(levels_of(amg, Hd), levels_of(amg, Hh))
    for l in range(Hh.L - 1):
        assert np.array_equal(Hd.cf_marker(l), Hh.cf_marker(l)), l


@pytest.mark.parametrize("ct,it", [(9, 6), (8, 6), (9, 3), (10, 6)])
@pytest.mark.parametrize("name", ["lap12", "lap16", "elast2", "elast3"])
def test_resident_setup_matches_host(amg, oracle, name, ct, it):
    n, rp, cj, v, theta, nfun = setup_problem(amg, oracle, name)
    kw = dict(coarsen_type=ct, interp_type=it, strong_threshold=theta, num_functions=nfun)
    Hh = amg.classical.ClassicalAMG(n, rp, cj, v, **kw)
    Hd = amg.classical.ClassicalAMG(n, rp, cj, v, device=0, setup_on_device=1, **kw)
    # the default max_coarse_size: the loop runs down to levels shorter than a wavefront
    assert Hh.L >= 3 and Hh.get(amg.AMG_GEN_A, Hh.L - 1)[0] < 64
    assert_same_hierarchy(amg, Hd, Hh)


@pytest.mark.parametrize("name", ["lap12", "elast2"])
def test_resident_setup_with_truncation(amg, oracle, name):
    n, rp, cj, v, theta, nfun = setup_problem(amg, oracle, name)
    kw = dict(coarsen_type=9, strong_threshold=theta, num_functions=nfun, P_max_elmts=4, trunc_factor=0.2)
    Hh = amg.classical.ClassicalAMG(n, rp, cj, v, **kw)
    Hd = amg.classical.ClassicalAMG(n, rp, cj, v, device=0, setup_on_device=1, **kw)
    assert max(np.diff(Hd.get(amg.AMG_GEN_P, l)[2]).max() for l in range(Hd.L - 1)) <= 4
    assert_same_hierarchy(amg, Hd, Hh)


def test_refused_calls_leave_the_device_usable(amg, oracle):
    o = operand(amg, oracle, "lap12")
    cl = amg.classical
    bad = o["cj"].copy()
    bad[len(bad) // 2] = o["n"]
    with pytest.raises(amg.AmgError, match="column"):
        cl.strength(o["n"], o["rp"], bad, o["v"], o["theta"], device=0)
    with pytest.raises(amg.AmgError, match="column"):
        cl.transpose(o["n"], o["n"], o["rp"], bad, o["v"], device=0)
    with pytest.raises(amg.AmgError, match="column"):
        cl.interp(o["n"], o["rp"], bad, o["v"], o["srp"], o["scj"], o["cf"], device=0)
    with pytest.raises(amg.AmgError, match="cf"):
        cl.interp(o["n"], o["rp"], o["cj"], o["v"], o["srp"], o["scj"], np.zeros(o["n"], np.int32), device=0)
    with pytest.raises(amg.AmgError, match="column"):
        cl.ClassicalAMG(o["n"], o["rp"], bad, o["v"], coarsen_type=9, device=0, setup_on_device=1)
    got = cl.strength(o["n"], o["rp"], o["cj"], o["v"], o["theta"], device=0)
    assert np.array_equal(got[0], o["srp"]) and np.array_equal(got[1], o["scj"])
    Hh = cl.ClassicalAMG(o["n"], o["rp"], o["cj"], o["v"], coarsen_type=9)
    Hd = cl.ClassicalAMG(o["n"], o["rp"], o["cj"], o["v"], coarsen_type=9, device=0, setup_on_device=1)
    assert_same_hierarchy(amg, Hd, Hh)
