"""The case table of cycle_cases.py against the oracle alone (no GPU): the
conditions under which test_gpu_cycle_options.py can tell a wrong cycle from a
right one."""
import itertools

import numpy as np
import pytest

import cycle_cases as cc

CYCLES = 6


def mult(amg, oracle, name, smoother, pair):
    return cc.oracle_solve(amg, oracle, name, cc.mult_opts(amg, smoother, pair[0], pair[1], CYCLES))


def additive(amg, oracle, name, solver, smoother, fine, coarse):
    return cc.oracle_solve(amg, oracle, name, cc.add_opts(amg, solver, smoother, fine, coarse, CYCLES))


@pytest.mark.parametrize("name", cc.HIERARCHIES)
def test_hierarchy_shapes(amg, oracle, name):
    L, hier = cc.host(amg, oracle, name)
    assert [A.nrows for A in hier["A"]] == cc.ROWS[name] and L == len(cc.ROWS[name])
    assert np.any(cc.guess(amg, name) != 0.0)


@pytest.mark.parametrize("smoother", cc.SMOOTHERS)
@pytest.mark.parametrize("name", cc.HIERARCHIES)
def test_every_mult_case_is_finite(amg, oracle, name, smoother):
    for pair in cc.SWEEPS:
        u, hist = mult(amg, oracle, name, smoother, pair)
        assert np.all(np.isfinite(u)) and np.all(np.isfinite(hist)), pair
        print(f"{name} {smoother} {pair}: relres {cc.relres(hist):.3e}")


@pytest.mark.parametrize("smoother", cc.SMOOTHERS)
@pytest.mark.parametrize("name", cc.MULTI_LEVEL)
def test_sweep_pairs_are_distinct(amg, oracle, name, smoother):
    """a device that ignored, swapped or clamped a sweep count reproduces another pair's iterate"""
    for a, b in itertools.combinations(cc.SWEEPS, 2):
        ua, ha = mult(amg, oracle, name, smoother, a)
        ub, hb = mult(amg, oracle, name, smoother, b)
        assert not cc.same_bits(ua, ub), (a, b)
        assert cc.relres(ha) != cc.relres(hb), (a, b)


@pytest.mark.parametrize("smoother", cc.SMOOTHERS)
def test_one_level_depends_on_the_sum_alone(amg, oracle, smoother):
    by_sum = {}
    for pair in cc.SWEEPS:
        u, _ = mult(amg, oracle, "tri257", smoother, pair)
        by_sum.setdefault(sum(pair), []).append(u)
    for us in by_sum.values():
        assert all(cc.same_bits(us[0], u) for u in us[1:])
    firsts = [us[0] for us in by_sum.values()]
    for ua, ub in itertools.combinations(firsts, 2):
        assert not cc.same_bits(ua, ub)
    assert sorted(sum(p) for p in cc.SWEEPS_ONE_LEVEL) == sorted(by_sum)


@pytest.mark.parametrize("smoother", cc.SMOOTHERS)
@pytest.mark.parametrize("name", cc.HIERARCHIES)
def test_no_sweeps_leave_the_guess(amg, oracle, name, smoother):
    u, hist = mult(amg, oracle, name, smoother, (0, 0))
    assert cc.same_bits(u, cc.guess(amg, name))
    assert np.all(hist == hist[0])


@pytest.mark.parametrize("smoother", cc.SMOOTHERS)
@pytest.mark.parametrize("name", ["lin16", "box"])
def test_additive_cases(amg, oracle, name, smoother):
    afacx = {fc: additive(amg, oracle, name, "afacx", smoother, *fc) for fc in [(1, 1)] + cc.FINE_COARSE}
    for fc, (u, hist) in afacx.items():
        assert np.all(np.isfinite(u)) and np.all(np.isfinite(hist)), fc
        print(f"{name} {smoother} AFACX {fc}: relres {cc.relres(hist):.3e}")
    for a, b in itertools.combinations(afacx, 2):
        assert not cc.same_bits(afacx[a][0], afacx[b][0]), (a, b)
        assert cc.relres(afacx[a][1]) != cc.relres(afacx[b][1]), (a, b)
    multadd = {fine: additive(amg, oracle, name, "multadd", smoother, fine, 1) for fine in [1] + cc.MULTADD_FINE}
    for fine, (u, hist) in multadd.items():
        assert np.all(np.isfinite(u)) and np.all(np.isfinite(hist)), fine
    for a, b in itertools.combinations(multadd, 2):
        assert not cc.same_bits(multadd[a][0], multadd[b][0]), (a, b)
    # MULTADD never reads num_coarse: the table does not pretend to vary it
    u12, h12 = additive(amg, oracle, name, "multadd", smoother, 1, 2)
    assert cc.same_bits(u12, multadd[1][0]) and cc.same_bits(h12, multadd[1][1])


@pytest.mark.parametrize("smoother", cc.SMOOTHERS)
@pytest.mark.parametrize("name", ["lin16", "agg2", "tri257"])
def test_pcg_model_reduces_the_residual(amg, oracle, name, smoother):
    for pre, post in cc.SWEEPS + [(2, 2)]:
        if pre + post == 0:
            continue
        run = cc.oracle_pcg(amg, oracle, name, cc.mult_opts(amg, smoother, pre, post, CYCLES), CYCLES)
        assert np.all(np.isfinite(run.xs[-1])) and np.all(np.isfinite(run.hist)), (pre, post)
        assert np.all(np.diff(run.hist) < 0), (pre, post, run.hist)
