"""The option space of the cycles (amg_solver.cpp: vcycle, smooth_one_level,
outer_residual, pcg_precond; amg_mrhs.cpp: cycle) as one table of cases, with the
oracle's answer to each.

Test infrastructure only.  test_cycle_cases.py checks on the host that the table
can tell a wrong cycle from a right one (every two sweep pairs give different
iterates, so a device that ignored or clamped a count could not pass);
test_gpu_cycle_options.py runs the table on the device.  Oracle results are
computed once per process and shared; their users never modify them.
"""
import numpy as np

import pcg_ref

# (num_pre_smooth_sweeps, num_post_smooth_sweeps) of the multiplicative cycle
SWEEPS = [(0, 1), (1, 0), (0, 2), (2, 0), (2, 1), (1, 2), (3, 3), (0, 0)]
# on one level the cycle is pre + post plain sweeps: one pair per sum
SWEEPS_ONE_LEVEL = [(0, 1), (0, 2), (2, 1), (3, 3), (0, 0)]
SMOOTHERS = ["jacobi", "l1"]
# (num_fine_smooth_sweeps, num_coarse_smooth_sweeps) of AFACX
FINE_COARSE = [(2, 1), (1, 2), (3, 2)]
# num_fine_smooth_sweeps of MULTADD, whose cycle never reads num_coarse
MULTADD_FINE = [2, 3]
WEIGHT = 0.8

MULTI_LEVEL = ["lin16", "box", "agg2"]
HIERARCHIES = MULTI_LEVEL + ["tri257"]
ROWS = {"lin16": [4096, 512, 64, 8], "box": [1680, 210, 18, 1], "agg2": [4096, 512], "tri257": [257]}

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def host(amg, oracle, name):
    """(L, {"A", "P", "R"}) of a named hierarchy as oracle.Csr"""
    def make():
        if name == "lin16":
            return pcg_ref.host_hierarchy(amg, oracle, 16)
        if name == "box":
            return pcg_ref.host_hierarchy(amg, oracle, (12, 10, 14))
        if name == "agg2":
            return pcg_ref.host_hierarchy(amg, oracle, 16, interp=amg.AMG_INTERP_AGGREGATE, levels=2)
        if name == "tri257":
            return pcg_ref.tridiag_hierarchy(oracle, 257)
        raise KeyError(name)
    return cached(("host", name), make)


def rows(name):
    return ROWS[name][0]


def rhs(amg, name):
    return cached(("f", name), lambda: amg.rhs_rand(0, rows(name)))


def guess(amg, name):
    """a nonzero first iterate, drawn apart from the right-hand side"""
    return cached(("u0", name), lambda: 0.25 * amg.rhs_rand(7, 7 + rows(name)))


def smoother_code(amg, smoother):
    return {"jacobi": amg.AMG_JACOBI, "l1": amg.AMG_L1_JACOBI, "hybrid": amg.AMG_HYBRID_JGS}[smoother]


def mult_opts(amg, smoother, pre, post, cycles, **kw):
    return amg.default_opts(**{"solver": amg.AMG_MULT, "smoother": smoother_code(amg, smoother),
                               "smooth_weight": WEIGHT, "num_pre_smooth_sweeps": pre, "num_post_smooth_sweeps": post,
                               "num_cycles": cycles, "tol": 0.0, "check_resnorm": 1, **kw})


def add_opts(amg, solver, smoother, fine, coarse, cycles, **kw):
    """sync AFACX, or sync MULTADD with the smoothed transfers composed"""
    sv = {"afacx": amg.AMG_AFACX, "multadd": amg.AMG_MULTADD}[solver]
    return amg.default_opts(**{"solver": sv, "smoother": smoother_code(amg, smoother), "smooth_weight": WEIGHT,
                               "num_fine_smooth_sweeps": fine, "num_coarse_smooth_sweeps": coarse,
                               "smooth_transfer": 1, "num_cycles": cycles, "tol": 0.0, "check_resnorm": 1, **kw})


def opts_key(o):
    """what the oracle's stationary solve depends on"""
    return (o.solver, o.smoother, o.num_pre_smooth_sweeps, o.num_post_smooth_sweeps, o.num_fine_smooth_sweeps,
            o.num_coarse_smooth_sweeps, o.smooth_weight, o.num_cycles, o.smooth_transfer, o.cheby_flag, o.cheby_mu,
            o.cheby_delta, max(o.num_threads, 1))


def oracle_hier(oracle, hier, opts):
    """pcg_ref.oracle_hier plus the Chebyshev options, which the stationary solve reads"""
    oo = oracle.make_opts(solver=opts.solver, smoother=opts.smoother, num_pre=opts.num_pre_smooth_sweeps,
                          num_post=opts.num_post_smooth_sweeps, num_fine=opts.num_fine_smooth_sweeps,
                          num_coarse=opts.num_coarse_smooth_sweeps, smooth_weight=opts.smooth_weight,
                          num_cycles=opts.num_cycles, tol=0.0, check_resnorm=1, cheby_flag=opts.cheby_flag,
                          cheby_mu=opts.cheby_mu, cheby_delta=opts.cheby_delta, num_threads=max(opts.num_threads, 1))
    OH = oracle.Hier(hier["A"], hier["P"], hier["R"], oo)
    if opts.smooth_transfer == 1 and opts.solver == oracle.OR_MULTADD:
        OH.set_composed_transfers()
    return OH


def oracle_solve(amg, oracle, name, opts, zero_guess=False):
    """(u, residual-norm history) of the oracle's SMEM_Solve under the device options, from
    guess(name) or from zero"""
    def make():
        _, hier = host(amg, oracle, name)
        u, hist, k = oracle_hier(oracle, hier, opts).solve(rhs(amg, name), None if zero_guess else guess(amg, name))
        assert k == opts.num_cycles
        return u, hist
    return cached(("solve", name, zero_guess) + opts_key(opts), make)


def oracle_pcg(amg, oracle, name, opts, iters):
    """pcg_ref.pcg_model from guess(name) with the device's dot product"""
    def make():
        _, hier = host(amg, oracle, name)
        return pcg_ref.pcg_model(oracle, hier, opts, rhs(amg, name), iters, pcg_ref.dev_dot, x0=guess(amg, name))
    return cached(("pcg", name, iters) + opts_key(opts), make)


def relres(hist):
    return hist[-1] / hist[0]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(np.all(a.view(np.uint64) == b.view(np.uint64)))
