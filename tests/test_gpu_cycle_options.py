"""The cycles above the kernels on the MI355X across their option space: sweep
counts, entry points and option changes on a live hierarchy.

vcycle / smooth_one_level / outer_residual / pcg_precond (amg_solver.cpp) and
their restatement for multivectors (amg_mrhs.cpp: cycle) are a small state
machine (zero_flag, zero_done, pre_ready, post_deferred, r0_stale, store_u1, the
u / u_alt swaps) gated on the sweep counts, the smoother, reuse_outer_residual,
L > 1 and the fused forms a hierarchy admits.  A wrong gate gives a convergent
wrong iterate, so every case here is held to the oracle bit for bit (iterates,
PCG scalars) and to rtol 1e-12 (residual-norm histories, whose summation order
differs); cycle_cases.py is the table, test_cycle_cases.py shows on the host that
its entries tell the counts apart.
"""
import ctypes as C

import numpy as np
import pytest

import cycle_cases as cc
import pcg_ref
from test_gpu_configs import free_hier, host_levels
from test_gpu_kernels import assert_bitwise
from test_gpu_pcg import check_run

pytestmark = pytest.mark.gpu

CYCLES = 4
ITERS = 6
PCG_PAIRS = [(0, 1), (1, 0), (2, 1), (2, 2)]
PRECOND_SWEEPS = [p for p in cc.SWEEPS if sum(p) > 0]
PRECOND_HIERS = ["lin16", "agg2", "tri257"]


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def device(amg, oracle, ctx, name, opts):
    return pcg_ref.device_hier(amg, ctx, cc.host(amg, oracle, name)[1], opts)


def run(amg, ctx, H, fn, f, x0):
    """amg_solve or amg_pcg_solve on host arrays: (iterate, history, steps done)"""
    fv, xv = ctx.vec(f), ctx.vec(x0)
    hist, k = np.zeros(H.opts.num_cycles + 1), C.c_int()
    amg.check(fn(H.h, fv.h, xv.h, _dp(hist), C.byref(k)))
    x = xv.download()
    fv.free()
    xv.free()
    return x, hist[:k.value + 1], k.value


def outer_residual(amg, H):
    v = H.vec(amg.AMG_VEC_R, 0)
    r = v.download()
    v.free()
    return r


def check_solve(amg, oracle, ctx, H, name, opts, what, hier=None, f=None, u0=None, ref=None):
    """amg_solve under opts on H: iterate bitwise the oracle's, history within rtol 1e-12, and
    amg_hier_vec(R, 0) bitwise the oracle's residual of that iterate; returns (u, history)"""
    hier = cc.host(amg, oracle, name)[1] if hier is None else hier
    f = cc.rhs(amg, name) if f is None else f
    u0 = cc.guess(amg, name) if u0 is None else u0
    u_c, h_c = cc.oracle_solve(amg, oracle, name, opts) if ref is None else ref
    u, h, k = run(amg, ctx, H, amg.lib.amg_solve, f, u0)
    assert k == opts.num_cycles
    assert_bitwise(u, u_c, f"{what}: iterate")
    np.testing.assert_allclose(h, h_c, rtol=1e-12, atol=0, err_msg=what)
    A0 = hier["A"][0]
    rr = oracle.smem_spgemv(A0, u, f, -1.0, 1.0, np.zeros(A0.nrows))
    assert_bitwise(outer_residual(amg, H), rr, f"{what}: outer residual")
    return u, h


# ---- a. the stationary multiplicative solve ------------------------------------------------
@pytest.mark.parametrize("smoother", cc.SMOOTHERS)
@pytest.mark.parametrize("name", cc.HIERARCHIES)
def test_mult_solve(amg, oracle, ctx, name, smoother):
    """every sweep pair, from a nonzero guess; on lin16 with the outer residual separate (0), fused
    into the next cycle's first sweep (1) and not stored (2)"""
    for pre, post in cc.SWEEPS:
        for reuse in ((0, 1, 2) if name == "lin16" else (0,)):
            opts = cc.mult_opts(amg, smoother, pre, post, CYCLES, reuse_outer_residual=reuse)
            H = device(amg, oracle, ctx, name, opts)
            check_solve(amg, oracle, ctx, H, name, opts, f"{name} {smoother} V({pre},{post}) reuse {reuse}")
            free_hier(H)
    assert ctx.device_errors() == 0


@pytest.mark.parametrize("pre,post", [(2, 1), (0, 1)])
def test_mult_solve_hybrid_jgs(amg, oracle, ctx, pre, post):
    opts = cc.mult_opts(amg, "hybrid", pre, post, CYCLES, num_threads=4)
    H = device(amg, oracle, ctx, "lin16", opts)
    check_solve(amg, oracle, ctx, H, "lin16", opts, f"hybrid JGS V({pre},{post})")
    free_hier(H)


# ---- b. the fused forms behind a pre-smoothing other than one sweep ----------------------
# form -> (box, planes per chunk, the context knob that switches it on)
FORMS = {
    "outer1": ((512, 8, 6), 4, ("fuse_outer", 1)),
    "outer2": ((512, 8, 6), 4, ("fuse_outer", 2)),
    "slab": ((512, 8, 6), 4, ("fuse_outer", 3)),
    "restrict": ((64, 16, 8), 16, None),
    "prolong": ((64, 16, 8), 16, ("fuse_prolong", 2)),
}
FORM_CASES = [(f, sm) for f in FORMS for sm in cc.SMOOTHERS]


def box_setup(amg, oracle, dims):
    """(generator, host levels, f) of a box, kept for the module"""
    def make():
        g = amg.Gen(*dims, interp=amg.AMG_INTERP_LINEAR)
        return g, host_levels(amg, oracle, g), amg.rhs_rand(0, dims[0] * dims[1] * dims[2])
    return cc.cached(("box", dims), make)


@pytest.fixture(scope="module", autouse=True)
def release_generators():
    yield
    for key in [k for k in cc._CACHE if isinstance(k, tuple) and k[0] == "box"]:
        cc._CACHE.pop(key)[0].free()


def box_oracle(amg, oracle, dims, opts):
    def make():
        _, hier, f = box_setup(amg, oracle, dims)
        u, hist, k = cc.oracle_hier(oracle, hier, opts).solve(f)
        assert k == opts.num_cycles
        return u, hist
    return cc.cached(("box solve", dims) + cc.opts_key(opts), make)


class knobs:
    """the context's form switches for one block, put back after it"""

    def __init__(self, ctx, zc, knob):
        self.ctx, self.zc, self.knob = ctx, zc, knob

    def __enter__(self):
        self.ctx.set_plane_march(1, self.zc, 1)
        if self.knob:
            getattr(self.ctx, "set_" + self.knob[0])(self.knob[1])

    def __exit__(self, *exc):
        self.ctx.set_plane_march(1, -1, 1)
        if self.knob:
            getattr(self.ctx, "set_" + self.knob[0])(0)


def expected_fused_outer(form, smoother, pre, post, reuse):
    """fused_outer_applies: reuse_applies (pre > 0, reuse on) with a post sweep to defer; the
    register marches (1, 2) are plain Jacobi only, the slab form takes L1 Jacobi as well"""
    mode = {"outer1": 1, "outer2": 2, "slab": 3}.get(form, 0)
    on = mode and pre > 0 and post >= 1 and reuse > 0 and (smoother == "jacobi" or mode == 3)
    return mode if on else 0


@pytest.mark.parametrize("pre", [0, 2, 3])
@pytest.mark.parametrize("form,smoother", FORM_CASES)
def test_fused_forms(amg, oracle, ctx, form, smoother, pre):
    """hierarchies built as the benchmark builds them (amg.build_hierarchy), so the forms are the
    ones it runs; each form is reported active exactly when its gate says so (off at pre = 0 for the
    deferred post sweep), and the iterate and history are the oracle's either way"""
    dims, zc, knob = FORMS[form]
    g, hier, f = box_setup(amg, oracle, dims)
    u0 = np.zeros(len(f))
    for post in (1, 2):
        for reuse in (1, 2):
            opts = cc.mult_opts(amg, smoother, pre, post, CYCLES, reuse_outer_residual=reuse)
            with knobs(ctx, zc, knob):
                H = amg.build_hierarchy(ctx, g, opts)
                what = f"{form} {smoother} V({pre},{post}) reuse {reuse}"
                assert H.fused_outer == expected_fused_outer(form, smoother, pre, post, reuse), what
                if dims[0] == 64:
                    # detect_geo looks at the operators alone: level 0's residual + restriction
                    # fused and geometric transfers whatever the sweep counts
                    assert H.fused & 3 == 3, (what, H.fused)
                    assert (H.fused_prolong & 1) == (1 if form == "prolong" else 0), (what, H.fused_prolong)
                check_solve(amg, oracle, ctx, H, None, opts, what, hier=hier, f=f, u0=u0,
                            ref=box_oracle(amg, oracle, dims, opts))
                free_hier(H)
    assert ctx.device_errors() == 0


# ---- c. the solve driven in parts ---------------------------------------------------------------
SPLITS = [[1, 1, 1, 1, 1, 1], [6], [2, 4], [5, 1]]


def check_splits(amg, ctx, H, f, u0, after, splits, what):
    """after[k]: the oracle's iterate after k cycles.  The one-shot history first, then every
    split: get_u after each part bitwise after[cycles so far], resnorm bitwise the history's entry"""
    total = sum(splits[0])
    _, h_one, k = run(amg, ctx, H, amg.lib.amg_solve, f, u0)
    assert k == total
    fv, uv, out = ctx.vec(f), ctx.vec(u0), ctx.vec(len(f))
    for parts in splits:
        assert H.solve_start(fv, uv) == h_one[0]
        done = 0
        for p in parts:
            H.iterate(p)
            done += p
            H.get_u(out)
            assert_bitwise(out.download(), after[done], f"{what}: split {parts}, iterate after {done} cycles")
            assert H.resnorm() == h_one[done], f"{what}: split {parts}, norm after {done} cycles"
    for v in (fv, uv, out):
        v.free()


@pytest.mark.parametrize("smoother", cc.SMOOTHERS)
@pytest.mark.parametrize("pre,post", [(2, 1), (0, 1)])
def test_split_driving(amg, oracle, ctx, pre, post, smoother):
    total = sum(SPLITS[0])
    after = {k: cc.oracle_solve(amg, oracle, "lin16", cc.mult_opts(amg, smoother, pre, post, k))[0]
             for k in range(1, total + 1)}
    for reuse in (0, 2):
        opts = cc.mult_opts(amg, smoother, pre, post, total, reuse_outer_residual=reuse)
        H = device(amg, oracle, ctx, "lin16", opts)
        check_splits(amg, ctx, H, cc.rhs(amg, "lin16"), cc.guess(amg, "lin16"), after, SPLITS,
                     f"{smoother} V({pre},{post}) reuse {reuse}")
        free_hier(H)


def test_split_driving_fused_outer(amg, oracle, ctx):
    """fuse_outer 2 writes the deferred sweep's u' only in a batch's last step (store_u1): what
    get_u shows after each batch is still the oracle's iterate"""
    dims, zc, knob = FORMS["outer2"]
    g, hier, f = box_setup(amg, oracle, dims)
    after = {k: box_oracle(amg, oracle, dims, cc.mult_opts(amg, "jacobi", 2, 1, k))[0] for k in (3, 6)}
    opts = cc.mult_opts(amg, "jacobi", 2, 1, 6, reuse_outer_residual=2)
    with knobs(ctx, zc, knob):
        H = amg.build_hierarchy(ctx, g, opts)
        assert H.fused_outer == 2
        check_splits(amg, ctx, H, f, np.zeros(len(f)), after, [[3, 3]], "fuse_outer 2 V(2,1)")
        free_hier(H)


# ---- d. preconditioner mode ---------------------------------------------------------------------
@pytest.mark.parametrize("smoother", cc.SMOOTHERS)
@pytest.mark.parametrize("name", PRECOND_HIERS)
def test_precond_apply(amg, oracle, ctx, name, smoother):
    r = cc.rhs(amg, name)
    for pre, post in PRECOND_SWEEPS:
        opts = cc.mult_opts(amg, smoother, pre, post, 1)
        H = device(amg, oracle, ctx, name, opts)
        z = H.precond_apply(r)
        z2 = H.precond_apply(r)
        free_hier(H)
        z_c = pcg_ref.oracle_precond(oracle, cc.host(amg, oracle, name)[1], opts)(r)
        assert_bitwise(z, z_c, f"{name} {smoother} V({pre},{post}): M^-1 r")
        assert_bitwise(z2, z_c, f"{name} {smoother} V({pre},{post}): second application")


@pytest.mark.parametrize("smoother", cc.SMOOTHERS)
@pytest.mark.parametrize("name", PRECOND_HIERS)
def test_pcg(amg, oracle, ctx, name, smoother):
    """both sides of pcg_fuse_zero: with a pre sweep the residual update writes level 0's zero-guess
    sweep, without one the cycle clears u itself"""
    for pre, post in PCG_PAIRS:
        opts = cc.mult_opts(amg, smoother, pre, post, ITERS)
        model = cc.oracle_pcg(amg, oracle, name, opts, ITERS)
        H = device(amg, oracle, ctx, name, opts)
        check_run(amg, H, ctx, cc.rhs(amg, name), model, ITERS, f"{name} {smoother} V({pre},{post})")
        free_hier(H)


def test_eigs_power(amg, oracle, ctx):
    opts = cc.mult_opts(amg, "jacobi", 2, 1, 1)
    emax_c, emin_c = cc.oracle_hier(oracle, cc.host(amg, oracle, "lin16")[1], opts).eigs_power(10)
    H = device(amg, oracle, ctx, "lin16", opts)
    emax_g, emin_g = H.eigs_power(10)
    free_hier(H)
    assert abs(emax_g - emax_c) <= 1e-10 * abs(emax_c)
    assert abs(emin_g - emin_c) <= 1e-8 * abs(emax_c)


# ---- e. multivectors ----------------------------------------------------------------------------
def columns(amg, name, count):
    """count right-hand sides and guesses, each column drawn apart from the others"""
    n = cc.rows(name)
    return ([amg.rhs_rand(100 * j, 100 * j + n) for j in range(count)],
            [0.25 * amg.rhs_rand(100 * j + 50, 100 * j + 50 + n) for j in range(count)])


def check_mrhs(amg, ctx, H, name, opts, count, what):
    """column j of amg_mrhs_precond_apply, amg_mrhs_solve (CYCLES cycles) and amg_mrhs_pcg_solve
    (ITERS iterations) against the single-vector entry point on column j"""
    fs, u0 = columns(amg, name, count)
    z = H.mrhs_precond_apply(fs)
    for j in range(count):
        assert_bitwise(z[j], H.precond_apply(fs[j]), f"{what}: M^-1 r, column {j}")
    us, hist, done = H.mrhs_solve(fs, u0)
    assert done == CYCLES and hist.shape == (CYCLES + 1, count)
    for j in range(count):
        u, h, k = run(amg, ctx, H, amg.lib.amg_solve, fs[j], u0[j])
        assert k == CYCLES
        assert_bitwise(us[j], u, f"{what}: iterate, column {j}")
        np.testing.assert_allclose(hist[:, j], h, rtol=1e-12, atol=0, err_msg=what)
    opts.num_cycles = ITERS
    H.set_opts(opts)
    xs, hist, done = H.mrhs_pcg_solve(fs, u0)
    assert done == ITERS and hist.shape == (ITERS + 1, count)
    for j in range(count):
        x, h, k = run(amg, ctx, H, amg.lib.amg_pcg_solve, fs[j], u0[j])
        assert k == ITERS
        assert_bitwise(xs[j], x, f"{what}: x, column {j}")
        for tag, a, b in zip(("alpha", "beta", "rho"), H.mrhs_pcg_scalars(j), H.pcg_scalars()):
            assert len(a) == ITERS
            assert_bitwise(a, b, f"{what}: {tag}, column {j}")
        np.testing.assert_allclose(hist[:, j], h, rtol=1e-12, atol=0, err_msg=what)


@pytest.mark.parametrize("smoother", cc.SMOOTHERS)
@pytest.mark.parametrize("name", PRECOND_HIERS)
def test_mrhs(amg, oracle, ctx, name, smoother):
    """amg_mrhs.cpp restates the cycle by hand: 4 columns under every sweep pair (no sweeps at all
    among them), on tri257 the one-level cycle in solve mode too"""
    for pre, post in cc.SWEEPS:
        opts = cc.mult_opts(amg, smoother, pre, post, CYCLES)
        H = device(amg, oracle, ctx, name, opts)
        check_mrhs(amg, ctx, H, name, opts, 4, f"{name} {smoother} V({pre},{post}) k=4")
        free_hier(H)
    assert ctx.device_errors() == 0


@pytest.mark.parametrize("count,pre,post", [(2, 2, 1), (8, 0, 2)])
def test_mrhs_widths(amg, oracle, ctx, count, pre, post):
    opts = cc.mult_opts(amg, "jacobi", pre, post, CYCLES)
    H = device(amg, oracle, ctx, "lin16", opts)
    check_mrhs(amg, ctx, H, "lin16", opts, count, f"lin16 jacobi V({pre},{post}) k={count}")
    free_hier(H)


# ---- f. the additive cycles ----------------------------------------------------------------------
@pytest.mark.parametrize("smoother", cc.SMOOTHERS)
@pytest.mark.parametrize("name", ["lin16", "box"])
def test_additive_sweeps(amg, oracle, ctx, name, smoother):
    """num_fine / num_coarse of sync AFACX and num_fine of sync MULTADD with the smoothed transfers
    composed (the zero-sweep gating of the composed transfers is test_gpu_async.py's)"""
    cases = [("afacx", f, c) for f, c in cc.FINE_COARSE] + [("multadd", f, 1) for f in cc.MULTADD_FINE]
    for solver, fine, coarse in cases:
        opts = cc.add_opts(amg, solver, smoother, fine, coarse, 6)
        H = device(amg, oracle, ctx, name, opts)
        check_solve(amg, oracle, ctx, H, name, opts, f"{name} {smoother} {solver} fine {fine} coarse {coarse}")
        free_hier(H)
    assert ctx.device_errors() == 0


# ---- g. option changes on a live hierarchy -----------------------------------------------------
def check_chain(amg, oracle, ctx, chain, what, extra=None):
    """create with chain[0] and solve; then set_opts to each following entry and solve: the oracle's
    bits under that entry's options, which are also those of a hierarchy created with them (extra:
    further entry points compared between the two hierarchies)"""
    H = device(amg, oracle, ctx, "lin16", chain[0])
    check_solve(amg, oracle, ctx, H, "lin16", chain[0], f"{what}: created")
    for step, opts in enumerate(chain[1:], 1):
        H.set_opts(opts)
        u, h = check_solve(amg, oracle, ctx, H, "lin16", opts, f"{what}: after change {step}")
        F = device(amg, oracle, ctx, "lin16", opts)
        u_f, h_f = check_solve(amg, oracle, ctx, F, "lin16", opts, f"{what}: created as change {step}")
        assert_bitwise(u, u_f, f"{what}: change {step} against a fresh hierarchy")
        assert_bitwise(h, h_f, f"{what}: change {step}, history against a fresh hierarchy")
        if extra:
            extra(H, F, opts, f"{what}: change {step}")
        free_hier(F)
    free_hier(H)


def chains(amg, oracle):
    m = lambda sm, pre=1, post=1, **kw: cc.mult_opts(amg, sm, pre, post, CYCLES, **kw)  # noqa: E731
    base = cc.mult_opts(amg, "jacobi", 1, 1, 10)
    emax, emin = cc.cached("eigs lin16", lambda: cc.oracle_hier(oracle, cc.host(amg, oracle, "lin16")[1],
                                                                  base).eigs_power(20))
    cheby = dict(cheby_flag=1, cheby_mu=(emax + emin) / (emax - emin), cheby_delta=2.0 / (emax + emin))
    return {
        "weight jacobi": [m("jacobi"), m("jacobi", smooth_weight=0.6)],
        "weight hybrid": [m("hybrid", num_threads=4), m("hybrid", num_threads=4, smooth_weight=0.6)],
        "smoother": [m("jacobi"), m("l1"), m("jacobi")],
        "threads hybrid": [m("hybrid", num_threads=4), m("hybrid", num_threads=8)],
        "sweeps": [m("jacobi", 1, 1), m("jacobi", 2, 1), m("jacobi", 0, 1)],
        "reuse": [m("jacobi", reuse_outer_residual=2), m("jacobi", reuse_outer_residual=0),
                  m("jacobi", reuse_outer_residual=2)],
        "cheby": [m("jacobi"), m("jacobi", **cheby)],
        "additive": [cc.add_opts(amg, "afacx", "jacobi", 1, 1, CYCLES), cc.add_opts(amg, "multadd", "jacobi", 1, 1, CYCLES)],
    }


@pytest.mark.parametrize("which", ["weight jacobi", "weight hybrid", "smoother", "threads hybrid", "sweeps", "reuse",
                                   "cheby", "additive"])
def test_set_opts(amg, oracle, ctx, which):
    check_chain(amg, oracle, ctx, chains(amg, oracle)[which], which)
    assert ctx.device_errors() == 0


def bpx_opts(amg, **kw):
    return amg.default_opts(**{"solver": amg.AMG_BPX, "smoother": amg.AMG_JACOBI, "smooth_weight": 0.6,
                               "num_cycles": CYCLES, "tol": 0.0, "check_resnorm": 1, **kw})


def test_set_opts_mult_to_bpx_and_back(amg, oracle, ctx):
    """a hierarchy created as MULT has no level-0 correction vectors for BPX; amg_hier_set_opts
    allocates them, and solve, precond_apply and pcg_solve then match a hierarchy created as BPX"""
    f, x0 = cc.rhs(amg, "lin16"), cc.guess(amg, "lin16")

    def extra(H, F, opts, what):
        assert_bitwise(H.precond_apply(f), F.precond_apply(f), f"{what}: M^-1 r")
        x, h, k = run(amg, ctx, H, amg.lib.amg_pcg_solve, f, x0)
        x_f, h_f, k_f = run(amg, ctx, F, amg.lib.amg_pcg_solve, f, x0)
        assert k == k_f == CYCLES
        assert_bitwise(x, x_f, f"{what}: PCG x")
        assert_bitwise(h, h_f, f"{what}: PCG history")
        for a, b in zip(H.pcg_scalars(), F.pcg_scalars()):
            assert_bitwise(a, b, f"{what}: PCG scalars")

    mult = cc.mult_opts(amg, "jacobi", 1, 1, CYCLES, smooth_weight=0.6)
    check_chain(amg, oracle, ctx, [mult, bpx_opts(amg), mult, bpx_opts(amg, num_pre_smooth_sweeps=2)], "MULT <-> BPX",
                extra)
    assert ctx.device_errors() == 0


def test_set_opts_refuses_the_other_family(amg, oracle, ctx):
    mult = cc.mult_opts(amg, "jacobi", 1, 1, CYCLES)
    H = device(amg, oracle, ctx, "lin16", mult)
    with pytest.raises(amg.AmgError) as err:
        H.set_opts(cc.add_opts(amg, "multadd", "jacobi", 1, 1, CYCLES))
    assert "ONE_LEVEL" in str(err.value) and "ALL_LEVELS" in str(err.value)
    assert H.opts is mult
    check_solve(amg, oracle, ctx, H, "lin16", mult, "after the refused change")
    free_hier(H)


def test_set_opts_ends_a_running_solve(amg, oracle, ctx):
    """the sweep the last outer residual prepared belongs to the old weight: iterate asks for a new start"""
    opts = cc.mult_opts(amg, "jacobi", 1, 1, CYCLES, reuse_outer_residual=2)
    H = device(amg, oracle, ctx, "lin16", opts)
    fv, uv = ctx.vec(cc.rhs(amg, "lin16")), ctx.vec(cc.guess(amg, "lin16"))
    H.solve_start(fv, uv)
    H.iterate(2)
    H.set_opts(cc.mult_opts(amg, "jacobi", 1, 1, CYCLES, reuse_outer_residual=2, smooth_weight=0.6))
    with pytest.raises(amg.AmgError):
        H.iterate(1)
    fv.free()
    uv.free()
    free_hier(H)
