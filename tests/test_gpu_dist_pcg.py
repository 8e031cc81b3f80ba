"""AMG-preconditioned conjugate gradients on the distributed hierarchy (amg_dist_pcg_*) on the
MI355X against the host model.

Ranks run as threads of this process over the host transport (dist.ThreadMailbox), each with
its own context on cuda:0, as in tests/test_gpu_dist.py; one rank also runs over RCCL.  The
recurrence is the single-GPU one (tests/test_gpu_pcg.py) with every dot product summed per rank
in amg_vec_dot's order and the rank values added in rank order, so the assembled iterate, the
recurrence residual and the alpha / beta / rho history are compared bit for bit with
pcg_ref.pcg_model under dist_pcg_ref.dist_dot of the partition the ranks report.  Norms pass
through a square root and are held to rtol 1e-12.

Not covered here: ranks as separate processes over RCCL.  The process launcher of
tests/test_gpu_slab_async_procs.py drives the asynchronous solve inside its rank function and
cannot run another solve without being edited.
"""
import numpy as np
import pytest

import dist_pcg_ref
import pcg_ref
from test_gpu_dist import row_parts, run_ranks
from test_gpu_kernels import assert_bitwise
from test_gpu_pcg import cached, case_opts

pytestmark = pytest.mark.gpu

ITERS = 6


def gen_host(amg, oracle, dims, interp="linear"):
    """(gen, L, host operators as oracle.Csr) of the structured problem, built once per shape"""
    def make():
        it = amg.AMG_INTERP_AGGREGATE if interp == "aggregate" else amg.AMG_INTERP_LINEAR
        g = amg.Gen(*dims, interp=it)
        host = {}
        for which, tag, cnt in ((amg.AMG_GEN_A, "A", g.L), (amg.AMG_GEN_P, "P", g.L - 1), (amg.AMG_GEN_R, "R", g.L - 1)):
            host[tag] = [oracle.Csr(*g.host_csr(which, l)) for l in range(cnt)]
        return g, g.L, host
    return cached(("dist_pcg_host", dims, interp), make)


def ranks(amg, nranks, make, body, rep=0, rccl=False, nstreams=2):
    """body(D, rank) on every rank of a fresh distributed hierarchy make(ctx, rank); results by rank"""
    hub = amg.dist.ThreadMailbox(nranks)

    def rank(r):
        c = amg.Context(0, nstreams=nstreams)
        tr = None
        if rccl:
            amg.dist.init_rccl(c, 1, 0, lambda b: b)
        else:
            tr = amg.dist.HostTransport(hub, r)
            amg.dist.init_host(c, nranks, r, tr)
        amg.dist.set_replicate_rows(c, rep)
        D = make(c, r)
        out = body(D, r)
        D.free()
        errs = c.device_errors()
        amg.dist.finalize(c)
        c.close()
        if tr is not None and tr.error is not None:
            raise tr.error
        assert errs == 0, f"rank {r}: device range-check flags {errs:#x}"
        return out

    return run_ranks(nranks, rank)


def structured(amg, gen, opts, slab=False):
    return lambda c, r: amg.dist.DistHier(c, gen, opts, slab=slab)


def drive(f, iters, x0=None, extra=None):
    """one iteration at a time: this rank's rows of x after every iteration, r at the end, the norms"""
    def body(D, r):
        sl = slice(D.row0, D.row0 + D.n0)
        hist = [D.pcg_start(f[sl], None if x0 is None else x0[sl])]
        xs = [D.pcg_get_x()]
        for _ in range(iters):
            D.pcg_iterate(1)
            xs.append(D.pcg_get_x())
            hist.append(D.pcg_resnorm())
        out = dict(row0=D.row0, n0=D.n0, xs=xs, hist=np.array(hist), r=D.pcg_get_r(), sc=D.pcg_scalars())
        if extra is not None:
            out["extra"] = extra(D)
        return out
    return body


def row_starts(res):
    rs = [t["row0"] for t in res] + [res[-1]["row0"] + res[-1]["n0"]]
    assert rs[0] == 0 and all(a <= b for a, b in zip(rs[:-1], rs[1:]))
    return rs


def check_model(res, run, iters, what):
    """every rank's drive() result against the model run, bit for bit (norms: rtol 1e-12)"""
    for k in range(iters + 1):
        assert_bitwise(np.concatenate([t["xs"][k] for t in res]), run.xs[k], f"{what}: x after iteration {k}")
    assert_bitwise(np.concatenate([t["r"] for t in res]), run.rs[iters], f"{what}: recurrence residual")
    for t in res:
        a, b, rho = t["sc"]
        assert len(a) == iters
        assert_bitwise(a, np.array(run.alpha), f"{what}: alpha")
        assert_bitwise(b, np.array(run.beta), f"{what}: beta")
        assert_bitwise(rho, np.array(run.rho), f"{what}: rho")
        np.testing.assert_array_equal(t["hist"], res[0]["hist"])  # every rank holds the same norms
    np.testing.assert_allclose(res[0]["hist"], run.hist, rtol=1e-12, atol=0)


def cut_parts(host, rs):
    """per rank: its rows (A, P, R) of the host operators with global columns, for row starts rs (L, nranks + 1)"""
    L = len(host["A"])

    def rows(M, a, b):
        lo, hi = M.rowptr[a], M.rowptr[b]
        return (b - a, M.rowptr[a:b + 1] - lo, M.col[lo:hi], M.val[lo:hi])

    return [([rows(host["A"][l], rs[l, r], rs[l, r + 1]) for l in range(L)],
             [rows(host["P"][l], rs[l, r], rs[l, r + 1]) for l in range(L - 1)],
             [rows(host["R"][l], rs[l + 1, r], rs[l + 1, r + 1]) for l in range(L - 1)])
            for r in range(rs.shape[1] - 1)]


def from_parts(amg, rs, parts, opts):
    return lambda c, r: amg.dist.DistHier.from_parts(c, rs, *parts[r], opts)


# ---- 1. the dot grid's edges on one level --------------------------------------------
@pytest.mark.parametrize("n,cuts", [(2306, [2049]), (513, [1, 256])])
def test_one_level_dot_edges(amg, oracle, n, cuts):
    """L = 1, A = tridiag(-1, 4, -1): local lengths 2049 | 257 (two workgroups and a tail of one row;
    one workgroup, one lane past a full stride) and 1 | 255 | 257"""
    L, host = pcg_ref.tridiag_hierarchy(oracle, n)
    rs = np.array([[0] + cuts + [n]], dtype=np.int64)
    opts = case_opts(amg, "mult_jacobi", num_cycles=ITERS)
    f = amg.rhs_rand(0, n)
    res = ranks(amg, len(cuts) + 1, from_parts(amg, rs, cut_parts(host, rs), opts), drive(f, ITERS))
    assert row_starts(res) == list(rs[0])
    assert [t["n0"] for t in res] == list(np.diff(rs[0]))
    run = dist_pcg_ref.dist_model(oracle, host, opts, f, ITERS, row_starts(res))
    check_model(res, run, ITERS, f"tridiag n={n}")


# ---- 2. multi-level, row form --------------------------------------------------------
@pytest.mark.parametrize("dims,interp,nranks,rep,name", [
    ((16, 16, 16), "linear", 2, 0, "mult_jacobi"),
    ((12, 10, 19), "linear", 3, 0, "mult_jacobi"),       # ragged planes
    ((16, 16, 16), "aggregate", 2, 0, "mult_jacobi"),    # smooth_weight 0.8
    ((16, 16, 16), "linear", 3, 512, "mult_l1"),
])
def test_multi_level_rows(amg, oracle, dims, interp, nranks, rep, name):
    gen, L, host = gen_host(amg, oracle, dims, interp)
    assert L >= 2
    opts = case_opts(amg, name, num_cycles=ITERS)
    assert opts.smooth_weight == 0.8
    f = amg.rhs_rand(0, dims[0] * dims[1] * dims[2])
    res = ranks(amg, nranks, structured(amg, gen, opts), drive(f, ITERS), rep=rep)
    run = dist_pcg_ref.dist_model(oracle, host, opts, f, ITERS, row_starts(res))
    check_model(res, run, ITERS, f"{dims} {interp} {name} x{nranks}")


# ---- 3. arbitrary partitions ---------------------------------------------------------
@pytest.mark.parametrize("cuts,rep", [((0.37,), 0), ((0.2, 0.5, 0.51), 0), ((0.6, 0.9), 4096)])
def test_any_partition(amg, oracle, cuts, rep):
    gen, L, host = gen_host(amg, oracle, (24, 20, 28))
    opts = case_opts(amg, "mult_jacobi", num_cycles=ITERS)
    f = amg.rhs_rand(0, 24 * 20 * 28)
    rs, parts = row_parts(amg, gen, cuts)
    res = ranks(amg, len(cuts) + 1, from_parts(amg, rs, parts, opts), drive(f, ITERS), rep=rep)
    assert row_starts(res) == list(rs[0])
    run = dist_pcg_ref.dist_model(oracle, host, opts, f, ITERS, row_starts(res))
    check_model(res, run, ITERS, f"cuts {cuts}")


# ---- 4. slab form --------------------------------------------------------------------
def test_slab_form(amg, oracle):
    """64^3 at 2 ranks: the smallest box tests/test_gpu_slab.py runs with the fused level-0 residual +
    restriction, which in preconditioner mode reads the outer residual's ghost planes"""
    gen, L, host = gen_host(amg, oracle, (64, 64, 64))
    opts = case_opts(amg, "mult_jacobi", num_cycles=ITERS)
    f = amg.rhs_rand(0, 64 ** 3)
    res = ranks(amg, 2, structured(amg, gen, opts, slab=True), drive(f, ITERS, extra=lambda D: D.slab_info()),
                rep=1 << 12)
    for t in res:
        Ld, geo, fused = t["extra"]
        assert Ld >= 1 and geo & 1 and fused == 1, t["extra"]
    run = dist_pcg_ref.dist_model(oracle, host, opts, f, ITERS, row_starts(res))
    check_model(res, run, ITERS, "slab 64^3")


# ---- 5. one rank is one GPU ----------------------------------------------------------
def single_gpu_pcg(amg, ctx, gen, opts, f, iters, name):
    def make():
        H = amg.build_hierarchy(ctx, gen, opts)
        fv, xv, out = ctx.vec(f), ctx.vec(np.zeros(f.size)), ctx.vec(f.size)
        hist = [H.pcg_start(fv, xv)]
        for _ in range(iters):
            H.pcg_iterate(1)
            hist.append(H.pcg_resnorm())
        H.pcg_get_x(out)
        x, sc = out.download(), H.pcg_scalars()
        H.free()
        for v in (fv, xv, out):
            v.free()
        return x, sc, np.array(hist)
    return cached(("single_gpu_pcg", name, f.size, iters), make)


@pytest.mark.parametrize("name,n", [("mult_jacobi", 24), ("mult_l1", 16)])
@pytest.mark.parametrize("rccl", [False, True])
def test_one_rank_is_one_gpu(amg, oracle, ctx, rccl, name, n):
    """x, alpha / beta / rho and the norms (the same kernel path: 0.0 + v is v) of Hier.pcg_*.  The two
    sides hand the fused zero-guess sweep different operands: the diagonal's one value (or a_ii) on one
    GPU, the owned rows' a_ii across ranks, the l1 norms under L1 Jacobi on both"""
    gen, L, host = gen_host(amg, oracle, (n, n, n))
    opts = case_opts(amg, name, num_cycles=ITERS)
    f = amg.rhs_rand(0, n ** 3)
    x1, sc1, h1 = single_gpu_pcg(amg, ctx, gen, opts, f, ITERS, name)
    (t,) = ranks(amg, 1, structured(amg, gen, opts), drive(f, ITERS), rccl=rccl)
    assert_bitwise(t["xs"][ITERS], x1, "x")
    for a, b, what in zip(t["sc"], sc1, ("alpha", "beta", "rho")):
        assert_bitwise(a, b, what)
    assert_bitwise(t["hist"], h1, "norm history")


# ---- 6. the preconditioner alone -----------------------------------------------------
@pytest.mark.parametrize("name", ["mult_jacobi", "mult_l1"])
def test_precond_apply_is_the_oracles(amg, oracle, name):
    gen, L, host = gen_host(amg, oracle, (16, 16, 16))
    opts = case_opts(amg, name, num_cycles=1)
    r = amg.rhs_rand(0, 16 ** 3)

    def body(D, rank):
        sl = slice(D.row0, D.row0 + D.n0)
        return D.precond_apply(r[sl]), D.precond_apply(r[sl])  # no state carried over

    res = ranks(amg, 2, structured(amg, gen, opts), body)
    z = np.concatenate([t[0] for t in res])
    assert_bitwise(z, pcg_ref.oracle_precond(oracle, host, opts)(r), f"M^-1 r ({name})")
    assert_bitwise(np.concatenate([t[1] for t in res]), z, "second application")


# ---- 7. both sides of the fused zero-guess sweep -------------------------------------
@pytest.mark.parametrize("pre", [0, 2])
def test_fused_sweep_condition(amg, oracle, pre):
    """num_pre_smooth_sweeps 0: no sweep to fuse (the cycle starts from the cleared u); 2: the fused
    zero-guess sweep, then a full one.  The default (1) is test_multi_level_rows"""
    gen, L, host = gen_host(amg, oracle, (16, 16, 16))
    opts = case_opts(amg, "mult_jacobi", num_cycles=ITERS, num_pre_smooth_sweeps=pre)
    f = amg.rhs_rand(0, 16 ** 3)
    res = ranks(amg, 2, structured(amg, gen, opts), drive(f, ITERS))
    run = dist_pcg_ref.dist_model(oracle, host, opts, f, ITERS, row_starts(res))
    check_model(res, run, ITERS, f"{pre} pre-sweeps")


# ---- 8. split and one-shot; who owns the state ---------------------------------------
def test_split_and_one_shot_agree(amg, oracle):
    gen, L, host = gen_host(amg, oracle, (16, 16, 16))
    opts = case_opts(amg, "mult_jacobi", num_cycles=6, check_resnorm=0)
    f = amg.rhs_rand(0, 16 ** 3)
    x0 = 0.25 * amg.rhs_rand(7, 7 + 16 ** 3)

    def body(D, rank):
        sl = slice(D.row0, D.row0 + D.n0)
        x_one, h_one, k = D.pcg_solve(f[sl], x0[sl])
        assert k == 6 and len(h_one) == 7

        def split(parts):
            r0 = D.pcg_start(f[sl], x0[sl])
            for p in parts:
                D.pcg_iterate(p)
            return D.pcg_get_x(), r0, D.pcg_resnorm(), D.pcg_scalars()

        x24, r0, rn24, sc24 = split([2, 4])
        x6, _, rn6, sc6 = split([6])  # a second start on the same D is fresh
        assert_bitwise(x24, x_one, "start + iterate(2) + iterate(4) against pcg_solve")
        assert_bitwise(x6, x24, "a second start")
        assert r0 == h_one[0] and rn24 == h_one[-1] and rn6 == rn24
        for a, b in zip(sc24, sc6):
            assert_bitwise(a, b, "scalar history")
        assert np.all(h_one[1:] > 0) and h_one[-1] < h_one[0]
        # a stationary solve takes r0 and lv[0].u over: the PCG state ends, and the other way round
        D.solve_start(f[sl])
        with pytest.raises(amg.AmgError):
            D.pcg_iterate(1)
        with pytest.raises(amg.AmgError):
            D.pcg_get_x()
        D.iterate(1)
        D.pcg_start(f[sl], x0[sl])
        with pytest.raises(amg.AmgError):
            D.iterate(1)
        D.pcg_iterate(6)
        assert_bitwise(D.pcg_get_x(), x_one, "a start after a stationary solve")
        return D.row0, x_one, h_one

    res = ranks(amg, 2, structured(amg, gen, opts), body)
    np.testing.assert_array_equal(res[0][2], res[1][2])
    rs = [res[0][0], res[1][0], 16 ** 3]
    run = dist_pcg_ref.dist_model(oracle, host, opts, f, 6, rs, x0=x0)
    assert_bitwise(np.concatenate([t[1] for t in res]), run.xs[6], "pcg_solve from x0 against the model")
    np.testing.assert_allclose(res[0][2], run.hist, rtol=1e-12, atol=0)


# ---- 9. the stop on tolerance --------------------------------------------------------
def test_stops_on_tolerance(amg, oracle):
    gen, L, host = gen_host(amg, oracle, (16, 16, 16))
    cap, tol = 30, 1e-6
    opts = case_opts(amg, "mult_jacobi", num_cycles=cap, tol=tol, check_resnorm=1)
    f = amg.rhs_rand(0, 16 ** 3)

    def body(D, rank):
        x, hist, k = D.pcg_solve(f[D.row0:D.row0 + D.n0])
        return D.row0, x, hist, k

    res = ranks(amg, 2, structured(amg, gen, opts), body)
    ks = [t[3] for t in res]
    assert ks[0] == ks[1], ks  # every rank stops at the same iteration
    run = dist_pcg_ref.dist_model(oracle, host, opts, f, cap, [res[0][0], res[1][0], 16 ** 3])
    rel = run.hist / run.hist[0]
    k_model = int(np.argmax(rel < tol))
    assert 0 < k_model < cap
    # the decision is not a matter of the last bits (the norms are compared at rtol 1e-12)
    for k in (k_model - 1, k_model):
        assert abs(rel[k] - tol) > 1e-9 * tol, (k, rel[k])
    assert ks[0] == k_model
    for t in res:
        hist = t[2]
        assert len(hist) == k_model + 1
        assert hist[-1] / hist[0] < tol <= hist[-2] / hist[0]
        np.testing.assert_array_equal(hist, res[0][2])
    assert_bitwise(np.concatenate([t[1] for t in res]), run.xs[k_model], "iterate at the stop")
    np.testing.assert_allclose(res[0][2], run.hist[:k_model + 1], rtol=1e-12, atol=0)


# ---- 10. zero right-hand side --------------------------------------------------------
def test_zero_right_hand_side(amg, oracle):
    gen, L, host = gen_host(amg, oracle, (16, 16, 16))
    opts = case_opts(amg, "mult_jacobi", num_cycles=4, check_resnorm=1)

    def body(D, rank):
        x, hist, k = D.pcg_solve(np.zeros(D.n0))  # x0 = 0
        a, b, rho = D.pcg_scalars()
        assert k == 4 and len(a) == 4
        assert np.array_equal(x.view(np.uint64), np.zeros(D.n0).view(np.uint64))  # x stays x0 bit for bit
        assert np.array_equal(hist, np.zeros(5))
        for s in (a, b, rho):
            assert np.all(np.isfinite(s)) and np.all(s == 0.0)
        return True

    assert all(ranks(amg, 2, structured(amg, gen, opts), body))


# ---- 11. refusals --------------------------------------------------------------------
@pytest.mark.parametrize("what", ["async_multadd", "richardson"])
def test_refused_before_any_collective(amg, oracle, what):
    """every rank gets AmgError and returns: the check precedes every collective, so nobody waits
    (a rank left waiting would run into the mailbox's time limit and fail the test)"""
    gen, L, host = gen_host(amg, oracle, (16, 16, 16))
    if what == "async_multadd":
        opts = amg.default_opts(solver=amg.AMG_ASYNC_MULTADD, smooth_weight=0.8, num_cycles=3, tol=0.0)
    else:
        opts = amg.default_opts(smooth_weight=0.8, num_cycles=3, tol=0.0, accel_type=amg.AMG_RICHARD_ACCEL,
                                cheby_mu=1.5, cheby_delta=0.5)
    f = amg.rhs_rand(0, 16 ** 3)

    def body(D, rank):
        fl = f[D.row0:D.row0 + D.n0]
        for call in (lambda: D.pcg_start(fl), lambda: D.pcg_solve(fl), lambda: D.precond_apply(fl)):
            with pytest.raises(amg.AmgError):
                call()
        with pytest.raises(amg.AmgError):
            D.pcg_iterate(1)  # no state was created
        return True

    assert all(ranks(amg, 2, structured(amg, gen, opts), body, nstreams=gen.L + 2))


# ---- 12. it converges faster than the stationary iteration ---------------------------
def test_beats_the_stationary_cycle(amg, oracle):
    gen, L, host = gen_host(amg, oracle, (24, 24, 24))
    opts = case_opts(amg, "mult_jacobi", num_cycles=8)
    f = amg.rhs_rand(0, 24 ** 3)

    def body(D, rank):
        fl = f[D.row0:D.row0 + D.n0]
        r0 = D.pcg_start(fl)
        D.pcg_iterate(8)
        pcg = D.pcg_resnorm()
        s0 = D.solve_start(fl)
        D.iterate(8)
        return r0, pcg, s0, D.resnorm()

    res = ranks(amg, 2, structured(amg, gen, opts), body)
    r0, pcg, s0, stat = res[0]
    print(f"relres after 8: PCG {pcg / r0:.3e}, stationary {stat / s0:.3e}")
    np.testing.assert_allclose(r0, s0, rtol=1e-12, atol=0)  # both start from x = 0
    assert pcg < stat
