"""Multi-rank solve phase on the MI355X: slab-distributed V-cycle vs one GPU.

Several ranks run as threads of this one process, each with its own context
(compute + communication streams) on cuda:0, exchanging ghost rows, the
replicated-level right-hand side and norms through ``dist.ThreadMailbox``
(the host transport; RCCL refuses two ranks on one device, and the
ring/xGMI path is exercised by bench.py --gpus N).  The distributed cycle
keeps every row sum in the single-GPU order, so the assembled iterate must be
BIT-IDENTICAL to the single-GPU SMEM_Solve iterate (which the solve tests pin
to the oracle); residual norms are sums over ranks, compared at rtol 1e-12.
"""
import threading

import numpy as np
import pytest

from async_band import race_tables

from test_gpu_kernels import assert_bitwise

pytestmark = pytest.mark.gpu


def run_ranks(nranks, fn):
    out, errs = [None] * nranks, []

    def body(r):
        try:
            out[r] = fn(r)
        except BaseException as e:  # noqa: BLE001
            errs.append((r, e))

    th = [threading.Thread(target=body, args=(r,)) for r in range(nranks)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    assert not errs, errs
    return out


def single_gpu(amg, ctx, gen, opts, f, cycles):
    H = amg.build_hierarchy(ctx, gen, opts)
    fv, uv = ctx.vec(f), ctx.vec(np.zeros(f.size))
    r0 = H.solve_start(fv, uv)
    hist = [r0]
    for _ in range(cycles):
        H.iterate(1)
        hist.append(H.resnorm())
    out = ctx.vec(f.size)
    H.get_u(out)
    u = out.download()
    H.free()
    return u, np.array(hist)


def distributed(amg, gen, opts, f, cycles, nranks, replicate_rows):
    hub = amg.dist.ThreadMailbox(nranks)

    def rank(r):
        ctx = amg.Context(0, nstreams=2)
        tr = amg.dist.HostTransport(hub, r)
        amg.dist.init_host(ctx, nranks, r, tr)
        amg.dist.set_replicate_rows(ctx, replicate_rows)
        D = amg.dist.DistHier(ctx, gen, opts)
        r0 = D.solve_start(f[D.row0:D.row0 + D.n0])
        hist = [r0]
        for _ in range(cycles):
            D.iterate(1)
            hist.append(D.resnorm())
        u = D.get_u()
        row0 = D.row0
        D.free()
        amg.dist.finalize(ctx)
        ctx.close()
        if tr.error is not None:
            raise tr.error
        return row0, u, np.array(hist)

    res = run_ranks(nranks, rank)
    res.sort(key=lambda t: t[0])
    u = np.concatenate([t[1] for t in res])
    for t in res[1:]:
        np.testing.assert_array_equal(t[2], res[0][2])  # every rank sees the same norms
    return u, res[0][2]


CASES = [
    # (dims, interp, nranks, replicate_rows, opts)
    ((32, 32, 32), "linear", 2, 1 << 18, {}),          # fine level distributed only
    ((32, 32, 32), "linear", 2, 0, {}),                # all but the coarsest distributed
    ((32, 32, 32), "linear", 4, 0, {}),                # empty slabs on coarse levels
    ((24, 20, 37), "linear", 3, 0, {}),                # ragged planes per rank
    ((16, 16, 16), "aggregate", 2, 0, {"smooth_weight": 0.8}),
    ((32, 32, 32), "linear", 3, 512, {"smoother": "l1"}),
    ((32, 32, 32), "linear", 2, 0, {"reuse_outer_residual": 0}),
    ((20, 24, 40), "linear", 4, 0, {"num_pre_smooth_sweeps": 2, "num_post_smooth_sweeps": 3}),
]


@pytest.mark.parametrize("dims,interp,nranks,rep,extra", CASES)
def test_dist_matches_single_gpu(amg, ctx, dims, interp, nranks, rep, extra):
    kw = dict(extra)
    if kw.pop("smoother", None) == "l1":
        kw["smoother"] = amg.AMG_L1_JACOBI
    opts = amg.default_opts(num_cycles=8, tol=0.0, **kw)
    it = amg.AMG_INTERP_AGGREGATE if interp == "aggregate" else amg.AMG_INTERP_LINEAR
    gen = amg.Gen(dims[0], dims[1], dims[2], interp=it)
    n = dims[0] * dims[1] * dims[2]
    f = amg.rhs_rand(0, n)
    cycles = 8
    u1, h1 = single_gpu(amg, ctx, gen, opts, f, cycles)
    ud, hd = distributed(amg, gen, opts, f, cycles, nranks, rep)
    assert_bitwise(ud, u1, "distributed iterate")
    np.testing.assert_allclose(hd, h1, rtol=1e-12, atol=0)
    assert hd[-1] < 0.5 * hd[0]
    gen.free()


def restart_ranks(amg, form, opts, cycles):
    """Two solves of `cycles` cycles on one 2-rank hierarchy of the given form;
    per rank: (first iterate, second iterate, slab_info's fused flag, the
    context's device range-check flags)."""
    slab = form == "slab"
    # slab: the smallest box whose level 0 runs the fused residual + restriction
    # (nx >= 64), so that solve-begin's exchange of f's ghost planes is exercised
    dims = (64, 64, 32) if slab else (24, 24, 24)
    gen = amg.Gen(*dims)
    f = amg.rhs_rand(0, dims[0] * dims[1] * dims[2])
    hub = amg.dist.ThreadMailbox(2)

    def rank(r):
        c = amg.Context(0, nstreams=2)
        tr = amg.dist.HostTransport(hub, r)
        amg.dist.init_host(c, 2, r, tr)
        amg.dist.set_replicate_rows(c, 4096)
        D = amg.dist.DistHier(c, gen, opts, slab=slab)
        fused = D.slab_info()[2]
        outs = []
        for _ in range(2):
            D.solve_start(f[D.row0:D.row0 + D.n0])
            D.iterate(cycles)
            outs.append(D.get_u())
        D.free()
        errs = c.device_errors()
        amg.dist.finalize(c)
        c.close()
        if tr.error is not None:
            raise tr.error
        return outs[0], outs[1], fused, errs

    res = run_ranks(2, rank)
    gen.free()
    return res


def check_restart(res, form, what):
    for a, b, fused, errs in res:
        assert_bitwise(b, a, what)
        assert np.all(np.isfinite(a)) and np.any(a != 0.0)
        assert fused == (1 if form == "slab" else 0), (form, fused)
        assert errs == 0, f"device range-check flags {errs:#x}"


@pytest.mark.parametrize("form", ["rows", "slab"])
def test_dist_restart_is_fresh(amg, form):
    """A second solve on the same distributed hierarchy starts from zero on every
    level (replicated coarsest included): identical to the first.  The slab
    case runs the fused level 0, whose f ghost planes solve-begin exchanges."""
    opts = amg.default_opts(num_cycles=4, tol=0.0)
    check_restart(restart_ranks(amg, form, opts, 4), form, "restart")


@pytest.mark.parametrize("form", ["rows", "slab"])
def test_dist_restart_is_fresh_accelerated(amg, form):
    """Accelerated MULT (DMEM_Mult with the Richardson update): a second solve
    also starts the iterate x, the update direction d and the ChebyUpdate
    recurrence afresh -- bit-identical to the first."""
    mu, delta = cheby_scalars(0.5, 4.0)
    opts = amg.default_opts(num_cycles=3, tol=0.0, smooth_weight=0.8, accel_type=amg.AMG_RICHARD_ACCEL,
                            cheby_mu=mu, cheby_delta=delta)
    check_restart(restart_ranks(amg, form, opts, 3), form, "accelerated restart")


def test_dist_allreduce(amg):
    hub = amg.dist.ThreadMailbox(3)

    def rank(r):
        c = amg.Context(0, nstreams=1)
        amg.dist.init_host(c, 3, r, amg.dist.HostTransport(hub, r))
        out = amg.dist.allreduce_sum(c, [r + 1.0, 2.0 * r])
        amg.dist.barrier(c)
        amg.dist.finalize(c)
        c.close()
        return out

    for o in run_ranks(3, rank):
        np.testing.assert_array_equal(o, [6.0, 6.0])


def test_dist_rccl_single_rank(amg, ctx):
    """The RCCL transport itself (unique id, communicator, allreduce/allgather on
    the stream) at world size 1 -- the only RCCL shape one GPU allows."""
    gen = amg.Gen(32)
    opts = amg.default_opts(num_cycles=6, tol=0.0)
    f = amg.rhs_rand(0, 32 ** 3)
    u1, h1 = single_gpu(amg, ctx, gen, opts, f, 6)
    c = amg.Context(0, nstreams=2)
    amg.dist.init_rccl(c, 1, 0, lambda b: b)
    amg.dist.set_replicate_rows(c, 0)
    D = amg.dist.DistHier(c, gen, opts)
    r0 = D.solve_start(f)
    hist = [r0]
    for _ in range(6):
        D.iterate(1)
        hist.append(D.resnorm())
    u = D.get_u()
    assert D.fine_spmv_ms(3) > 0
    D.free()
    np.testing.assert_array_equal(amg.dist.allreduce_sum(c, [1.5, 2.5]), [1.5, 2.5])
    amg.dist.finalize(c)
    c.close()
    assert_bitwise(u, u1, "rccl single rank")
    np.testing.assert_allclose(hist, h1, rtol=1e-12, atol=0)
    gen.free()


def row_parts(amg, gen, cuts):
    """Per-level row partitions (arbitrary, not plane-aligned) and each rank's
    rows of A/P/R with global column ids, cut from the full host operators."""
    L = gen.L
    full = {w: [gen.host_csr(w, l) for l in range(L if w == amg.AMG_GEN_A else L - 1)]
            for w in (amg.AMG_GEN_A, amg.AMG_GEN_P, amg.AMG_GEN_R)}
    nranks = len(cuts) + 1
    rs = np.zeros((L, nranks + 1), dtype=np.int64)
    for l in range(L):
        n = gen.rows(amg.AMG_GEN_A, l)
        rs[l, 1:-1] = [int(round(c * n)) for c in cuts]
        rs[l, -1] = n

    def rows(w, l, a, b):
        nr, nc, rp, cj, cv = full[w][l]
        lo, hi = rp[a], rp[b]
        return (b - a, rp[a:b + 1] - lo, cj[lo:hi], cv[lo:hi])

    parts = []
    for r in range(nranks):
        A = [rows(amg.AMG_GEN_A, l, rs[l, r], rs[l, r + 1]) for l in range(L)]
        P = [rows(amg.AMG_GEN_P, l, rs[l, r], rs[l, r + 1]) for l in range(L - 1)]
        R = [rows(amg.AMG_GEN_R, l, rs[l + 1, r], rs[l + 1, r + 1]) for l in range(L - 1)]
        parts.append((A, P, R))
    return rs, parts


@pytest.mark.parametrize("cuts,rep", [((0.37,), 0), ((0.2, 0.5, 0.51), 0), ((0.6, 0.9), 4096)])
def test_dist_from_parts_any_partition(amg, ctx, cuts, rep):
    """The general entry (ParCSR-style row_starts + local CSR with global
    columns): any contiguous row partition, empty or ragged ranks included,
    gives the single-GPU iterate bit for bit."""
    gen = amg.Gen(24, 20, 28)
    opts = amg.default_opts(num_cycles=6, tol=0.0)
    n = 24 * 20 * 28
    f = amg.rhs_rand(0, n)
    u1, h1 = single_gpu(amg, ctx, gen, opts, f, 6)
    rs, parts = row_parts(amg, gen, cuts)
    nranks = len(cuts) + 1
    hub = amg.dist.ThreadMailbox(nranks)

    def rank(r):
        c = amg.Context(0, nstreams=2)
        tr = amg.dist.HostTransport(hub, r)
        amg.dist.init_host(c, nranks, r, tr)
        amg.dist.set_replicate_rows(c, rep)
        A, P, R = parts[r]
        D = amg.dist.DistHier.from_parts(c, rs, A, P, R, opts)
        assert (D.row0, D.n0) == (rs[0, r], rs[0, r + 1] - rs[0, r])
        D.solve_start(f[D.row0:D.row0 + D.n0])
        hist = [D.resnorm()]
        for _ in range(6):
            D.iterate(1)
            hist.append(D.resnorm())
        u = D.get_u()
        D.free()
        amg.dist.finalize(c)
        c.close()
        return u, np.array(hist)

    res = run_ranks(nranks, rank)
    assert_bitwise(np.concatenate([t[0] for t in res]), u1, "from_parts iterate")
    np.testing.assert_allclose(res[0][1], h1, rtol=1e-12, atol=0)
    gen.free()


def split_host(host, cuts):
    """row_starts + per-rank (A, P, R) pieces from full host operators (oracle Csr)."""
    L = len(host["A"])
    nranks = len(cuts) + 1
    rs = np.zeros((L, nranks + 1), dtype=np.int64)
    for l in range(L):
        n = host["A"][l].nrows
        rs[l, 1:-1] = [int(round(c * n)) for c in cuts]
        rs[l, -1] = n

    def rows(M, a, b):
        lo, hi = M.rowptr[a], M.rowptr[b]
        return (b - a, M.rowptr[a:b + 1] - lo, M.col[lo:hi], M.val[lo:hi])

    parts = []
    for r in range(nranks):
        parts.append(([rows(host["A"][l], rs[l, r], rs[l, r + 1]) for l in range(L)],
                      [rows(host["P"][l], rs[l, r], rs[l, r + 1]) for l in range(L - 1)],
                      [rows(host["R"][l], rs[l + 1, r], rs[l + 1, r + 1]) for l in range(L - 1)]))
    return rs, parts


@pytest.mark.parametrize("solver,cuts,rep", [("multadd", (0.5,), 0), ("multadd", (0.3, 0.7), 1000),
                                             ("afacx", (0.45,), 0), ("multadd", (), 0),
                                             ("afacx", (), 1000)])
def test_dist_async_band(amg, oracle, ctx, solver, cuts, rep):
    """Distributed asynchronous additive AMG (level streams x ranks, one comm
    stream): nondeterministic; its relres after N corrections per level lies in
    [0.5 x min, 2 x max] of the oracle's asynchronous band (SMEM_Async_Add_AMG
    on OpenMP threads, tests/async_band.py), as the single-GPU async solver."""
    from test_gpu_solve import hierarchy, oracle_opts
    _, L, host = hierarchy(amg, oracle, 24, amg.AMG_INTERP_LINEAR)
    w = 0.8
    Ps, Rs = [], []
    for lev in range(L - 1):
        ps, rs_ = oracle.smooth_transfer(host["A"][lev], host["P"][lev], w)
        Ps.append(ps)
        Rs.append(rs_)
    host = {"A": host["A"], "P": Ps, "R": Rs}
    N = 15
    f = amg.rhs_rand(0, 24 ** 3)
    sync_solver = amg.AMG_MULTADD if solver == "multadd" else amg.AMG_AFACX
    sync_opts = amg.default_opts(solver=sync_solver, smooth_weight=w, num_cycles=N, tol=0.0)
    _, h_c, _ = oracle.Hier(host["A"], host["P"], host["R"], oracle_opts(oracle, sync_opts)).solve(f)
    sync_rel = h_c[-1] / h_c[0]
    a_solver = amg.AMG_ASYNC_MULTADD if solver == "multadd" else amg.AMG_ASYNC_AFACX
    opts = amg.default_opts(solver=a_solver, smooth_weight=w, num_cycles=N, tol=0.0)
    rs, parts = split_host(host, cuts)
    nranks = len(cuts) + 1
    hub = amg.dist.ThreadMailbox(nranks)

    def rank(r):
        c = amg.Context(0, nstreams=L)
        if nranks == 1:  # one rank: the RCCL transport itself
            amg.dist.init_rccl(c, 1, 0, lambda b: b)
        else:
            amg.dist.init_host(c, nranks, r, amg.dist.HostTransport(hub, r))
        amg.dist.set_replicate_rows(c, rep)
        A, P, R = parts[r]
        D = amg.dist.DistHier.from_parts(c, rs, A, P, R, opts)
        out = []
        for _ in range(3):
            rel, cnt = D.async_solve(f[D.row0:D.row0 + D.n0])
            e_, s_ = race_tables(D)
            out.append((rel, D.get_u(), cnt.copy(), e_, s_))
        D.free()
        amg.dist.finalize(c)
        c.close()
        return out

    res = run_ranks(nranks, rank)
    from async_band import replay_check
    rels, runs = [], []
    for q in range(3):
        rq = [t[q][0] for t in res]
        assert all(r == rq[0] for r in rq)  # one allreduced norm
        u = np.concatenate([t[q][1] for t in res])
        assert np.all(np.isfinite(u))
        cnt = res[0][q][2]
        assert list(cnt[:L - 1]) == [N] * (L - 1)
        assert rq[0] < 1.0
        rels.append(rq[0])
        runs.append((rq[0], [t[q][3] for t in res], [int(x) for x in rs[0]], [t[q][4] for t in res]))
    # the oracle's model of each run: the replay of its recorded update orders
    # (every correction's update point; the slowest rank's and each rank's),
    # or_async_add under the timed schedule (the arithmetic itself is pinned by
    # test_dist_async_schedule_bitwise)
    print(f"dist async {solver} {nranks} ranks: sync {sync_rel:.4e}, device {rels}")
    widest = replay_check(amg, oracle, host, f, opts, runs, what=f"dist async {solver} {nranks} ranks")
    assert widest <= 20.0


@pytest.mark.parametrize("solver,cuts,rep,sched", [("multadd", (0.5,), 0, 3), ("multadd", (0.3, 0.7), 1000, 1),
                                                   ("afacx", (0.45,), 0, 2), ("multadd", (), 0, 2),
                                                   ("afacx", (0.5,), 1000, 3)])
def test_dist_async_schedule_bitwise(amg, oracle, ctx, solver, cuts, rep, sched):
    """The row-partitioned asynchronous additive solve (from_parts, explicit
    smoothed transfers) under a deterministic schedule (async_schedule 1 / 2 /
    3: finest first, coarsest first, round robin) against the oracle's
    or_async_add under the same schedule, one thread per level group: the
    assembled iterate is the same bits at 1-3 ranks."""
    from test_gpu_solve import hierarchy, oracle_opts
    _, L, host = hierarchy(amg, oracle, 24, amg.AMG_INTERP_LINEAR)
    w, N = 0.8, 10
    Ps, Rs = [], []
    for lev in range(L - 1):
        ps, rs_ = oracle.smooth_transfer(host["A"][lev], host["P"][lev], w)
        Ps.append(ps)
        Rs.append(rs_)
    host = {"A": host["A"], "P": Ps, "R": Rs}
    f = amg.rhs_rand(0, 24 ** 3)
    a_solver = amg.AMG_ASYNC_MULTADD if solver == "multadd" else amg.AMG_ASYNC_AFACX
    opts = amg.default_opts(solver=a_solver, smooth_weight=w, num_cycles=N, tol=0.0, async_schedule=sched)
    rs, parts = split_host(host, cuts)
    nranks = len(cuts) + 1
    hub = amg.dist.ThreadMailbox(nranks)

    def rank(r):
        c = amg.Context(0, nstreams=L)
        if nranks == 1:
            amg.dist.init_rccl(c, 1, 0, lambda b: b)
        else:
            amg.dist.init_host(c, nranks, r, amg.dist.HostTransport(hub, r))
        amg.dist.set_replicate_rows(c, rep)
        A, P, R = parts[r]
        D = amg.dist.DistHier.from_parts(c, rs, A, P, R, opts)
        rel, cnt = D.async_solve(f[D.row0:D.row0 + D.n0])
        out = (D.row0, rel, cnt.copy(), D.get_u())
        D.free()
        amg.dist.finalize(c)
        c.close()
        return out

    res = sorted(run_ranks(nranks, rank), key=lambda t: t[0])
    u = np.concatenate([t[3] for t in res])
    rel, cnt = res[0][1], res[0][2]
    OH = oracle.Hier(host["A"], host["P"], host["R"], oracle_opts(oracle, opts))
    oracle.lib().or_set_async_schedule(sched)
    try:
        uo, relo, cnto = OH.async_add(f, [1] * L)
    finally:
        oracle.lib().or_set_async_schedule(0)
    nd = int(np.count_nonzero(u.view(np.uint64) != uo.view(np.uint64)))
    print(f"dist async {solver} {nranks} ranks schedule {sched}: device {rel:.13e} oracle {relo:.13e}, "
          f"differing entries {nd}")
    assert list(cnt[:L - 1]) == list(cnto[:L - 1]) == [N] * (L - 1)
    assert_bitwise(u, uo, "row-partitioned async iterate vs oracle")
    assert abs(rel - relo) <= 1e-12 * relo


@pytest.mark.parametrize("nranks,l1", [(1, 0), (2, 0), (3, 1)])
def test_dist_async_jacobi(amg, oracle, ctx, nranks, l1):
    """DMEM_AsyncSmooth: Jacobi in residual-update form with asynchronous ghost
    deltas.  Every delta is applied exactly once (drained at the end), so the
    result matches synchronous Jacobi up to the order of the additions; the
    single-rank run goes through RCCL itself."""
    n = 20
    gen = amg.Gen(n)
    f = amg.rhs_rand(0, n ** 3)
    K, w = 15, 0.7
    nr, nc, rp, cj, cv = gen.host_csr(amg.AMG_GEN_A, 0)
    A = oracle.Csr(nr, nc, rp, cj, cv)
    # synchronous reference: SMEM_Sync_Parfor_Jacobi from zero (zero_flag 0)
    u = np.zeros(nr)
    if l1:
        l1n = oracle.l1_norms(A)
        for _ in range(K):
            oracle.smem_l1jacobi(A, f, u, np.zeros(nr), l1n, 1, 0, 0, nr)
    else:
        for _ in range(K):
            oracle.smem_jacobi(A, f, u, np.zeros(nr), w, 1, 0, 0, nr)
    r = f - oracle.smem_matvec(A, u, np.zeros(nr))
    ref_rel = np.linalg.norm(r) / np.linalg.norm(f)
    opts = amg.default_opts(smooth_weight=w)
    hub = amg.dist.ThreadMailbox(nranks)

    def rank(q):
        c = amg.Context(0, nstreams=2)
        if nranks == 1:
            amg.dist.init_rccl(c, 1, 0, lambda b: b)
        else:
            amg.dist.init_host(c, nranks, q, amg.dist.HostTransport(hub, q))
        D = amg.dist.DistHier(c, gen, opts)
        rel = D.async_jacobi(f[D.row0:D.row0 + D.n0], K, l1)
        x = D.get_u()
        st = D.async_jacobi_stats()
        log = D.async_jacobi_log()
        row0 = D.row0
        D.free()
        amg.dist.finalize(c)
        c.close()
        return row0, x, rel, st, log

    res = sorted(run_ranks(nranks, rank), key=lambda t: t[0])
    x = np.concatenate([t[1] for t in res])
    assert all(t[2] == res[0][2] for t in res)
    st = res[0][3]
    print(f"async jacobi {nranks} ranks l1={l1}: relres {res[0][2]:.6e} (sync {ref_rel:.6e}), {st}")
    # every delta applied exactly once: the incrementally kept residual is f - A x
    assert abs(st["incremental_resnorm"] - st["true_resnorm"]) <= 1e-9 * st["true_resnorm"], st
    if nranks > 1:
        assert st["device_links"] == 1.0 and 0.0 <= st["on_time_fraction"] <= 1.0, st
    if nranks == 1:  # nothing to wait for: exactly synchronous Jacobi, rounding aside
        np.testing.assert_allclose(res[0][2], ref_rel, rtol=1e-8)
        np.testing.assert_allclose(x, u, rtol=1e-9, atol=1e-12 * np.abs(u).max())
    # the run against the replay of its own schedule (which relaxation of each
    # peer every rank's residual had seen when it relaxed, tests/ajac_replay.py)
    from ajac_replay import check_replay, host_csr
    rs = [t[0] for t in res] + [nr]
    check_replay(host_csr(nr, nc, rp, cj, cv), f, rs, [t[4] for t in res], x, res[0][2], w,
                 l1=oracle.l1_norms(A) if l1 else None, what=f"async jacobi {nranks} ranks l1={l1}")
    gen.free()


def test_dist_async_jacobi_one_way_peers(amg, oracle, ctx):
    """DMEM_AsyncSmooth on a pattern-nonsymmetric operator (upwind: the 7-pt
    Laplacian's lower triangle, a_ij = 0 for j > i): rank 0's rows read no
    ghost column, rank 1's read rank 0's -- rank 0 only sends, rank 1 only
    receives.  The device-resident channels carry both directions (every delta
    applied once: the incrementally kept residual is f - A x); rank 0's rows
    depend on rank 0's alone, so they are synchronous Jacobi's (rounding aside:
    residual-update form); rank 1's see rank 0's deltas late, and the whole
    iterate still contracts."""
    from test_gpu_solve import hierarchy
    _, L, host = hierarchy(amg, oracle, 16, amg.AMG_INTERP_LINEAR)
    A0 = host["A"][0]
    rp, cj, cv = [0], [], []
    for i in range(A0.nrows):
        for q in range(A0.rowptr[i], A0.rowptr[i + 1]):
            if A0.col[q] <= i:
                cj.append(A0.col[q])
                cv.append(A0.val[q])
        rp.append(len(cj))
    up = oracle.Csr(A0.nrows, A0.ncols, np.array(rp), np.array(cj, dtype=np.int32), np.array(cv))
    host = {"A": [up] + host["A"][1:], "P": host["P"], "R": host["R"]}
    n = up.nrows
    f = amg.rhs_rand(0, n)
    K, w = 12, 0.7
    u = np.zeros(n)
    for _ in range(K):
        oracle.smem_jacobi(up, f, u, np.zeros(n), w, 1, 0, 0, n)
    ref_rel = np.linalg.norm(f - oracle.smem_matvec(up, u, np.zeros(n))) / np.linalg.norm(f)
    rs, parts = split_host(host, (0.5,))
    hub = amg.dist.ThreadMailbox(2)
    opts = amg.default_opts(smooth_weight=w)

    def rank(q):
        c = amg.Context(0, nstreams=2)
        amg.dist.init_host(c, 2, q, amg.dist.HostTransport(hub, q))
        A, P, R = parts[q]
        D = amg.dist.DistHier.from_parts(c, rs, A, P, R, opts)
        rel = D.async_jacobi(f[D.row0:D.row0 + D.n0], K)
        st = D.async_jacobi_stats()
        x = D.get_u()
        log = D.async_jacobi_log()
        row0 = D.row0
        D.free()
        amg.dist.finalize(c)
        c.close()
        return rel, st, x, row0, log

    res = sorted(run_ranks(2, rank), key=lambda t: t[3])
    for rel, st, x, row0, _ in res:
        print(f"one-way peers: rank at row {row0}: relres {rel:.6e} (sync {ref_rel:.6e}), {st}")
        assert np.all(np.isfinite(x))
        assert st["device_links"] == 1.0, st
        assert abs(st["incremental_resnorm"] - st["true_resnorm"]) <= 1e-9 * st["true_resnorm"], st
        assert rel < 0.1, rel
    x0 = res[0][2]
    np.testing.assert_allclose(x0, u[:x0.size], rtol=1e-9, atol=1e-12 * np.abs(u).max())
    from ajac_replay import check_replay, host_csr
    check_replay(host_csr(n, n, up.rowptr, up.col, up.val), f, [0, res[1][3], n], [t[4] for t in res],
                 np.concatenate([t[2] for t in res]), res[0][0], w, what="one-way peers")


# ---------------------------------------------------------------------------
# DMEM outer acceleration (DMEM_ChebyUpdate, DMEM_Misc.cpp:612-666)
# ---------------------------------------------------------------------------
def cheby_scalars(alpha, beta):
    """DMEM_Setup.cpp:1905-1908: mu = (b + a) / (b - a), delta = 2 / (b + a)."""
    return (beta + alpha) / (beta - alpha), 2.0 / (beta + alpha)


@pytest.mark.parametrize("accel,nranks,rep,extra", [
    ("richard", 1, 1 << 18, {}),
    ("richard", 2, 0, {}),
    ("recur", 3, 512, {}),
    ("recur", 2, 0, {"smoother": "l1", "num_pre_smooth_sweeps": 2}),
])
def test_dist_mult_accel_matches_oracle(amg, oracle, accel, nranks, rep, extra):
    """DMEM_Mult with -cheby / -richard: per cycle e = M r from zero, x += e,
    ChebyUpdate(d, e), x += d.  The slab-distributed iterate is BIT-IDENTICAL
    to the oracle's restatement (or_dmem_mult_solve), norms within 1e-12.
    The reference adds both e and d (DMEM_Mult.cpp:46-55), so the update is
    about twice the preconditioned correction: the eigenvalue bounds given
    here (0.5, 4) are wider than M^-1 A's (about 0.48, 0.99) to keep it
    convergent, as a user of the reference would have to."""
    from test_gpu_solve import hierarchy, oracle_opts
    kw = dict(extra)
    if kw.pop("smoother", None) == "l1":
        kw["smoother"] = amg.AMG_L1_JACOBI
    mu, delta = cheby_scalars(0.5, 4.0)
    acc = amg.AMG_RICHARD_ACCEL if accel == "richard" else amg.AMG_CHEBY_RECUR_ACCEL
    cycles = 8
    opts = amg.default_opts(num_cycles=cycles, tol=0.0, smooth_weight=0.8, accel_type=acc,
                            cheby_mu=mu, cheby_delta=delta, reuse_outer_residual=1, **kw)
    gen, L, host = hierarchy(amg, oracle, 24, amg.AMG_INTERP_LINEAR)
    f = amg.rhs_rand(0, 24 ** 3)
    OH = oracle.Hier(host["A"], host["P"], host["R"], oracle_opts(oracle, opts))
    acc_o = oracle.OR_RICHARD_ACCEL if accel == "richard" else oracle.OR_CHEBY_RECUR_ACCEL
    x_o, h_o, k = OH.dmem_mult_solve(f, acc_o, mu, delta)
    assert k == cycles
    xd, hd = distributed(amg, gen, opts, f, cycles, nranks, rep)
    assert_bitwise(xd, x_o, "accelerated DMEM_Mult iterate")
    np.testing.assert_allclose(hd, h_o, rtol=1e-12, atol=0)
    # with these bounds the unaccelerated DMEM_Mult converges slower
    _, h_plain, _ = OH.dmem_mult_solve(f, oracle.OR_NO_ACCEL)
    assert h_o[-1] < h_plain[-1]
    gen.free()


@pytest.mark.parametrize("nranks,l1,accel,grid", [(1, 0, "richard", 0), (1, 1, "recur", 0),
                                                   (1, 0, "recur", 1), (2, 0, "richard", 0),
                                                   (3, 1, "recur", 0)])
def test_dist_async_jacobi_accel(amg, oracle, ctx, nranks, l1, accel, grid):
    """DMEM_AsyncSmooth with ChebyUpdate on the relaxation (async branch; the
    fine grid is grid 0, so cheby_grid 0 carries d and any other value scales
    u by w*delta).  One rank has nothing asynchronous: BIT-IDENTICAL to the
    oracle (or_dmem_async_jacobi).  More ranks apply late ghost deltas one
    relaxation later: a band around the one-rank result."""
    n = 20
    gen = amg.Gen(n)
    f = amg.rhs_rand(0, n ** 3)
    K, w = 25, 0.7
    mu, delta = cheby_scalars(0.1 * w, 2.0 * w)
    acc = amg.AMG_RICHARD_ACCEL if accel == "richard" else amg.AMG_CHEBY_RECUR_ACCEL
    nr, nc, rp, cj, cv = gen.host_csr(amg.AMG_GEN_A, 0)
    A = oracle.Csr(nr, nc, rp, cj, cv)
    l1n = oracle.l1_norms(A) if l1 else None
    acc_o = oracle.OR_RICHARD_ACCEL if accel == "richard" else oracle.OR_CHEBY_RECUR_ACCEL
    if grid == 0:
        x_o, rn_o = oracle.dmem_async_jacobi(A, f, K, w, l1n, acc_o, mu, delta)
    else:  # cheby_grid != 0: u = w*delta*u after the first relaxation
        x_o, rn_o = None, None
    x_plain, rn_plain = oracle.dmem_async_jacobi(A, f, K, w, l1n)
    fn = np.linalg.norm(f)
    opts = amg.default_opts(smooth_weight=w, accel_type=acc, cheby_mu=mu, cheby_delta=delta,
                            cheby_grid=grid)
    hub = amg.dist.ThreadMailbox(nranks)

    def rank(q):
        c = amg.Context(0, nstreams=2)
        if nranks == 1:
            amg.dist.init_rccl(c, 1, 0, lambda b: b)
        else:
            amg.dist.init_host(c, nranks, q, amg.dist.HostTransport(hub, q))
        D = amg.dist.DistHier(c, gen, opts)
        rel = D.async_jacobi(f[D.row0:D.row0 + D.n0], K, l1)
        x = D.get_u()
        log = D.async_jacobi_log()
        row0 = D.row0
        D.free()
        amg.dist.finalize(c)
        c.close()
        return row0, x, rel, log

    res = sorted(run_ranks(nranks, rank), key=lambda t: t[0])
    x = np.concatenate([t[1] for t in res])
    rel = res[0][2]
    assert all(t[2] == rel for t in res)
    assert np.all(np.isfinite(x))
    if x_o is not None and nranks == 1:
        assert_bitwise(x, x_o, "accelerated async Jacobi (one rank)")
        np.testing.assert_allclose(rel, rn_o / fn, rtol=1e-12)
        if grid == 0:
            assert rel < rn_plain / fn  # the momentum helps on the Laplacian
    elif x_o is not None:
        print(f"accelerated async jacobi {nranks} ranks: relres {rel:.4e}, one rank {rn_o / fn:.4e}")
    # more ranks: late ghost deltas; the run against the replay of its own
    # schedule with the same ChebyUpdate coefficients (tests/ajac_replay.py)
    from ajac_replay import check_replay, host_csr
    rs = [t[0] for t in res] + [nr]
    check_replay(host_csr(nr, nc, rp, cj, cv), f, rs, [t[3] for t in res], x, rel, w, l1=l1n,
                 what=f"accelerated async jacobi {nranks} ranks {accel} grid {grid}")
    gen.free()


@pytest.mark.parametrize("solver,accel,cuts,grid,bounds", [
    ("multadd", "richard", (0.5,), 0, (0.5, 4.0)),
    ("afacx", "recur", (0.4,), 1, (0.2, 2.0)),
    ("afacx", "richard", (), 0, (0.2, 2.0)),
])
def test_dist_async_additive_accel(amg, oracle, solver, accel, cuts, grid, bounds):
    """Asynchronous additive AMG with ChebyUpdate on every level's fine
    correction (DMEM_Add.cpp:319-324): the cheby_grid level carries d, the
    others scale by w*delta.  Nondeterministic: its relres must lie in
    [0.5 x min, 2 x max] of the oracle's asynchronous band with the same
    ChebyUpdate per level group (or_set_async_accel).  (Measured on one MI355X,
    24^3, 15 corrections, profiles/r03/async_global/: MULTADD + Richardson
    2.0e-5 in [2.1e-5, 1.4e-2] (plain 4.7e-6), AFACx + recurrence 3.0e-3 in
    [3.0e-3, 1.4e-2], AFACx + Richardson 4.4e-5 in [4.2e-5, 1.1e-2] (plain
    5.0e-4) -- the device lands at the band's low end.)"""
    from test_gpu_solve import hierarchy
    _, L, host = hierarchy(amg, oracle, 24, amg.AMG_INTERP_LINEAR)
    w = 0.8
    Ps, Rs = [], []
    for lev in range(L - 1):
        ps, rs_ = oracle.smooth_transfer(host["A"][lev], host["P"][lev], w)
        Ps.append(ps)
        Rs.append(rs_)
    host = {"A": host["A"], "P": Ps, "R": Rs}
    N = 15
    f = amg.rhs_rand(0, 24 ** 3)
    mu, delta = cheby_scalars(*bounds)
    acc = amg.AMG_RICHARD_ACCEL if accel == "richard" else amg.AMG_CHEBY_RECUR_ACCEL
    a_solver = amg.AMG_ASYNC_MULTADD if solver == "multadd" else amg.AMG_ASYNC_AFACX
    rs, parts = split_host(host, cuts)
    nranks = len(cuts) + 1

    def solve(accel_type):
        opts = amg.default_opts(solver=a_solver, smooth_weight=w, num_cycles=N, tol=0.0,
                                accel_type=accel_type, cheby_mu=mu, cheby_delta=delta, cheby_grid=grid)
        hub = amg.dist.ThreadMailbox(nranks)

        def rank(r):
            c = amg.Context(0, nstreams=L)
            if nranks == 1:
                amg.dist.init_rccl(c, 1, 0, lambda b: b)
            else:
                amg.dist.init_host(c, nranks, r, amg.dist.HostTransport(hub, r))
            A, P, R = parts[r]
            D = amg.dist.DistHier.from_parts(c, rs, A, P, R, opts)
            rel, cnt = D.async_solve(f[D.row0:D.row0 + D.n0])
            u = D.get_u()
            ms = race_tables(D)
            D.free()
            amg.dist.finalize(c)
            c.close()
            return rel, u, cnt.copy(), ms

        res = run_ranks(nranks, rank)
        assert all(t[0] == res[0][0] for t in res)
        assert all(np.all(np.isfinite(t[1])) for t in res)
        return res[0][0], [t[3][0] for t in res], [t[3][1] for t in res]

    from async_band import replay_check
    (rel_acc, d_acc, s_acc), (rel_plain, _, _) = solve(acc), solve(amg.AMG_NO_ACCEL)
    d_acc = (d_acc, [int(x) for x in rs[0]], s_acc)
    assert rel_acc < 1.0
    opts = amg.default_opts(solver=a_solver, smooth_weight=w, num_cycles=N, tol=0.0, accel_type=acc,
                            cheby_mu=mu, cheby_delta=delta, cheby_grid=grid)
    # the oracle's model of the run: the replay of its recorded update order,
    # with the same ChebyUpdate per level group (timed schedule)
    print(f"dist async {solver} {accel} grid {grid}: device {rel_acc:.4e} (no accel {rel_plain:.4e})")
    replay_check(amg, oracle, host, f, opts, [(rel_acc,) + d_acc], what=f"dist async {solver} {accel}")


@pytest.mark.slow
@pytest.mark.parametrize("R", [8, 2])
def test_dist_async_jacobi_512(amg, ctx, R):
    """DMEM_AsyncSmooth at config 4's size: the 512^3 fine operator (A0 of
    11.8 GB) as 8 row-partitioned ranks (threads) on one GPU, the ghost deltas
    through the device-resident channels (a send is a copy kernel on the comm
    stream into the neighbour's slot, overlapping the interior product; a
    receive an MPI_Test-like poll).  Properties: every delta applied exactly
    once (the incrementally kept residual equals f - A x to rounding, every
    rank received `sweeps` messages from each neighbour), the residual
    contracts like Jacobi, and the fraction of the exchange hidden behind the
    interior product is reported per rank."""
    n, K, w = 512, 12, 0.8
    gen = amg.Gen(n)
    f = amg.rhs_rand(0, n ** 3)
    opts = amg.default_opts(smooth_weight=w)
    hub = amg.dist.ThreadMailbox(R, timeout=900.0)

    def rank(q):
        c = amg.Context(0, nstreams=2)
        amg.dist.init_host(c, R, q, amg.dist.HostTransport(hub, q))
        amg.dist.set_replicate_rows(c, 1 << 18)
        D = amg.dist.DistHier(c, gen, opts)
        rel = D.async_jacobi(f[D.row0:D.row0 + D.n0], K, 0)
        st = D.async_jacobi_stats()
        D.free()
        amg.dist.finalize(c)
        c.close()
        return rel, st

    res = run_ranks(R, rank)
    rels = [t[0] for t in res]
    assert all(r == rels[0] for r in rels)
    for q, (rel, st) in enumerate(res):
        print(f"512^3 async Jacobi {R} ranks, rank {q}: relres {rel:.6e}, hidden {st['hidden_fraction']:.3f}, exchange "
              f"{st['exchange_ms_per_sweep']:.3f} ms, interior {st['interior_ms_per_sweep']:.3f} ms, on time "
              f"{st['on_time_fraction']:.3f}, late {st['late_deltas']:.0f}, send wait "
              f"{st['send_wait_ms_per_sweep']:.3f} ms/sweep")
        assert st["device_links"] == 1.0
        assert abs(st["incremental_resnorm"] - st["true_resnorm"]) <= 1e-9 * st["true_resnorm"], st
    # Jacobi on the 7-pt Laplacian: the smooth residual decays slowly, but it decays
    assert 0.0 < rels[0] < 1.0
    gen.free()
