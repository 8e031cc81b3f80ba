"""The CG-Lanczos eigenvalue estimate on the distributed level-0 operator (amg_dist_eigs_cg,
amg_dist_pcg_eigs) on the MI355X against the host model.

Ranks run as threads over the host transport, as in tests/test_gpu_dist_pcg.py; one rank also
runs over RCCL.  Every dot product is summed per rank in amg_vec_dot's order and the rank values
are added in rank order, so the alpha / beta / gamma history, the number of valid iterations and
both extremes are compared bit for bit with eigs_ref.eigs_model under dist_pcg_ref.dist_dot of the
partition the ranks report, and every rank must return the same bits.
"""
import numpy as np
import pytest

import dist_pcg_ref
import eigs_ref
from test_gpu_dist import row_parts
from test_gpu_dist_pcg import cut_parts, from_parts, gen_host, ranks, row_starts, structured
from test_gpu_kernels import assert_bitwise
from test_gpu_pcg import case_opts

pytestmark = pytest.mark.gpu

ITERS = 10


def start_vector(n, seed=9):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


def drive(iters, scale=1, r0=None):
    def body(D, r):
        sl = slice(D.row0, D.row0 + D.n0)
        return dict(row0=D.row0, n0=D.n0, res=D.eigs_cg(iters, scale, None if r0 is None else r0[sl]))
    return body


def check_model(oracle, res, A, iters, scale, r0, what):
    """every rank's eigs_cg result against the model under the partition's rank-ordered dot"""
    ma, mb, mg = eigs_ref.eigs_model(oracle, A, iters, scale, r0, dot=dist_pcg_ref.dist_dot(row_starts(res)))
    want = eigs_ref.estimate(ma, mb, mg)
    assert want[2] == iters
    for t in res:
        emax, emin, a, b, g, k = t["res"]
        assert_bitwise(g, mg, f"{what}: gamma")
        assert_bitwise(a, ma, f"{what}: alpha")
        assert_bitwise(b, mb, f"{what}: beta")
        assert k == want[2]
        assert_bitwise(np.array([emax, emin]), np.array(want[:2]), f"{what}: extremes")


# ---- 1. row form ----------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [1, 2, 3])
def test_structured_rows(amg, oracle, nranks):
    gen, L, host = gen_host(amg, oracle, (12, 12, 12))
    opts = case_opts(amg, "mult_jacobi", num_cycles=1)
    for scale, r0 in ((1, None), (0, start_vector(12 ** 3))):
        res = ranks(amg, nranks, structured(amg, gen, opts), drive(ITERS, scale, r0))
        assert len(res) == nranks and sum(t["n0"] for t in res) == 12 ** 3
        check_model(oracle, res, host["A"][0], ITERS, scale, r0, f"12^3 x{nranks} scale={scale}")


def test_any_partition_with_an_empty_rank(amg, oracle):
    gen, L, host = gen_host(amg, oracle, (12, 12, 12))
    opts = case_opts(amg, "mult_jacobi", num_cycles=1)
    rs, parts = row_parts(amg, gen, (0.23, 0.23, 0.71))
    assert rs[0, 1] == rs[0, 2]  # rank 1 owns nothing
    r0 = start_vector(12 ** 3)
    for scale, start in ((1, None), (1, r0), (0, r0)):
        res = ranks(amg, 4, from_parts(amg, rs, parts, opts), drive(ITERS, scale, start))
        assert row_starts(res) == list(rs[0]) and res[1]["n0"] == 0
        check_model(oracle, res, host["A"][0], ITERS, scale, start, f"cuts with an empty rank, scale={scale}")


# ---- 2. slab form ---------------------------------------------------------------------
def test_slab_form(amg, oracle):
    gen, L, host = gen_host(amg, oracle, (64, 64, 64))
    opts = case_opts(amg, "mult_jacobi", num_cycles=1)

    def body(D, r):
        out = drive(6)(D, r)
        out["slab"] = D.slab_info()
        return out

    res = ranks(amg, 2, structured(amg, gen, opts, slab=True), body, rep=1 << 12)
    for t in res:
        assert t["slab"][0] >= 1, t["slab"]
    check_model(oracle, res, host["A"][0], 6, 1, None, "slab 64^3")


# ---- 3. one rank is one GPU -----------------------------------------------------------
@pytest.mark.parametrize("rccl", [False, True])
def test_one_rank_is_one_gpu(amg, oracle, ctx, rccl):
    gen, L, host = gen_host(amg, oracle, (12, 12, 12))
    opts = case_opts(amg, "mult_jacobi", num_cycles=1)
    A = host["A"][0]
    M = ctx.csr(A.nrows, A.ncols, A.rowptr, A.col, A.val)
    r0 = start_vector(A.nrows)
    cases = ((1, None), (0, r0))

    def body(D, r):  # one communicator for both cases
        return [drive(ITERS, scale, start)(D, r)["res"] for scale, start in cases]

    (got,) = ranks(amg, 1, structured(amg, gen, opts), body, rccl=rccl)
    for (scale, start), res in zip(cases, got):
        one = ctx.eigs_cg(M, ITERS, scale, start)
        assert res[5] == one[5] == ITERS
        assert_bitwise(np.array(res[:2]), np.array(one[:2]), "extremes")
        for a, b, what in zip(res[2:5], one[2:5], ("alpha", "beta", "gamma")):
            assert_bitwise(a, b, what)
    M.free()


# ---- 4. the default start does not depend on the partition ----------------------------
def test_default_start_by_global_row(amg, oracle):
    gen, L, host = gen_host(amg, oracle, (12, 12, 12))
    opts = case_opts(amg, "mult_jacobi", num_cycles=1)
    n = 12 ** 3
    whole = 2.0 * amg.lehmer_stream(n) - 1.0  # the one-GPU default
    assert_bitwise(whole, eigs_ref.default_start(n), "the one-GPU default start")

    def body(D, r):
        mine = 2.0 * amg.lehmer_stream(D.n0, skip=D.row0) - 1.0
        return dict(row0=D.row0, n0=D.n0, mine=mine, default=D.eigs_cg(ITERS), given=D.eigs_cg(ITERS, 1, mine))

    res = ranks(amg, 3, structured(amg, gen, opts), body)
    assert_bitwise(np.concatenate([t["mine"] for t in res]), whole, "the start assembled over 3 ranks")
    for t in res:  # the device's default is that vector
        assert t["default"][5] == t["given"][5] == ITERS
        for a, b, what in zip(t["default"][2:5], t["given"][2:5], ("alpha", "beta", "gamma")):
            assert_bitwise(a, b, what)
    for t in res:
        t["res"] = t["default"]
    check_model(oracle, res, host["A"][0], ITERS, 1, None, "default start x3")


# ---- 5. the running PCG's spectrum ----------------------------------------------------
def test_pcg_eigs(amg, oracle):
    gen, L, host = gen_host(amg, oracle, (16, 16, 16))
    opts = case_opts(amg, "mult_jacobi", num_cycles=6)
    f = amg.rhs_rand(0, 16 ** 3)

    def body(D, r):
        with pytest.raises(amg.AmgError, match="no PCG state"):
            D.pcg_eigs()
        D.pcg_start(f[D.row0:D.row0 + D.n0])
        D.pcg_iterate(6)
        return D.pcg_scalars(), D.pcg_eigs()

    res = ranks(amg, 2, structured(amg, gen, opts), body)
    for (a, b, rho), (emax, emin, k) in res:
        assert k == 6 and len(a) == 6
        assert_bitwise(np.array([emax, emin]), np.array(amg.lanczos_extremes(a, b)), "pcg_eigs")
        assert_bitwise(a, res[0][0][0], "alpha on every rank")
    assert res[0][1] == res[1][1]


# ---- 6. a refusal returns on every rank -----------------------------------------------
def test_zero_diagonal_refused_on_every_rank(amg, oracle):
    """the bad row is rank 1's alone: the counts are gathered, so rank 0 refuses too and nobody is
    left waiting in a collective (a rank left waiting would run into the mailbox's time limit)"""
    n = 600
    A = eigs_ref.tridiag_varied(oracle, n)
    val = A.val.copy()
    val[A.rowptr[450]] = 0.0
    host = {"A": [oracle.Csr(n, n, A.rowptr, A.col, val)], "P": [], "R": []}
    rs = np.array([[0, 300, n]], dtype=np.int64)
    opts = case_opts(amg, "mult_jacobi", num_cycles=1)

    def body(D, r):
        with pytest.raises(amg.AmgError, match=r"status -1: amg_dist_eigs_cg: .*1 row\(s\) with a_ii <= 0"):
            D.eigs_cg(5, scale=1)
        return dict(row0=D.row0, n0=D.n0, res=D.eigs_cg(5, scale=0))  # d is not read: both go on together

    res = ranks(amg, 2, from_parts(amg, rs, cut_parts(host, rs), opts), body)
    ma, mb, mg = eigs_ref.eigs_model(oracle, host["A"][0], 5, 0, None, dot=dist_pcg_ref.dist_dot([0, 300, n]))
    for t in res:
        assert_bitwise(t["res"][4], mg, "gamma, unscaled")
        assert_bitwise(t["res"][2], ma, "alpha, unscaled")
