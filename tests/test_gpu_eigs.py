"""The CG-Lanczos eigenvalue estimate (amg_eigs_cg, amg_pcg_eigs) on the MI355X against the host
model (tests/eigs_ref.py).

Every statement of the recurrence is one rounded fp64 operation and every sum runs in
amg_vec_dot's order, so the whole alpha / beta / gamma history, the number of valid iterations
and both extremes are compared bit for bit, in whatever storage form the operator has.
"""
import numpy as np
import pytest

import eigs_ref
import pcg_ref
from test_gpu_kernels import assert_bitwise
from test_gpu_pcg import cached, case_opts

pytestmark = pytest.mark.gpu


def start_vector(n, seed=5):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


def check_case(amg, oracle, ctx, M, A, iters, scale, r0, what):
    """one amg_eigs_cg call against the model; returns (emax, emin, k), or None where k = 0 is refused"""
    ma, mb, mg = eigs_ref.eigs_model(oracle, A, iters, scale, r0)
    want = eigs_ref.estimate(ma, mb, mg)
    if want[2] == 0:
        with pytest.raises(amg.AmgError, match="no valid iteration"):
            ctx.eigs_cg(M, iters, scale, r0)
        return None
    emax, emin, a, b, g, k = ctx.eigs_cg(M, iters, scale, r0)
    assert len(a) == iters and len(b) == iters and len(g) == iters + 1
    assert_bitwise(g, mg, f"{what}: gamma")
    assert_bitwise(a, ma, f"{what}: alpha")
    assert_bitwise(b, mb, f"{what}: beta")
    assert k == want[2], (what, k, want[2])
    assert_bitwise(np.array([emax, emin]), np.array(want[:2]), f"{what}: extremes")
    return emax, emin, k


def both_scales(amg, oracle, ctx, M, A, iters, what):
    """scale 1 from the default start and from a given one, scale 0 likewise"""
    out = {}
    for scale in (1, 0):
        for r0 in (None, start_vector(A.nrows)):
            tag = f"{what} scale={scale} {'default' if r0 is None else 'given'} start"
            out[scale, r0 is None] = check_case(amg, oracle, ctx, M, A, iters, scale, r0, tag)
    return out


# ---- 1. the vector kernels' grid edges ------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1023, 1025, 2049, 4097, 9001])
def test_tridiagonal_sizes(amg, oracle, ctx, n):
    """tridiag(-1, 4 + 0.25 (i % 5), -1): lanes past the end, both sides of the four-stride main
    loop (one workgroup: 1024 rows a round), red_blocks 1, 2, 3 and 5.  At n = 1 and 2 the residual
    dies inside max_iter = 6: fewer valid iterations than asked for, and the zero-divisor rules"""
    A = eigs_ref.tridiag_varied(oracle, n)
    M = ctx.csr(A.nrows, A.ncols, A.rowptr, A.col, A.val)
    iters = 6 if n <= 2 else 8
    res = both_scales(amg, oracle, ctx, M, A, iters, f"tridiag n={n}")
    for (scale, default), r in res.items():
        assert r is not None
        if n <= 2:
            assert r[2] == n, (scale, default, r)  # CG ends after n steps
        else:
            assert r[2] == iters
    if n == 1:
        _, _, a, b, g, k = ctx.eigs_cg(M, 6)
        assert g[1] == 0.0 and np.all(a[1:] == 0.0) and np.all(b == 0.0)  # alpha, beta = 0 where the divisor is
    M.free()


# ---- 2. storage forms -----------------------------------------------------------------
def test_7pt_default_form(amg, oracle, ctx):
    A = cached(("eigs_lap", 16), lambda: oracle.laplace_7pt(16))
    M = ctx.csr(A.nrows, A.ncols, A.rowptr, A.col, A.val)
    assert M.master_pattern != 0 and M.plane_march == 0  # 256-row planes: the master-pattern kernel
    res = both_scales(amg, oracle, ctx, M, A, 20, "16^3")
    emax = res[1, True][0]
    assert 1.9 < emax < 2.0  # D^-1 A of the 7-pt operator: below 2
    assert ctx.optimal_jacobi_weight(M, 20) == 1.0 / emax
    assert ctx.optimal_jacobi_weight(M) == 1.0 / emax  # 20 iterations by default
    M.free()


def test_plane_marched(amg, oracle, ctx):
    """32 x 16 x 8: the smallest box whose planes (512 rows) the marching kernel takes"""
    A = oracle.laplace_7pt(32, 16, 8)
    M = ctx.csr(A.nrows, A.ncols, A.rowptr, A.col, A.val)
    assert M.plane_march == 512 and M.march_points == 7
    both_scales(amg, oracle, ctx, M, A, 10, "32x16x8 marched")
    M.free()


def random_symmetric(oracle, n, seed=11):
    """a symmetrised random pattern with ragged rows, distinct values, strictly diagonally dominant"""
    g = np.random.default_rng(seed)
    off = {}
    for i in range(n):
        for j in g.integers(0, n, size=int(g.integers(0, 9))).tolist():
            if i != j:
                off[min(i, j), max(i, j)] = g.uniform(-1.0, 1.0)
    rows = [[] for _ in range(n)]
    for (i, j), v in sorted(off.items()):
        rows[i].append((j, v))
        rows[j].append((i, v))
    rp, col, val = [0], [], []
    for i, r in enumerate(rows):
        col.append(i)
        val.append(1.0 + g.uniform(0.0, 1.0) + sum(abs(v) for _, v in r))
        for j, v in sorted(r):
            col.append(j)
            val.append(v)
        rp.append(len(col))
    return oracle.Csr(n, n, np.array(rp), np.array(col, dtype=np.int32), np.array(val))


def test_random_plain_csr(amg, oracle, ctx):
    A = random_symmetric(oracle, 3001)
    M = ctx.csr(A.nrows, A.ncols, A.rowptr, A.col, A.val)
    assert M.value_index == 0 and M.dict_index == 0 and M.row_pattern == 0  # plain CSR
    lens = np.diff(A.rowptr)
    assert lens.min() < 4 and lens.max() > 12
    res = both_scales(amg, oracle, ctx, M, A, 12, "random")
    assert res[1, True][0] < 2.0  # Gershgorin: D^-1 A of a strictly dominant matrix
    M.free()


def test_elasticity_blocks(amg, oracle, ctx):
    """3x3 blocks, a non-uniform diagonal and the identity rows of the fixed dofs"""
    n, rp, cj, v, _ = amg.classical.elasticity(2)
    A = oracle.Csr(n, n, rp, cj, v)
    M = ctx.csr(n, n, rp, cj, v)
    assert M.bsr3 != 0
    d = eigs_ref.diag_of(A)
    assert np.unique(d).size > 2 and np.any((d == 1.0) & (np.diff(A.rowptr) == 1))
    both_scales(amg, oracle, ctx, M, A, 10, "elasticity r=2")
    M.free()


# ---- 3. refusals ----------------------------------------------------------------------
def test_zero_diagonal_is_refused(amg, oracle, ctx):
    A = eigs_ref.tridiag_varied(oracle, 700)
    val = A.val.copy()
    for i in (3, 300, 699):
        val[A.rowptr[i]] = 0.0 if i != 300 else -2.0
    M = ctx.csr(A.nrows, A.ncols, A.rowptr, A.col, val)
    with pytest.raises(amg.AmgError, match=r"status -1: amg_eigs_cg: .*3 row\(s\) with a_ii <= 0"):
        ctx.eigs_cg(M, 5, scale=1)
    B = oracle.Csr(A.nrows, A.ncols, A.rowptr, A.col, val)
    check_case(amg, oracle, ctx, M, B, 5, 0, None, "zero diagonal, unscaled")  # d is not read
    M.free()


def test_bad_arguments(amg, oracle, ctx):
    A = eigs_ref.tridiag_varied(oracle, 10)
    M = ctx.csr(A.nrows, A.ncols, A.rowptr, A.col, A.val)
    for kw in (dict(iters=0), dict(iters=4097), dict(scale=2)):
        with pytest.raises(amg.AmgError, match="status -1"):
            ctx.eigs_cg(M, **kw)
    R = ctx.csr(2, 3, [0, 1, 2], [0, 1], [1.0, 1.0])
    with pytest.raises(amg.AmgError, match="square"):
        ctx.eigs_cg(R, 3, 1, np.ones(2))
    with pytest.raises(amg.AmgError, match="no valid iteration"):
        ctx.eigs_cg(M, 4, 1, np.zeros(10))  # gamma_0 = 0
    M.free()
    R.free()


# ---- 4. the running PCG's spectrum ----------------------------------------------------
def test_pcg_eigs(amg, oracle, ctx):
    L, host = cached(("host", 16), lambda: pcg_ref.host_hierarchy(amg, oracle, 16))
    opts = case_opts(amg, "mult_jacobi", num_cycles=8)
    H = pcg_ref.device_hier(amg, ctx, host, opts)
    with pytest.raises(amg.AmgError, match="no PCG state"):
        H.pcg_eigs()
    n = host["A"][0].nrows
    fv, xv = ctx.vec(amg.rhs_rand(0, n)), ctx.vec(np.zeros(n))
    H.pcg_start(fv, xv)
    with pytest.raises(amg.AmgError, match="status -5"):
        H.pcg_eigs()  # no iteration yet
    for done in (1, 3, 8):
        H.pcg_iterate(done - len(H.pcg_scalars()[0]))
        a, b, rho = H.pcg_scalars()
        assert len(a) == done
        emax, emin, k = H.pcg_eigs()
        assert k == done
        assert_bitwise(np.array([emax, emin]), np.array(amg.lanczos_extremes(a, b)), f"after {done}")
        assert_bitwise(np.array([emax, emin]), np.array(eigs_ref.lanczos_extremes(a, b)[:2]), f"model after {done}")
    assert 0.0 < emin < emax < 1.5  # M^-1 A of a V(1,1) cycle with weighted Jacobi
    H.free()
    fv.free()
    xv.free()
