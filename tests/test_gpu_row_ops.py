"""The row operators' format ladder as a matrix: every storage form of an
operator x every operator (SpMV, SpGEMV in each (alpha, beta) branch, the
two-pass residual, Jacobi, L1 Jacobi) x row ranges that stay on and leave the
pair and march forms.  Every output is bit-identical to the oracle's loops and
to the plain-CSR registration of the same matrix.

A form a matrix does not admit is skipped for it, but each form names one
matrix (ACTIVE) on which the library must report it active, so no rung of the
ladder can go unexercised.
"""
import numpy as np
import pytest

import bsr_cases
from conftest import random_csr, rng
from test_gpu_kernels import assert_bitwise, _vecs

pytestmark = pytest.mark.gpu

P = 512  # the box's plane, the smallest the march admits
# (alpha, beta): every accumulator start x sign / scale branch of the SpGEMV
SPGEMV = [(1, 0), (-1, 0), (2.5, 0), (1, -1), (-1, 1), (0.5, -0.5),
          (1, 1), (-1, -1), (3, 3), (1, 0.3), (-1, 0.7), (1.7, -0.4)]


def _quantise(oracle, A, nv):
    """A's structure with values from nv levels (value-indexed), the diagonal the largest."""
    levels = np.linspace(-1.0, 1.0, nv) * (1.0 + 1.0 / 3.0)
    q = levels[rng(nv).integers(0, nv, size=A.val.size)]
    d = A.rowptr[:-1][np.diff(A.rowptr) > 0]
    q[d] = levels[-1]
    return oracle.Csr(A.nrows, A.ncols, A.rowptr, A.col, q)


def _longrows(oracle):
    """Two rows longer than an LDS chunk among short ones (36 entries per row on average)."""
    g = rng(3)
    n = 600
    rows = []
    for i in range(n):
        k = 5000 if i in (7, 300) else int(g.integers(1, 40))
        rows.append([i] + sorted(set(g.integers(0, n, size=k).tolist()) - {i}))
    rp = np.cumsum([0] + [len(r) for r in rows])
    cj = np.concatenate([np.array(r, dtype=np.int32) for r in rows])
    cv = g.uniform(-1, 1, size=cj.size)
    cv[rp[:-1]] = 50.0
    return oracle.Csr(n, n, rp, cj, cv)


@pytest.fixture(scope="module")
def host(oracle, amg):
    g = amg.Gen(64, 32, 8, interp=amg.AMG_INTERP_LINEAR)
    gal = oracle.Csr(*g.host_csr(amg.AMG_GEN_A, 1))
    g.free()
    assert gal.nrows == 32 * 16 * 4
    n, rp, cj, cv = bsr_cases.make("main").arrays
    return {
        "lap7": oracle.laplace_7pt(32, 16, 4),     # 7-pt box, P = 512
        "gal27": gal,                              # the 27-pt Galerkin operator of a 32 x 16 x 4 box
        "rand_q": _quantise(oracle, random_csr(oracle, 2000, 2000, 9, seed=1, with_zero_diag=True), 256),
        "longrows_q": _quantise(oracle, _longrows(oracle), 37),
        "dense_q": _quantise(oracle, random_csr(oracle, 1100, 1100, 90, seed=7, with_zero_diag=True), 200),
        "bsr": oracle.Csr(n, n, rp, cj, cv),       # 3x3 blocks, 199 distinct values
    }


# form -> the context switches its registration runs under (the rest at their defaults;
# pair_pattern 2 pair-codes long rows at any size); long_form is a launch-time switch
DEFAULTS = dict(value_index=1, dict_index=1, row_pattern=1, pair_pattern=2, master_pattern=1, plane_march=1,
                bsr3=0, long_form=0)
FORMS = {
    "plain": dict(value_index=0),
    "vi": dict(dict_index=0),
    "dict": dict(row_pattern=0),
    "rowpat": dict(pair_pattern=0),
    "pair": dict(master_pattern=0),
    "master": dict(plane_march=0),
    "march7": dict(),
    "march27": dict(),
    "bsr21": dict(bsr3=1),
    "bsr64": dict(bsr3=2),
    "bsr21f": dict(bsr3=1, value_index=0),
    "long0": dict(long_form=0),
    "long1": dict(long_form=1),
    "long2": dict(long_form=2),
}


def _active(amg, form, M):
    """Whether registration M has the form (and none of the forms above it)."""
    sl = amg.lib.amg_mat_bsr3_slice(M.h)
    return {
        "plain": M.value_index == 0 and M.dict_index == 0 and M.bsr3 == 0,
        "vi": M.value_index > 0 and M.dict_index == 0,
        "dict": M.dict_index > 0 and M.row_pattern == 0,
        "rowpat": M.row_pattern > 0 and M.pair_pattern == 0,
        "pair": M.pair_pattern > 0 and M.master_pattern == 0,
        "master": M.master_pattern != 0 and M.plane_march == 0,
        "march7": M.march_points == 7 and M.plane_march == P,
        "march27": M.march_points == 27 and M.plane_march == P,
        "bsr21": M.bsr3 == 1 and sl == 21,
        "bsr64": M.bsr3 == 1 and sl == 64,
        "bsr21f": M.bsr3 == 2 and sl == 21,
        # the long-row rung: at least 64 entries per row, no dictionary
        "long0": M.nnz >= 64 * M.nrows and M.dict_index == 0 and M.value_index > 0,
        "long1": M.nnz >= 64 * M.nrows and M.dict_index == 0 and M.value_index > 0,
        "long2": M.nnz >= 64 * M.nrows and M.dict_index == 0 and M.value_index > 0,
    }[form]


# the matrix on which each form must be active
ACTIVE = {"plain": "lap7", "vi": "rand_q", "dict": "lap7", "rowpat": "lap7", "pair": "lap7", "master": "lap7",
          "march7": "lap7", "march27": "gal27", "bsr21": "bsr", "bsr64": "bsr", "bsr21f": "bsr",
          "long0": "dense_q", "long1": "dense_q", "long2": "dense_q"}
# further (matrix, form) pairs, run where the matrix admits the form
ALSO = [("gal27", f) for f in ("plain", "vi", "dict", "rowpat", "pair", "master")] + \
       [("rand_q", "plain"), ("longrows_q", "plain"), ("longrows_q", "vi"), ("dense_q", "plain"), ("bsr", "plain"),
        ("bsr", "vi")]
CASES = [(m, f) for f, m in ACTIVE.items()] + ALSO


def _register(ctx, A, form):
    k = dict(DEFAULTS, **FORMS[form])
    ctx.set_value_index(k["value_index"])
    ctx.set_dict_index(k["dict_index"])
    ctx.set_row_pattern(k["row_pattern"])
    ctx.set_pair_pattern(k["pair_pattern"])
    ctx.set_master_pattern(k["master_pattern"])
    ctx.set_plane_march(k["plane_march"])
    ctx.set_bsr3(k["bsr3"])
    try:
        return ctx.csr(A.nrows, A.ncols, A.rowptr, A.col, A.val)
    finally:
        ctx.set_value_index(1)
        ctx.set_dict_index(1)
        ctx.set_row_pattern(1)
        ctx.set_pair_pattern(1)
        ctx.set_master_pattern(1)
        ctx.set_plane_march(1)
        ctx.set_bsr3(2)


def _ranges(name, n):
    r = [(0, n), (2, n - 5), (3, n - 6), (P, 3 * P), (P + 2, 3 * P)]
    if name == "bsr":  # whole slices of 21 / of 64 block rows inside the matrix: the block rung on a sub-range
        r += [(63 * 4, 63 * 40), (192 * 2, 192 * 15)]
    return [(a, min(b, n)) for a, b in r]


def _inputs(A):
    n = A.nrows
    return dict(x=_vecs(A.ncols, 40), b=_vecs(n, 41), y0=_vecs(n, 42), r0=_vecs(n, 43))


def _oracle_results(oracle, name, A):
    """Every (operator, range) result of the oracle's loops, computed once per matrix."""
    v = _inputs(A)
    l1 = oracle.l1_norms(A)
    out = {}
    for ns, ne in _ranges(name, A.nrows):
        out["matvec", ns, ne] = oracle.smem_matvec(A, v["x"], v["y0"].copy(), ns, ne)
        for ab in SPGEMV:
            out["spgemv", ab, ns, ne] = oracle.smem_spgemv(A, v["x"], v["b"], ab[0], ab[1], v["y0"].copy(), ns, ne)
        y, r = v["y0"].copy(), v["r0"].copy()
        oracle.smem_residual(A, v["b"], v["x"], y, r, ns, ne)
        out["residual_y", ns, ne], out["residual_r", ns, ne] = y, r
        # amg_jacobi copies the whole u to u_prev, the oracle's slice only [ns, ne): start u_prev = u
        u, up = v["y0"].copy(), v["y0"].copy()
        oracle.smem_jacobi(A, v["b"], u, up, 0.8, 2, 0, ns, ne)
        out["jacobi", ns, ne] = u
        u, up = v["y0"].copy(), v["y0"].copy()
        oracle.smem_l1jacobi(A, v["b"], u, up, l1, 2, 0, ns, ne)
        out["l1_jacobi", ns, ne] = u
    return out


def _gpu_results(ctx, amg, name, A, M):
    v = _inputs(A)
    n = A.nrows
    x, b = ctx.vec(v["x"]), ctx.vec(v["b"])
    l1 = ctx.vec(n)
    amg.smem.L1_row_norm(ctx, M, l1)
    out = {}
    for ns, ne in _ranges(name, n):
        y = ctx.vec(v["y0"])
        amg.smem.SMEM_MatVec(ctx, M, x, y, ns, ne)
        out["matvec", ns, ne] = y.download()
        for ab in SPGEMV:
            y = ctx.vec(v["y0"])
            amg.smem.SMEM_SpGEMV(ctx, M, x, b, ab[0], ab[1], y, ns, ne)
            out["spgemv", ab, ns, ne] = y.download()
        y, r = ctx.vec(v["y0"]), ctx.vec(v["r0"])
        amg.smem.SMEM_Residual(ctx, M, b, x, y, r, ns, ne)
        out["residual_y", ns, ne], out["residual_r", ns, ne] = y.download(), r.download()
        u, up = ctx.vec(v["y0"]), ctx.vec(n)
        amg.smem.SMEM_Sync_Jacobi(ctx, M, b, u, up, 2, 0, 0.8, ns, ne)
        out["jacobi", ns, ne] = u.download()
        u, up = ctx.vec(v["y0"]), ctx.vec(n)
        amg.check(amg.lib.amg_l1_jacobi(ctx.h, M.h, b.h, u.h, up.h, l1.h, 2, 0, ns, ne, 0))
        out["l1_jacobi", ns, ne] = u.download()
    return out


@pytest.fixture(scope="module")
def refs(oracle, ctx, amg, host):
    """Per matrix: the oracle's results and the plain-CSR registration's, shared by every form."""
    cache = {}

    def get(name):
        if name not in cache:
            A = host[name]
            M = _register(ctx, A, "plain")
            assert _active(amg, "plain", M), name
            cache[name] = (_oracle_results(oracle, name, A), _gpu_results(ctx, amg, name, A, M))
            M.free()
        return cache[name]
    return get


@pytest.mark.parametrize("name,form", CASES, ids=[f"{m}-{f}" for m, f in CASES])
def test_row_op_ladder(ctx, amg, host, refs, name, form):
    A = host[name]
    M = _register(ctx, A, form)
    try:
        if ACTIVE[form] == name:
            assert _active(amg, form, M), (name, form, M.value_index, M.dict_index, M.row_pattern, M.pair_pattern,
                                           M.master_pattern, M.plane_march, M.march_points, M.bsr3)
        elif not _active(amg, form, M):
            pytest.skip(f"{name} does not admit {form}")
        ref, plain = refs(name)
        ctx.set_long_form(dict(DEFAULTS, **FORMS[form])["long_form"], 1)
        try:
            got = _gpu_results(ctx, amg, name, A, M)
        finally:
            ctx.set_long_form(0, 1)
        assert got.keys() == ref.keys() == plain.keys()
        for key in ref:
            assert_bitwise(got[key], ref[key], f"{name} {form} {key} against the oracle")
            assert_bitwise(got[key], plain[key], f"{name} {form} {key} against plain CSR")
    finally:
        M.free()
