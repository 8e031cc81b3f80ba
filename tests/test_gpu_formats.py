"""The compressed forms' decisions at their boundaries: 256 against 257 keys of
the (offset, value) dictionary and of the row patterns, a row one entry too
long, and degenerate shapes.  Expected counts come from the numpy restatement
(format_ref); the accepted 256-key matrices give bit-identical SpGEMV and
Jacobi results to plain CSR.

Not here: a value with the bit pattern of the hash table's empty marker (all
ones).  It is meant to turn the value index off, but a collector lane's repeat
filter starts out holding that very pattern, so a lane whose first new value is
the marker skips it: an 8^3 7-pt operator with one such entry registers with
value_index == 2.  That is a defect of the collector from before this test was
written, to be fixed and pinned together."""
import numpy as np
import pytest

import format_ref
from test_gpu_kernels import assert_bitwise

pytestmark = pytest.mark.gpu


def csr_of_rows(oracle, n, rows):
    """square n x n CSR from per-row lists of (column, value), in the given order"""
    rp = np.cumsum([0] + [len(r) for r in rows])
    cj = np.array([c for r in rows for c, _ in r], dtype=np.int32)
    cv = np.array([v for r in rows for _, v in r], dtype=np.float64)
    return oracle.Csr(n, n, rp, cj, cv)


def dict_boundary(oracle, extra):
    """16 offsets (0, +-1 .. +-7, +8) times 16 values: every (offset, value) pair
    occurs, 256 in all, rows of 16 entries, diagonal first then ascending.
    extra: one row also holds offset +9, the 257th pair."""
    n = 1100  # five workgroups of the collect / encode kernels
    vals = 1.0 + np.arange(16) / 16.0
    offs = [0] + list(range(-7, 0)) + list(range(1, 9))
    rows = []
    for i in range(n):
        r = [(i + o, vals[(i + j) % 16]) for j, o in enumerate(offs) if 0 <= i + o < n]
        if extra and i == 500:
            r.append((i + 9, vals[0]))
        rows.append(r)
    return csr_of_rows(oracle, n, rows)


def row_boundary(oracle, extra):
    """rows = diagonal (4 or 5) + a subset of the offsets 1 .. 7 (value -1): 2 x 128
    = 256 distinct rows of 1 .. 8 entries (8: the hashed row key, fewer: the exact
    one); the last rows, which cannot reach +7, repeat the bare diagonal.
    extra: one row with a third diagonal value, the 257th pattern.  519 rows: odd."""
    n = 519
    rows = []
    for i in range(n):
        mask = i % 128 if i + 7 < n else 0
        diag = 6.0 if (extra and i == 256) else (4.0 if (i // 128) % 2 == 0 else 5.0)
        rows.append([(i, diag)] + [(i + o, -1.0) for o in range(1, 8) if mask >> (o - 1) & 1])
    return csr_of_rows(oracle, n, rows)


def expected(A):
    """the four count getters from the host matrix alone"""
    vi = format_ref.value_index(A)
    dc = format_ref.dict_index(A)
    rp = format_ref.row_pattern(A, dc > 0)
    pp = 0
    if rp:
        npair, ok = format_ref.pair_patterns(A)
        pp = npair if ok else 0
    return vi, dc, rp, pp


def forms(M):
    return M.value_index, M.dict_index, M.row_pattern, M.pair_pattern


def register(ctx, A):
    return ctx.csr(A.nrows, A.ncols, A.rowptr, A.col, A.val)


def check_against_plain(ctx, amg, A, M):
    """SpGEMV and one Jacobi sweep of M, bit for bit those of A registered as plain CSR"""
    ctx.set_value_index(0)
    plain = register(ctx, A)
    ctx.set_value_index(1)
    assert forms(plain) == (0, 0, 0, 0) and plain.master_pattern == 0 and plain.plane_march == 0
    g = np.random.default_rng(11)
    x, b, u0 = (g.uniform(-1, 1, A.nrows) for _ in range(3))
    outs = []
    for m in (plain, M):
        y = ctx.vec(A.nrows)
        amg.smem.SMEM_SpGEMV(ctx, m, ctx.vec(x), ctx.vec(b), -1.0, 1.0, y, 0, A.nrows)
        u = ctx.vec(u0)
        amg.smem.SMEM_Sync_Parfor_Jacobi(ctx, m, ctx.vec(b), u, ctx.vec(A.nrows), 1, 0, 0.7)
        outs.append((y.download(), u.download()))
    plain.free()
    assert_bitwise(outs[1][0], outs[0][0], "SpGEMV")
    assert_bitwise(outs[1][1], outs[0][1], "Jacobi")


@pytest.mark.parametrize("extra", [0, 1])
def test_dictionary_boundary(ctx, oracle, amg, extra):
    A = dict_boundary(oracle, extra)
    assert format_ref.value_count(A) == 16 and np.diff(A.rowptr).max() == 16 + extra
    assert format_ref.dict_pairs(A) == 256 + extra
    M = register(ctx, A)
    print("dictionary boundary", extra, forms(M), expected(A))
    assert M.value_index == 16
    assert M.dict_index == (0 if extra else 256)
    # rows of more than 8 entries below the pair-coding size keep the pair form
    # only for the 27-pt march, which this is not
    assert forms(M) == expected(A)[:3] + (0,)
    assert M.master_pattern == 0 and M.plane_march == 0 and M.march_points == 0 and M.bsr3 == 0
    if not extra:
        check_against_plain(ctx, amg, A, M)
    M.free()


@pytest.mark.parametrize("extra", [0, 1])
def test_row_pattern_boundary(ctx, oracle, amg, extra):
    A = row_boundary(oracle, extra)
    assert format_ref.row_patterns(A) == 256 + extra and np.diff(A.rowptr).max() == 8
    assert format_ref.dict_index(A) == 9 + extra
    M = register(ctx, A)
    print("row-pattern boundary", extra, forms(M), expected(A))
    assert M.dict_index == 9 + extra
    assert M.row_pattern == (0 if extra else 256)
    assert forms(M) == expected(A)
    assert M.plane_march == 0 and M.bsr3 == 0
    if not extra:
        check_against_plain(ctx, amg, A, M)
    M.free()


def test_row_one_entry_too_long(ctx, oracle):
    """one row of AMG_DC_MAXROW + 1 entries in a 7-pt operator: no dictionary"""
    L = oracle.laplace_7pt(12)
    rows = [list(zip(L.col[L.rowptr[i]:L.rowptr[i + 1]].tolist(), L.val[L.rowptr[i]:L.rowptr[i + 1]].tolist()))
            for i in range(L.nrows)]
    i = 800
    rows[i] = [rows[i][0]] + [(c, -1.0) for c in range(100, 100 + 2 * 32, 2)]
    A = csr_of_rows(oracle, L.nrows, rows)
    assert np.diff(A.rowptr).max() == format_ref.DC_MAXROW + 1 and format_ref.dict_pairs(A) <= 256
    M = register(ctx, A)
    print("long row", forms(M), expected(A))
    assert forms(M) == (2, 0, 0, 0) == expected(A)
    assert M.master_pattern == 0 and M.plane_march == 0
    M.free()


def degenerate(oracle, name):
    if name == "no_entries":
        return oracle.Csr(5, 5, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0))
    if name == "one_row":
        return csr_of_rows(oracle, 1, [[(0, 2.0)]])
    # three rows: the last pair holds one row
    return csr_of_rows(oracle, 3, [[(0, 2.0), (1, -1.0)], [(1, 2.0), (0, -1.0), (2, -1.0)], [(2, 2.0), (1, -1.0)]])


@pytest.mark.parametrize("name", ["no_entries", "one_row", "three_rows"])
def test_degenerate_shapes(ctx, oracle, name):
    A = degenerate(oracle, name)
    M = register(ctx, A)
    print(name, forms(M), expected(A), M.master_pattern)
    assert (M.nrows, M.ncols, M.nnz) == (A.nrows, A.ncols, A.nnz)
    assert forms(M) == expected(A)
    if name == "no_entries":
        assert forms(M) == (0, 0, 0, 0) and M.master_pattern == 0
    assert M.pair_anchor16 == 0 and M.plane_march == 0 and M.march_points == 0 and M.bsr3 == 0
    M.free()
