"""The compressed forms' decisions at their boundaries: 256 against 257 keys of
the (offset, value) dictionary and of the row patterns, a row one entry too
long, and degenerate shapes.  Expected counts come from the numpy restatement
(format_ref); the accepted 256-key matrices give bit-identical SpGEMV and
Jacobi results to plain CSR.

Values with awkward bit patterns: one entry with the pattern of the hash
table's empty marker (all ones) turns the value index off, wherever it stands;
signed zeros, infinities, a subnormal and two NaNs of different payloads are
kept as distinct table entries."""
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


# ---- values with awkward bit patterns ----------------------------------------------------------
MARKER = np.uint64(2 ** 64 - 1).view(np.float64)  # the hash table's empty marker, read as a double


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_empty_marker_value_turns_value_index_off(ctx, oracle, amg, where):
    """The 8^3 7-pt operator with one entry of the all-ones pattern, at entry 0 (a collector
    lane's first value, which its repeat filter used to skip: value_index == 2 and every
    compressed form computing with the largest key instead), in the middle and at the end:
    plain CSR, and SpGEMV and a Jacobi sweep as the same matrix registered with the value index
    off (the entry's rows NaN in both, every other row exact)."""
    L = oracle.laplace_7pt(8)
    val = L.val.copy()
    at = {"first": 0, "middle": val.size // 2, "last": val.size - 1}[where]
    val[at] = MARKER
    A = oracle.Csr(L.nrows, L.ncols, L.rowptr, L.col, val)
    assert format_ref.value_count(A) == 3 and format_ref.value_index(A) == 0
    M = register(ctx, A)
    try:
        print("empty marker", where, forms(M), expected(A))
        assert forms(M) == (0, 0, 0, 0) == expected(A)
        assert M.master_pattern == 0 and M.plane_march == 0 and M.march_points == 0
        check_against_plain(ctx, amg, A, M)
    finally:
        M.free()


NAN_A = np.uint64(0x7FF8000000000001).view(np.float64)
NAN_B = np.uint64(0x7FF8000000000ABC).view(np.float64)
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, NAN_A, NAN_B, -1.0])


def special_operator(oracle, zeros_signed=True):
    """7-pt operator on 12^3 whose off-diagonals cycle, in storage order, through +0.0, -0.0,
    +inf, -inf, the smallest subnormal, two quiet NaNs of different payloads and -1.0"""
    L = oracle.laplace_7pt(12)
    val = L.val.copy()
    off = np.ones(val.size, bool)
    off[L.rowptr[:-1]] = False
    cyc = SPECIAL.copy()
    if not zeros_signed:
        cyc[1] = 0.0
    val[off] = cyc[np.arange(np.count_nonzero(off)) % cyc.size]
    return oracle.Csr(L.nrows, L.ncols, L.rowptr, L.col, val)


SPECIAL_AB = [(1.0, 0.0), (1.0, -1.0), (-1.0, 1.0)]


def special_inputs(n):
    return [("ones", np.ones(n)), ("uniform", np.random.default_rng(12).uniform(-1, 1, n))]


def test_special_values_kept_distinct(ctx, oracle, amg):
    """Every distinct bit pattern is a table entry of its own (9: the eight off-diagonal values
    and the diagonal), and every form gives the plain-CSR SpGEMV bit for bit, a NaN meeting a
    NaN.

    The case does not tell the signed zeros apart: with x = ones or uniform and b = zeros a
    zero product is added to a sum that holds 6 x_i, an infinity or a NaN, where its sign
    cannot show; the oracle's outputs for this operator and for a copy with -0.0 replaced by
    +0.0 are the same bits for every (alpha, beta, x) of the list (computed below and printed,
    not asserted).  That -0.0 and +0.0 are two table entries is what value_index == 9 says.
    No row of these outputs is finite (12 rows are infinite for x = ones, 218 for x = uniform,
    the others NaN): what the comparison can show is a row that should be infinite or NaN and
    is not, or an infinity of the wrong sign."""
    A = special_operator(oracle)
    n = A.nrows
    assert np.unique(SPECIAL.view(np.uint64)).size == 8
    assert format_ref.value_count(A) == 9 == format_ref.value_index(A)
    same, finite = True, []
    Z = special_operator(oracle, zeros_signed=False)
    assert format_ref.value_count(Z) == 8
    for _, x in special_inputs(n):
        for al, be in SPECIAL_AB:
            ya = oracle.smem_spgemv(A, x, np.zeros(n), al, be, np.zeros(n))
            yz = oracle.smem_spgemv(Z, x, np.zeros(n), al, be, np.zeros(n))
            same &= bool(np.all((ya.view(np.uint64) == yz.view(np.uint64)) | (np.isnan(ya) & np.isnan(yz))))
            finite.append(int(np.count_nonzero(np.isfinite(ya))))
    print("signed zeros told apart by the oracle's outputs:", not same, "- finite rows per (x, alpha, beta):", finite)
    regs = []
    try:
        for sw in ({"value_index": 0}, {"dict_index": 0}, {"row_pattern": 0}, {"pair_pattern": 0}, {}):
            for k, v in sw.items():
                getattr(ctx, "set_" + k)(v)
            try:
                regs.append(register(ctx, A))
            finally:
                for k in sw:
                    getattr(ctx, "set_" + k)(1)
        plain, vi_only, dc_only, rp_only, full = regs
        print("special values", [forms(M) for M in regs], expected(A))
        assert forms(plain) == (0, 0, 0, 0)
        for M in regs[1:]:
            assert M.value_index == 9
        assert vi_only.dict_index == 0 and dc_only.dict_index > 0 and dc_only.row_pattern == 0
        assert rp_only.pair_pattern == 0 and forms(full) == expected(A)
        for tag, x in special_inputs(n):
            xv, bv = ctx.vec(x), ctx.vec(n)
            for al, be in SPECIAL_AB:
                ref = oracle.smem_spgemv(A, x, np.zeros(n), al, be, np.zeros(n))
                outs = []
                for M in regs:
                    y = ctx.vec(n)
                    amg.smem.SMEM_SpGEMV(ctx, M, xv, bv, al, be, y, 0, n)
                    outs.append(y.download())
                    y.free()
                assert_bitwise(outs[0], ref, f"plain CSR vs oracle, x {tag}, {al} {be}")
                for k, o in enumerate(outs[1:]):
                    assert_bitwise(o, outs[0], f"form {k + 1} vs plain CSR, x {tag}, {al} {be}")
            xv.free()
            bv.free()
    finally:
        for M in regs:
            M.free()
