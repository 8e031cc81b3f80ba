"""CPU: the classical setup's sparse product on its own (amg_csr_spgemm, host
path) and the case table tests/test_gpu_spgemm.py runs on the device.

What is pinned here:
  * the host product, bit for bit against a Python-float restatement
    (spgemm_py) and against oracle.spgemm, on every case of the table;
  * on the dyadic cases (every product and partial sum exactly representable)
    against a dense numpy product, which is neither the library nor the oracle:
    stored values exact, every non-zero stored, pattern = structural pattern;
  * sums that cancel stay stored as +0.0;
  * bad operands are AmgError.
Each generated case asserts the property it exists for, so a case cannot
silently lose its point."""
import numpy as np
import pytest

from test_truncation import assert_csr_bitwise, problem

HASH_MULT = 2654435761  # spgemm_row_k's multiplicative hash (odd)


# ---- restatement and table arithmetic ---------------------------------------
def spgemm_py(A, B):
    """The rule of include/amg_mi355x.h (amg_csr_spgemm), literally: Python
    floats are IEEE doubles; per row a dict, the products of the (A entry,
    B entry) pairs added in storage order, a column's first contribution added
    to 0.0; columns sorted, the diagonal first when the result is square."""
    an, am, arp, acj, av = A
    bn, bm, brp, bcj, bv = B
    assert am == bn
    arp, acj, brp, bcj = (np.asarray(x).tolist() for x in (arp, acj, brp, bcj))
    av, bv = np.asarray(av, dtype=np.float64).tolist(), np.asarray(bv, dtype=np.float64).tolist()
    rp, oc, ov = [0], [], []
    for r in range(an):
        acc = {}
        for ka in range(arp[r], arp[r + 1]):
            k, a = acj[ka], av[ka]
            for kb in range(brp[k], brp[k + 1]):
                c = bcj[kb]
                if c not in acc:
                    acc[c] = 0.0
                acc[c] = acc[c] + a * bv[kb]
        cols = sorted(acc)
        if an == bm and r in acc:
            cols.remove(r)
            cols.insert(0, r)
        oc += cols
        ov += [acc[c] for c in cols]
        rp.append(len(oc))
    return (an, bm, np.array(rp, dtype=np.int32), np.array(oc, dtype=np.int32).reshape(-1),
            np.array(ov, dtype=np.float64).reshape(-1))


def ub_of(A, B):
    """ub[r]: the number of products of row r (the sum of the B rows its A entries name)"""
    an, _, arp, acj, _ = A
    blen = np.diff(np.asarray(B[2], dtype=np.int64))
    rows = np.repeat(np.arange(an), np.diff(arp))
    return np.bincount(rows, weights=blen[np.asarray(acj[:arp[-1]])], minlength=an).astype(np.int64)


def cap_of(ub):
    """table capacity per row, the rule of amg_spgemm.hip's header comment: the
    smallest power of two that is at least 2 ub and at least 2"""
    cap = np.full(len(ub), 2, dtype=np.int64)
    for _ in range(40):
        small = cap < 2 * np.asarray(ub)
        if not small.any():
            break
        cap[small] *= 2
    assert np.all(cap >= 2 * np.asarray(ub)) and np.all(cap & (cap - 1) == 0)
    return cap


def home_slot(cols, cap):
    return ((np.asarray(cols, dtype=np.uint64) * np.uint64(HASH_MULT)) & np.uint64(0xFFFFFFFF)
            & np.uint64(cap - 1)).astype(np.int64)


def batches_of(cap, budget):
    """spgemm_dev's greedy batching: (number of batches, rows whose table alone exceeds the budget)"""
    nb, tot = 0, 0
    for c in cap.tolist():
        if tot == 0 or tot + c > budget:
            nb += 1
            tot = 0
        tot += c
    return nb, int((cap > budget).sum())


# ---- case construction ------------------------------------------------------
def csr_of(nrows, ncols, rows):
    """rows: one (cols, vals) pair per row"""
    rp, cj, cv = [0], [], []
    for c, v in rows:
        assert len(c) == len(v)
        cj += [int(x) for x in c]
        cv += [float(x) for x in v]
        rp.append(len(cj))
    assert len(rows) == nrows and (not cj or (min(cj) >= 0 and max(cj) < ncols))
    return (nrows, ncols, np.array(rp, dtype=np.int32), np.array(cj, dtype=np.int32).reshape(-1),
            np.array(cv, dtype=np.float64).reshape(-1))


def rand_rows(g, nrows, ncols, lo, hi, empty=0.0, dyadic=False):
    """lo..hi distinct columns per row in random (unsorted) order, values uniform
    in (-1, 1) or k / 8 with integer k in [-32, 32]; a fraction of rows empty"""
    rows = []
    for _ in range(nrows):
        k = 0 if g.random() < empty else int(g.integers(lo, hi + 1))
        c = g.choice(ncols, size=k, replace=False)
        v = g.integers(-32, 33, size=k) / 8.0 if dyadic else g.uniform(-1.0, 1.0, size=k)
        rows.append((c.tolist(), v.tolist()))
    return rows


def row_sets(M):
    n, _, rp, cj, _ = M
    return [set(cj[rp[r]:rp[r + 1]].tolist()) for r in range(n)]


def structural_pattern(A, B):
    bs = row_sets(B)
    an, _, arp, acj, _ = A
    return [set().union(*[bs[k] for k in acj[arp[r]:arp[r + 1]].tolist()]) for r in range(an)]


def case_rand():
    g = np.random.default_rng(101)
    A = csr_of(1500, 1200, rand_rows(g, 1500, 1200, 0, 14))
    B = csr_of(1200, 900, rand_rows(g, 1200, 900, 0, 10))
    alen, blen = np.diff(A[2]), np.diff(B[2])
    assert (alen == 0).any() and (blen == 0).any() and alen.max() == 14 and blen.max() == 10
    assert (blen[A[3]] == 0).any(), "no entry of A names an empty row of B"
    return dict(A=A, B=B)


def case_rand_sq():
    g = np.random.default_rng(102)
    A = csr_of(700, 500, rand_rows(g, 700, 500, 0, 10))
    B = csr_of(500, 700, rand_rows(g, 500, 700, 0, 16))
    pat = structural_pattern(A, B)
    with_d = [r for r in range(700) if r in pat[r]]
    moved = [r for r in with_d if min(pat[r]) < r]
    assert len(with_d) >= 10 and len(moved) >= 5, "too few rows with a diagonal to move"
    assert sum(1 for r in range(700) if pat[r] and r not in pat[r]) >= 10, "no row without a diagonal"
    return dict(A=A, B=B, diag_rows=with_d)


def case_empty():
    g = np.random.default_rng(103)
    ra = rand_rows(g, 400, 300, 1, 3, empty=0.4)
    ra[0] = ra[-1] = ([], [])
    A = csr_of(400, 300, ra)
    B = csr_of(300, 350, rand_rows(g, 300, 350, 1, 6, empty=0.4))
    alen, blen = np.diff(A[2]), np.diff(B[2])
    assert alen[0] == 0 and alen[-1] == 0
    assert 0.3 < (alen == 0).mean() < 0.5 and 0.3 < (blen == 0).mean() < 0.5
    pat = structural_pattern(A, B)
    assert any(alen[r] > 0 and not pat[r] for r in range(400)), "no empty row of C from a non-empty row of A"
    return dict(A=A, B=B)


def case_collide():
    """Three rows of C whose forty columns c0 + 4096 j all share one home slot
    (the multiplier is odd, so columns congruent modulo 4096 collide in every
    table of up to 4096 slots): home slots cap - 3 (the chain wraps through
    slot 0), 0 and cap - 1.  Each is reached through 3 entries of A whose rows of
    B overlap (j = 0..19, 10..29 and 15..39: 65 products, a table of 256)."""
    g = np.random.default_rng(104)
    Bm, nfill = 4096 * 40 + 4096, 48
    pieces = (range(0, 20), range(10, 30), range(15, 40))
    ub = sum(len(p) for p in pieces)
    cap = int(cap_of(np.array([ub]))[0])
    assert cap <= 4096
    rb, ra, special = [], [], []
    for target in (cap - 3, 0, cap - 1):
        c0 = next(c for c in range(4096) if home_slot([c], cap)[0] == target)  # brute force
        for p in pieces:
            js = g.permutation(np.array(list(p)))
            rb.append(((c0 + 4096 * js).tolist(), g.uniform(-1.0, 1.0, size=len(js)).tolist()))
        special.append((c0, target))
    nsp = len(rb)
    rb += rand_rows(g, nfill, Bm, 1, 12)
    # filler rows of A first, between and after the crafted ones
    fill = rand_rows(g, 61, nsp + nfill, 1, 6)
    where = (5, 31, 63)
    for r in range(64):
        if r in where:
            i = where.index(r)
            ra.append(([3 * i, 3 * i + 1, 3 * i + 2], g.uniform(-1.0, 1.0, size=3).tolist()))
        else:
            ra.append(fill.pop())
    A, B = csr_of(64, nsp + nfill, ra), csr_of(nsp + nfill, Bm, rb)
    # recomputed from the operands: if the table rule changes, this fails loudly
    caps = cap_of(ub_of(A, B))
    pat = structural_pattern(A, B)
    for r, (c0, target) in zip(where, special):
        assert caps[r] == cap and caps[r] <= 4096
        assert sorted(pat[r]) == [c0 + 4096 * j for j in range(40)]
        assert np.all(home_slot(sorted(pat[r]), int(caps[r])) == target), (r, target)
    assert [t for _, t in special] == [cap - 3, 0, cap - 1]
    return dict(A=A, B=B, rows=where)


def case_hub():
    g = np.random.default_rng(105)
    Bm = 20000
    rb = rand_rows(g, 300, Bm, 40, 40) + rand_rows(g, 300, Bm, 1, 6)
    ra = rand_rows(g, 600, 600, 1, 8)
    for r in (7, 411):
        ra[r] = (g.permutation(300).tolist(), g.uniform(-1.0, 1.0, size=300).tolist())
    A, B = csr_of(600, 600, ra), csr_of(600, Bm, rb)
    ub = ub_of(A, B)
    assert ub[7] == 12000 and ub[411] == 12000
    pat = structural_pattern(A, B)
    assert len(pat[7]) > 5000 and len(pat[411]) > 5000
    rest = np.delete(np.diff(A[2]), [7, 411])
    assert rest.min() >= 1 and rest.max() <= 8
    assert np.all(np.diff(B[2])[:300] == 40)
    return dict(A=A, B=B)


def _with_repeats(g, rows):
    """every row of at least 2 entries gets its first column again at position 2
    and, half of the time when it is long enough, once more at position 4:
    two or three times in the row, never next to itself"""
    out = []
    for c, v in rows:
        c, v = list(c), list(v)
        if len(c) >= 2:
            col = c[0]
            c.insert(2, col)
            v.insert(2, float(g.uniform(-1.0, 1.0)))
            if len(c) >= 4 and g.random() < 0.5:
                c.insert(4, col)
                v.insert(4, float(g.uniform(-1.0, 1.0)))
        out.append((c, v))
    return out


def _repeat_stats(M):
    n, _, rp, cj, _ = M
    rep = adj = 0
    for r in range(n):
        c = cj[rp[r]:rp[r + 1]].tolist()
        rep += len(c) != len(set(c))
        adj += any(x == y for x, y in zip(c, c[1:]))
    return rep, adj


def case_dup():
    g = np.random.default_rng(106)
    A = csr_of(200, 150, _with_repeats(g, rand_rows(g, 200, 150, 0, 7)))
    B = csr_of(150, 180, _with_repeats(g, rand_rows(g, 150, 180, 2, 9)))
    ra, aa = _repeat_stats(A)
    rb, ab = _repeat_stats(B)
    assert rb == 150 and ab == 0, "every row of B repeats a column, never adjacent"
    assert ra >= 100 and aa == 0
    three = sum(1 for r in range(150) if np.bincount(B[3][B[2][r]:B[2][r + 1]]).max() == 3)
    assert three >= 20, "no column three times in a row of B"
    return dict(A=A, B=B)


def case_cancel():
    """Dyadic values; C (120 x 120, square) has entries whose products cancel:
    B rows 2i and 2i + 1 hold column 110 + i with +b and -b, B rows 10..12 hold
    column 115 with 1/2, 1/4 and -3/4; a row of A that names such a group with
    one value sums to exactly +0.0 there.  Rows 110, 111 and 115 cancel on their
    own diagonal.  The random fill keeps to columns below 100 and B rows >= 13."""
    g = np.random.default_rng(107)
    rb = []
    for k in range(13):
        c, v = rand_rows(g, 1, 100, 2, 5, dyadic=True)[0]
        if k < 10:
            if k % 2 == 0:
                b = float(g.integers(1, 33)) / 8.0
            c, v = c + [110 + k // 2], v + [b if k % 2 == 0 else -b]
        else:
            c, v = [115] + c, [(0.5, 0.25, -0.75)[k - 10]] + v
        rb.append((c, v))
    rb += rand_rows(g, 87, 100, 0, 8, dyadic=True)
    ra = [([13 + x for x in c], v) for c, v in rand_rows(g, 120, 87, 0, 8, dyadic=True)]
    zeros = []
    for r, grp in ((3, 0), (17, 1), (40, 5), (64, 2), (110, 0), (111, 1), (115, 5), (119, 4)):
        a = float(g.integers(1, 33)) / 8.0 * (-1.0 if r % 2 else 1.0)
        names = [10, 11, 12] if grp == 5 else [2 * grp, 2 * grp + 1]
        c, v = ra[r]
        # the group's entries spread through the row, not side by side
        for i, k in enumerate(names):
            pos = min(len(c), 2 * i)
            c.insert(pos, k)
            v.insert(pos, a)
        zeros.append((r, 110 + grp))
    A, B = csr_of(120, 100, ra), csr_of(100, 120, rb)
    assert {(110, 110), (111, 111), (115, 115)} <= set(zeros)
    return dict(A=A, B=B, zeros=zeros)


def case_dyadic():
    g = np.random.default_rng(108)
    A = csr_of(300, 250, rand_rows(g, 300, 250, 0, 12, dyadic=True))
    B = csr_of(250, 300, rand_rows(g, 250, 300, 0, 12, dyadic=True))
    for M in (A, B):
        assert np.array_equal(M[4] * 8, np.round(M[4] * 8)) and np.abs(M[4]).max() <= 4.0
        assert np.diff(M[2]).max() == 12
    return dict(A=A, B=B)


def case_lap(amg, oracle):
    """R times (A P) of the 12^3 classical level 0: the shape the setup runs"""
    n, rp, cj, v, kw, _ = problem(amg, oracle, "lap12")
    H = amg.classical.ClassicalAMG(n, rp, cj, v, **kw)
    A, P, R = (H.get(w, 0) for w in (amg.AMG_GEN_A, amg.AMG_GEN_P, amg.AMG_GEN_R))
    AP = oracle.spgemm(oracle.Csr(*A), oracle.Csr(*P))
    return dict(A=R, B=(AP.nrows, AP.ncols, AP.rowptr, AP.col, AP.val), Ac=H.get(amg.AMG_GEN_A, 1))


CASE_NAMES = ["rand", "rand_sq", "empty", "collide", "hub", "dup", "cancel", "dyadic", "lap"]
_cache = {}


def cases(amg, oracle):
    """name -> {"A", "B", ...}: built once per process, never modified"""
    if not _cache:
        for nm in CASE_NAMES:
            fn = globals()["case_" + nm]
            _cache[nm] = fn(amg, oracle) if nm == "lap" else fn()
        for nm, c in _cache.items():
            assert c["A"][1] == c["B"][0], nm
            for M in (c["A"], c["B"]):
                for x in M[2:]:
                    x.setflags(write=False)
    return _cache


def crafted_operator():
    """(n, rowptr, col, val) for the smoothing-factor tests: 1500 rows, a
    symmetric pattern (a 30 x 50 five-point grid plus three hub rows of 65, 129
    and 300 entries, mirrored), the diagonal first and log-uniform over
    [1, 1e4], off-diagonals negative with row i's summing to -0.9 a_ii (strictly
    diagonally dominant), so a_ij and a_ji differ and a_ij / a_ii is not
    a_ij / a_jj."""
    g = np.random.default_rng(109)
    nx, ny = 30, 50
    n = nx * ny
    nb = [set() for _ in range(n)]
    for y in range(ny):
        for x in range(nx):
            i = x + nx * y
            for dx, dy in ((1, 0), (0, 1)):
                if x + dx < nx and y + dy < ny:
                    j = i + dx + nx * dy
                    nb[i].add(j)
                    nb[j].add(i)
    hubs = {97: 65, 700: 129, 1333: 300}
    for h, ln in hubs.items():
        others = [j for j in g.permutation(n).tolist() if j != h and j not in nb[h] and j not in hubs]
        for j in others[:ln - 1 - len(nb[h])]:
            nb[h].add(j)
            nb[j].add(h)
    d = 10.0 ** g.uniform(0.0, 4.0, size=n)
    d[0], d[1] = 1.0, 1e4
    rows = []
    for i in range(n):
        c = sorted(nb[i])
        u = g.uniform(0.5, 1.0, size=len(c))
        rows.append(([i] + c, [d[i]] + (-0.9 * d[i] * u / u.sum()).tolist()))
    _, _, rp, cj, v = csr_of(n, n, rows)
    ln = np.diff(rp)
    assert [int(ln[h]) for h in hubs] == [65, 129, 300]
    assert all(i in nb[j] for i in range(n) for j in nb[i]), "pattern not symmetric"
    diag = v[rp[:-1]]
    assert np.all(cj[rp[:-1]] == np.arange(n)) and diag.min() == 1.0 and diag.max() == 1e4
    off = np.abs(np.add.reduceat(v, rp[:-1]) - diag)
    assert np.all(off < diag)
    return n, rp, cj, v


CRAFTED_KW = dict(coarsen_type=10, strong_threshold=0.25, max_levels=2)


# ---- tests -------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(amg, oracle):
    return cases(amg, oracle)


@pytest.fixture(scope="module")
def host_products(amg, table):
    return {nm: amg.classical.spgemm(c["A"], c["B"]) for nm, c in table.items()}


@pytest.mark.parametrize("name", CASE_NAMES)
def test_host_matches_restatement_and_oracle(amg, oracle, table, host_products, name):
    A, B = table[name]["A"], table[name]["B"]
    got = host_products[name]
    assert (got[0], got[1]) == (A[0], B[1])
    ref = spgemm_py(A, B)
    assert_csr_bitwise(got[2:], ref[2:], f"{name} vs spgemm_py")
    o = oracle.spgemm(oracle.Csr(*A), oracle.Csr(*B))
    assert (o.nrows, o.ncols) == (got[0], got[1])
    assert_csr_bitwise(got[2:], (o.rowptr, o.col, o.val), f"{name} vs oracle")


@pytest.mark.parametrize("name", ["dyadic", "cancel"])
def test_dyadic_against_dense(table, host_products, name):
    A, B = table[name]["A"], table[name]["B"]

    def dense(M):
        n, m, rp, cj, v = M
        D = np.zeros((n, m))
        np.add.at(D, (np.repeat(np.arange(n), np.diff(rp)), cj), v)  # repeated columns add up, exactly
        return D

    D = dense(A) @ dense(B)
    n, m, rp, cj, v = host_products[name]
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert np.array_equal(v, D[rows, cj]), "a stored value is not the exact sum"
    stored = np.zeros((n, m), dtype=bool)
    stored[rows, cj] = True
    assert stored.sum() == len(cj), "a column is stored twice"
    assert not np.any((D != 0) & ~stored), "a non-zero of the product is not stored"
    pat = structural_pattern(A, B)
    got = row_sets(host_products[name])
    assert got == pat, "stored pattern is not the structural pattern"
    if name == "cancel":
        assert all(D[r, c] == 0.0 and stored[r, c] for r, c in table[name]["zeros"])


def test_cancelled_sums_stay(table, host_products):
    n, m, rp, cj, v = host_products["cancel"]
    for r, c in table["cancel"]["zeros"]:
        k = [q for q in range(rp[r], rp[r + 1]) if cj[q] == c]
        assert len(k) == 1, (r, c)
        assert v[k[0]] == 0.0 and not np.signbit(v[k[0]]), (r, c, v[k[0]])
        if r == c:
            assert k[0] == rp[r], "a cancelled diagonal still goes first"


def test_square_result_from_rectangular_operands(table, host_products):
    n, m, rp, cj, v = host_products["rand_sq"]
    assert n == m == 700
    with_d = table["rand_sq"]["diag_rows"]
    for r in range(n):
        c = cj[rp[r]:rp[r + 1]]
        if r in with_d:
            assert c[0] == r and np.all(np.diff(c[1:]) > 0), r
        else:
            assert np.all(np.diff(c) > 0) and r not in c, r


def test_lap_case_is_the_setups_coarse_operator(table, host_products):
    Ac = table["lap"]["Ac"]
    got = host_products["lap"]
    assert (got[0], got[1]) == (Ac[0], Ac[1])
    assert_csr_bitwise(got[2:], Ac[2:], "R (A P) of 12^3")


def test_bad_operands(amg):
    ok = (3, 4, np.array([0, 2, 3, 4]), np.array([0, 3, 1, 2]), np.array([1.0, 2.0, 3.0, 4.0]))
    B = (4, 5, np.array([0, 1, 2, 3, 4]), np.array([0, 4, 2, 1]), np.array([1.0, 2.0, 3.0, 4.0]))
    n, m, rp, cj, v = amg.classical.spgemm(ok, B)
    assert (n, m) == (3, 5) and list(rp) == [0, 2, 3, 4]
    bad = [
        ((3, 4, np.array([0, 3, 2, 4]), ok[3], ok[4]), B, "rowptr decreases"),
        ((3, 4, np.array([1, 2, 3, 4]), ok[3], ok[4]), B, "rowptr"),
        ((3, 4, ok[2], np.array([0, 4, 1, 2]), ok[4]), B, "A: column 4"),
        ((3, 4, ok[2], np.array([0, -1, 1, 2]), ok[4]), B, "A: column -1"),
        (ok, (4, 5, B[2], np.array([0, 5, 2, 1]), B[4]), "B: column 5"),
        (ok, (4, 5, np.array([0, 1, 3, 2, 4]), B[3], B[4]), "B: rowptr decreases"),
        ((0, 4, np.array([0]), np.zeros(0, np.int32), np.zeros(0)), B, "bad argument"),
    ]
    for X, Y, msg in bad:
        with pytest.raises(amg.AmgError, match=msg):
            amg.classical.spgemm(X, Y)
    with pytest.raises(amg.AmgError, match="slots"):
        amg.classical.set_spgemm_scratch(-1)
    amg.classical.set_spgemm_scratch(0)


def test_batch_conditions_of_the_table(table):
    """what tests/test_gpu_spgemm.py relies on at a budget of 256 slots"""
    nb = {}
    for nm in ("rand", "hub", "collide", "empty"):
        cap = cap_of(ub_of(table[nm]["A"], table[nm]["B"]))
        nb[nm] = batches_of(cap, 256)
    print("batches at 256 slots (batches, rows over the budget):", nb)
    assert max(b for b, _ in nb.values()) >= 8
    assert max(o for _, o in nb.values()) >= 1


def test_crafted_operator_smoothed_on_host(amg, oracle):
    """the operator of the device smoothing-factor test coarsens, and the host
    path agrees with the oracle on it (w = 0.8 and w = 1: diagonal factor 0.0)"""
    n, rp, cj, v = crafted_operator()
    H = amg.classical.ClassicalAMG(n, rp, cj, v, **CRAFTED_KW)
    assert H.L == 2
    A, P = oracle.Csr(*H.get(amg.AMG_GEN_A, 0)), oracle.Csr(*H.get(amg.AMG_GEN_P, 0))
    assert 0 < P.ncols < n
    for w in (0.8, 1.0):
        H.smooth_transfers(w)
        ps, rs = oracle.smooth_transfer(A, P, w)
        assert_csr_bitwise(H.get(amg.AMG_GEN_PS, 0)[2:], (ps.rowptr, ps.col, ps.val), f"PS w={w}")
        assert_csr_bitwise(H.get(amg.AMG_GEN_RS, 0)[2:], (rs.rowptr, rs.col, rs.val), f"RS w={w}")
