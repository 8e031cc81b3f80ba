"""CPU: the crafted block operators of tests/bsr_cases.py hold every case the
GPU suite (tests/test_gpu_bsr_edges.py) relies on.  If an edit of the generator
loses a case, this file fails rather than the GPU suite quietly testing less.

Everything is asserted on the restated selection rule (bsr_cases.bsr3_counts),
which the GPU suite in turn compares with what the device stored."""
import numpy as np
import pytest

import bsr_cases as bc


@pytest.fixture(scope="module")
def cases():
    out = {}
    for v in bc.VARIANTS:
        A = bc.make(v)
        out[v] = (A, bc.bsr3_counts(A.n, A.n, A.rowptr, A.col))
    return out


@pytest.mark.parametrize("variant", bc.VARIANTS)
def test_crafted_cases_present(cases, variant):
    A, cnt = cases[variant]
    nb = A.nb
    assert cnt is not None and cnt.dtype == np.uint8 and cnt.size == nb and A.n == 3 * nb
    assert nb == (1344 if variant == "aligned" else 1291)
    # exactly the intended CSR-form set, 92% blocked, nnz over the 24 n gate
    csr = np.nonzero(cnt == 0)[0]
    assert csr.tolist() == sorted(A.csr_kinds)
    assert csr.size == 103 and 10 * (nb - csr.size) >= 9 * nb
    assert int(A.rowptr[-1]) >= 24 * A.n
    # CSR-form block rows of every kind; the non-identity ones have rows of more than one entry
    inside = lambda t: any(lo <= t < hi for lo, hi in bc.RUNS)
    for k in bc.KINDS:  # every kind on its own among blocked rows, and inside each all-CSR run
        assert any(A.csr_kinds[t] == k and not inside(t) for t in csr), k
        for lo, hi in bc.RUNS:
            assert any(A.csr_kinds[t] == k for t in range(lo, hi)), (k, lo)
    assert sum(A.csr_kinds[t] == "ident" and not inside(t) for t in csr) == 14
    assert [t for t in csr if A.csr_kinds[t] == "short" and not inside(t)] == [150, 900]
    assert [t for t in csr if A.csr_kinds[t] == "shifted" and not inside(t)] == [300]
    assert [t for t in csr if A.csr_kinds[t] == "diffset" and not inside(t)] == [1100]
    assert all(t in A.csr_kinds for lo, hi in bc.RUNS for t in range(lo, hi)) and bc.RUNS == ((21, 42), (704, 768))
    lens = np.diff(A.rowptr).reshape(-1, 3)[:nb]
    for t in csr:
        k = A.csr_kinds[t]
        if k == "ident":
            assert lens[t].tolist() == [1, 1, 1]
        elif k == "short":  # rows of unequal length
            assert lens[t, 0] == lens[t, 2] == lens[t, 1] + 1 and lens[t, 0] % 3 == 0
        else:  # equal lengths divisible by 3: refused for their columns alone
            assert lens[t, 0] == lens[t, 1] == lens[t, 2] >= 9 and lens[t, 0] % 3 == 0
            rows = [np.sort(A.col[A.rowptr[3 * t + c]:A.rowptr[3 * t + c + 1]]) for c in range(3)]
            if k == "shifted":  # not node-aligned
                assert all(r[0] % 3 != 0 for r in rows) and np.array_equal(rows[0], rows[2])
            else:  # node-aligned, but component 2 names another node set
                assert all(np.array_equal(r[::3] % 3, np.zeros(r.size // 3)) for r in rows)
                assert np.array_equal(rows[0], rows[1]) and not np.array_equal(rows[0], rows[2])
    # hubs: 255 blocks (the stored count's limit) and 130 in the last block row
    assert cnt.max() == 255 and cnt[bc.HUB] == 255 and cnt[nb - 1] == 130
    assert sorted(np.nonzero(cnt > 27)[0].tolist()) == [bc.HUB, nb - 1]
    # diagonal-only block rows
    assert np.nonzero(cnt == 1)[0].tolist() == list(bc.DIAG_ONLY) == [7, 640]
    # base graph: 6..11 blocks, the diagonal block at every position from first to last
    assert set(np.unique(cnt).tolist()) == {0, 1, 6, 7, 8, 9, 10, 11, 130, 255}
    pos = set()
    for t in np.nonzero(cnt)[0]:
        nodes = bc.block_row_nodes(A.rowptr, A.col, t)
        pos.add((int(np.searchsorted(nodes, t)), nodes.size))
    assert {(0, 6), (0, 1), (5, 11), (129, 130)} <= pos  # first of several, alone, mid-row, last
    assert {k for k, m in pos if m <= 11} == set(range(6))
    assert any(k > 5 and k < m - 6 and m == 255 for k, m in pos)  # the hub's diagonal block mid-row
    # rows are diagonal first, then ascending
    for r in range(A.n):
        c = A.col[A.rowptr[r]:A.rowptr[r + 1]]
        assert c[0] == r and np.all(np.diff(c[1:]) > 0)
    # slices made only of CSR-form block rows, in both slice sizes
    assert bc.all_csr_slices(cnt, 21) == [1, 34, 35] and bc.all_csr_slices(cnt, 64) == [11]
    # the hubs' slices hold short rows too, padded to the hub's width
    for sl in (21, 64):
        s = bc.HUB // sl
        assert 0 < cnt[s * sl:(s + 1) * sl][cnt[s * sl:(s + 1) * sl] > 0].min() <= 11
    # the last slice: partial in both forms (main) or full (aligned)
    if variant == "aligned":
        assert nb % 21 == 0 and nb % 64 == 0
    else:
        assert nb % 21 == 10 and nb % 64 == 11
    assert (nb - 1) // 21 == (nb + 20) // 21 - 1 and cnt[nb - 1] == 130  # the hub sits in the last slice


def test_slice_mixing_one_block_and_hub():
    """A slice (of 21 and of 64) holding a 1-block row and the 255-block row, which
    pads to the widest: the small hub operator; with 256 blocks nothing is stored."""
    A, _ = bc.boundary("hub255")
    cnt = bc.bsr3_counts(A.n, A.n, A.rowptr, A.col)
    assert cnt[150] == 255 and cnt[155] == 1 and 150 // 21 == 155 // 21 and 150 // 64 == 155 // 64
    # the main case: block row 7 (one block) pads to its slice's 11; the hub's 64-slice holds
    # one CSR-form row (491) among rows padded to 255
    cnt = bc.bsr3_counts(*[bc.make("main").__dict__[k] for k in ("n", "n", "rowptr", "col")])
    assert cnt[0:21].max() == 11 and cnt[7] == 1
    assert cnt[448:512].max() == 255 and np.nonzero(cnt[448:512] == 0)[0].tolist() == [491 - 448]


@pytest.mark.parametrize("variant,nd,vi", [("main", 199, True), ("cont", None, False), ("unidiag", 101, True),
                                            ("unidiag_broken", 102, True), ("zerodiag", 199, True),
                                            ("aligned", 199, True)])
def test_value_counts(cases, variant, nd, vi):
    """The distinct-value count sits on the intended side of 256 (value-indexed blocks or fp64 blocks)."""
    A, cnt = cases[variant]
    n = bc.distinct_values(A.val)
    assert (n <= 256) == vi and (nd is None or n == nd), n
    assert bc.bsr3_form(cnt, A.val, 2, 1) == ((1, 64) if vi else (2, 21))
    assert bc.bsr3_form(cnt, A.val, 1, 1) == ((1, 21) if vi else (2, 21))
    assert bc.bsr3_form(cnt, A.val, 1, 0) == (2, 21) and bc.bsr3_form(cnt, A.val, 0, 0) == (0, 0)
    if vi:  # 0.0 and -0.0 are both stored, as different table entries
        bits = set(A.val.view(np.uint64).tolist())
        assert 0 in bits and (1 << 63) in bits


def test_diagonals(cases):
    d = {v: A.val[A.rowptr[:-1]] for v, (A, _) in cases.items()}
    assert np.all(d["main"] >= 4.0) and np.unique(d["main"]).size == 99
    assert np.all(d["unidiag"] == 6.0)  # CSR-form rows included
    bad = np.nonzero(d["unidiag_broken"] != 6.0)[0]
    assert bad.tolist() == [bc.BROKEN_DIAG_ROW] and d["unidiag_broken"][bad[0]] == 5.0
    A, cnt = cases["zerodiag"]
    z = np.nonzero(d["zerodiag"] == 0.0)[0]
    assert z.tolist() == sorted(bc.ZERO_DIAG_ROWS)
    where = [(int(cnt[r // 3]), A.csr_kinds.get(r // 3)) for r in z]
    assert any(c > 0 for c, _ in where) and (255, None) in where  # blocked rows, the hub among them
    assert {k for c, k in where if c == 0} == {"short", "shifted", "diffset"}  # non-identity CSR-form rows
    assert any(r // 3 >= 1281 for r in z)  # the partial last slice (both forms)
    # off-diagonal values are shared by all table variants: the same structure, other diagonals
    off = np.ones(A.val.size, bool)
    off[A.rowptr[:-1]] = False
    assert np.array_equal(cases["main"][0].val[off].view(np.uint64), A.val[off].view(np.uint64))


@pytest.mark.parametrize("which,blocks", [("ninety_exact", True), ("ninety_below", False), ("sparse", False),
                                          ("hub255", True), ("hub256", False), ("not_mod3", False),
                                          ("not_diag_first", False)])
def test_selection_boundaries(which, blocks):
    A, diag_first = bc.boundary(which)
    cnt = bc.bsr3_counts(A.n, A.n, A.rowptr, A.col, diag_first)
    assert (cnt is not None) == blocks
    nnz = int(A.rowptr[-1])
    # each refusal has one cause alone: the other conditions hold
    if which == "ninety_exact":
        assert A.nb == 100 and np.count_nonzero(cnt) == 90 and nnz >= 24 * A.n
    elif which == "ninety_below":
        assert A.nb == 100 and len(A.csr_kinds) == 11 and nnz >= 24 * A.n
        blocked = sum(bc.block_row_nodes(A.rowptr, A.col, t) is not None for t in range(A.nb))
        assert blocked == 89 and max(np.diff(A.rowptr)) <= 3 * 255
    elif which == "sparse":
        assert nnz < 24 * A.n
        assert all(bc.block_row_nodes(A.rowptr, A.col, t) is not None for t in range(A.nb))
    elif which == "hub255":
        assert cnt.max() == 255 and np.all(cnt > 0) and nnz >= 24 * A.n
    elif which == "hub256":
        assert bc.block_row_nodes(A.rowptr, A.col, 150).size == 256
        assert all(bc.block_row_nodes(A.rowptr, A.col, t) is not None for t in range(A.nb)) and nnz >= 24 * A.n
    elif which == "not_mod3":
        assert A.n % 3 == 1 and nnz >= 24 * A.n
        assert bc.bsr3_counts(A.n - 1, A.n - 1, A.rowptr, A.col) is not None  # without the extra row it blocks
    else:
        assert diag_first == 0 and bc.bsr3_counts(A.n, A.n, A.rowptr, A.col, 1) is not None


def test_rule_other_refusals(cases):
    A, cnt = cases["main"]
    assert bc.bsr3_counts(A.n, A.n, A.rowptr, A.col, enabled=False) is None
    assert bc.bsr3_counts(A.n, A.n + 3, A.rowptr, A.col) is None  # not square
    assert bc.bsr3_form(None, A.val) == (0, 0)
