"""format_ref's restatement of the compressed forms' rules on matrices small
enough to count by hand, and at each rule's gate."""
from types import SimpleNamespace

import numpy as np

import format_ref


def csr(rows):
    """host CSR from per-row lists of (column, value)"""
    rp = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    cj = np.array([c for r in rows for c, _ in r], dtype=np.int32)
    cv = np.array([v for r in rows for _, v in r], dtype=np.float64)
    return SimpleNamespace(nrows=len(rows), ncols=len(rows), rowptr=rp, col=cj, val=cv)


def test_tridiagonal_counts():
    A = csr([[(0, 2.0), (1, -1.0)], [(1, 2.0), (0, -1.0), (2, -1.0)], [(2, 2.0), (1, -1.0)]])
    assert format_ref.value_count(A) == 2 and format_ref.value_index(A) == 2
    assert format_ref.dict_pairs(A) == 3 and format_ref.dict_index(A) == 3  # (0, 2), (1, -1), (-1, -1)
    assert format_ref.row_patterns(A) == 3 and format_ref.row_pattern(A, True) == 3
    assert format_ref.row_pattern(A, False) == 0
    assert format_ref.pair_patterns(A) == (2, True)  # rows (0, 1) and the single last row


def test_value_gates():
    many = csr([[(0, float(k))] for k in range(257)])
    assert format_ref.value_count(many) == 257 and format_ref.value_index(many) == 0
    assert format_ref.value_index(csr([[(0, float(k))] for k in range(256)])) == 256
    empty = csr([[], []])
    assert format_ref.value_index(empty) == 0 and format_ref.dict_index(empty) == 0
    assert format_ref.row_pattern(empty, False) == 0


def test_empty_marker_value_turns_the_index_off():
    """the all-ones bit pattern (a NaN) is the hash table's empty marker: no value index, so no form"""
    marker = np.uint64(2 ** 64 - 1).view(np.float64)
    for at in (0, 3, 6):
        rows = [[(0, 2.0), (1, -1.0)], [(1, 2.0), (0, -1.0), (2, -1.0)], [(2, 2.0), (1, -1.0)]]
        flat = [(i, j) for i, r in enumerate(rows) for j in range(len(r))]
        i, j = flat[at]
        rows[i][j] = (rows[i][j][0], marker)
        A = csr(rows)
        assert format_ref.value_count(A) == 3
        assert format_ref.value_index(A) == 0 and format_ref.dict_index(A) == 0
    # another NaN is a value like any other
    A = csr([[(0, 2.0), (1, np.nan)], [(1, 2.0)]])
    assert format_ref.value_index(A) == 2


def test_dictionary_and_row_gates():
    long_row = csr([[(0, 1.0)] + [(c, 2.0) for c in range(1, 32)]] + [[(i, 1.0)] for i in range(1, 40)])
    assert np.diff(long_row.rowptr).max() == format_ref.DC_MAXROW and format_ref.dict_index(long_row) == 32
    long_row = csr([[(0, 1.0)] + [(c, 2.0) for c in range(1, 33)]] + [[(i, 1.0)] for i in range(1, 40)])
    assert np.diff(long_row.rowptr).max() == format_ref.DC_MAXROW + 1 and format_ref.dict_index(long_row) == 0
    hole = csr([[(0, 1.0)], [], [(2, 1.0)]])
    assert format_ref.dict_index(hole) == 1 and format_ref.row_patterns(hole) == 2
    assert format_ref.row_pattern(hole, True) == 0  # an empty row
