"""Numpy restatement of which compressed forms a registered matrix takes.

A host CSR `A` (nrows, rowptr, col, val) in, the counts that the form getters of
the registered matrix report out.  Every function restates one rung of the
ladder from the matrix alone: value index, (offset, value)
dictionary, row patterns, paired-row patterns.
"""
import numpy as np

MAX_KEYS = 256     # a form's table holds at most this many keys
DC_MAXROW = 32     # longest row of a dictionary-coded matrix (AMG_DC_MAXROW)


def _row(A, i):
    """row i as (columns relative to its first column, value bit patterns)"""
    b, e = A.rowptr[i], A.rowptr[i + 1]
    c = A.col[b:e].astype(np.int64)
    return (c - c[0] if c.size else c), A.val[b:e].view(np.int64)


def value_count(A):
    """distinct values by bit pattern"""
    return int(np.unique(A.val.view(np.int64)).size)


def value_index(A):
    """value_index getter: the table size, 0 above MAX_KEYS values, for no entry
    at all, or when some value has the all-ones bit pattern (the hash table's
    empty marker)"""
    if np.any(A.val.view(np.int64) == -1):
        return 0
    nd = value_count(A)
    return nd if nd <= MAX_KEYS else 0


def dict_pairs(A):
    """distinct (column - the row's first column, value) pairs"""
    if A.col.size == 0:
        return 0
    lens = np.diff(A.rowptr)
    first = np.repeat(A.col[A.rowptr[:-1][lens > 0]], lens[lens > 0]).astype(np.int64)
    keys = np.stack([A.col.astype(np.int64) - first, A.val.view(np.int64)], axis=1)
    return int(np.unique(keys, axis=0).shape[0])


def dict_index(A):
    """dict_index getter: on top of the value index, at most MAX_KEYS pairs and
    no row longer than DC_MAXROW"""
    n = dict_pairs(A)
    ok = value_index(A) > 0 and 1 <= n <= MAX_KEYS and np.diff(A.rowptr).max(initial=0) <= DC_MAXROW
    return n if ok else 0


def row_patterns(A):
    """distinct rows, a row being its sequence of (column - first column, value) pairs"""
    pats = set()
    for i in range(A.nrows):
        c, v = _row(A, i)
        pats.add(tuple(c.tolist()) + tuple(v.tolist()) if c.size else ())
    return len(pats)


def row_pattern(A, dict_on):
    """row_pattern getter of a matrix whose dictionary form is on (dict_on):
    no empty row and at most MAX_KEYS distinct rows"""
    n = row_patterns(A)
    ok = dict_on and A.nrows > 0 and np.all(np.diff(A.rowptr) > 0) and n <= MAX_KEYS
    return n if ok else 0


def pair_patterns(A):
    """(distinct row pairs, pair-coded?) of a row-pattern-coded matrix with rows:
    pairs are (pattern of row 2t, pattern of row 2t+1, anchor delta in [-8, 8)),
    the anchor a row's first column; coded with rows of <= 32 entries, <= 256
    pairs whose table (17 words per pair for rows of <= 8 entries, 65 for <= 32)
    fits 32 KiB of LDS, and merged lists at most 1.15 times the longer rows"""
    lens = np.diff(A.rowptr)
    anch = A.col[A.rowptr[:-1]].astype(np.int64)
    # every row starts at its own index: no anchor array (square, or a slab)
    anch_is_row = bool(np.all(anch == np.arange(A.nrows)))
    pat = []
    for i in range(A.nrows):
        c, v = _row(A, i)
        pat.append(tuple(c.tolist()) + tuple(v.tolist()))
    pairs, da_ok = set(), True
    # a row's entries as (column relative to its anchor) for the merge test
    rel = [tuple(_row(A, i)[0].tolist()) for i in range(A.nrows)]
    for t in range((A.nrows + 1) // 2):
        if 2 * t + 1 < A.nrows:
            da = int(anch[2 * t + 1] - anch[2 * t])
            da_ok &= -8 <= da < 8
            pairs.add((pat[2 * t], pat[2 * t + 1], da))
        else:
            pairs.add((pat[2 * t], None, 0))
    stride = 17 if lens.max() <= 8 else 65
    # merged list = shortest common supersequence: la + lb - LCS, entries
    # matched when row 2t+1's column is row 2t's + 1 (anchor delta da)
    merged = single = 0
    seen = {}
    for t in range(A.nrows // 2):
        key = (pat[2 * t], pat[2 * t + 1], int(anch[2 * t + 1] - anch[2 * t]))
        if key in seen:  # counted over all row pairs
            merged += seen[key][0]
            single += seen[key][1]
            continue
        ra, rb_ = rel[2 * t], rel[2 * t + 1]
        da = key[2] if not anch_is_row else 1
        L = np.zeros((len(ra) + 1, len(rb_) + 1), dtype=np.int64)
        for i in range(len(ra) - 1, -1, -1):
            for j in range(len(rb_) - 1, -1, -1):
                L[i, j] = L[i + 1, j + 1] + 1 if rb_[j] + da == ra[i] + 1 else max(L[i + 1, j], L[i, j + 1])
        seen[key] = (len(ra) + len(rb_) - L[0, 0], max(len(ra), len(rb_)))
        merged += seen[key][0]
        single += seen[key][1]
    ok = (da_ok and lens.max() <= 32 and len(pairs) <= 256 and len(pairs) * stride * 4 <= 32768
          and merged <= 1.15 * single)
    return len(pairs), bool(ok)
