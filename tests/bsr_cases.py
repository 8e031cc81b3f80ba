"""Crafted num_functions = 3 operators for the 3x3 block kernels, and a
restatement of the selection rule of amg_mat_build_bsr3 (csrc/amg_format.hip).

Pure numpy, seeded, no GPU: tests/test_bsr_cases.py pins what the generator
contains, tests/test_gpu_bsr_edges.py runs the kernels on it.

The operator: nb nodes, three dofs per node (rows 3t..3t+2), node t coupled to
nodes t-reach..t+reach (clipped), every row diagonal first and then ascending.
On top of that base graph:

* hubs: block rows of many blocks (255 is the stored count's limit);
* diagonal-only block rows (one block);
* block rows that must stay in CSR form, of four kinds:
    ident    the three rows hold their diagonal only (a fixed dof);
    short    component 1 is one entry short (unequal row lengths);
    shifted  the columns moved one off node alignment, length still 3 x nodes;
    diffset  component 2 names another node set of the same size.

The operator is not an M-matrix and need not be symmetric: it checks layout,
indexing and arithmetic, not convergence.
"""
import numpy as np

KINDS = ("ident", "short", "shifted", "diffset")


class Case:
    """One crafted operator: CSR arrays plus what the generator intended."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def arrays(self):
        return self.n, self.rowptr, self.col, self.val


def _node_sets(nb, reach, hubs, diag_only, g):
    sets = []
    for t in range(nb):
        if t in diag_only:
            sets.append([t])
            continue
        J = list(range(max(0, t - reach), min(nb, t + reach + 1)))
        if t in hubs:
            rest = np.setdiff1d(np.arange(nb), J)
            J = sorted(J + g.choice(rest, size=hubs[t] - len(J), replace=False).tolist())
        sets.append(J)
    return sets


def _rows_of(t, J, kind, nb):
    """Column lists (diagonal first, then ascending) of block row t's three rows."""
    n = 3 * nb
    full = [3 * j + cc for j in J for cc in range(3)]
    rows = []
    for c in range(3):
        r = 3 * t + c
        cols = full
        if kind == "ident":
            cols = [r]
        elif kind == "shifted":
            # one column off alignment; both shifts keep every diagonal inside for an interior t
            sh = 1 if full[-1] + 1 < n else -1
            cols = [x + sh for x in full]
        elif kind == "diffset" and c == 2:
            # swap the node farthest from t for its outside neighbour
            out = J[-1] + 1 if J[-1] + 1 < nb else J[0] - 1
            drop = J[-1] if out > J[-1] else J[0]
            cols = sorted(3 * j + cc for j in [x for x in J if x != drop] + [out] for cc in range(3))
        assert r in cols, (t, kind)
        cols = [r] + [x for x in cols if x != r]
        if kind == "short" and c == 1:
            cols = cols[:-1]
        rows.append(cols)
    return rows


def build(nb, reach=5, hubs=None, diag_only=(), csr_kinds=None, values="table", diag="table", seed=2024,
          zero_diag_rows=(), extra_rows=0):
    """The crafted operator.

    hubs {node: blocks}; diag_only nodes; csr_kinds {node: kind}; values
    'table' (100 values with 0.0 and -0.0, diagonals 4 + |table value|) or
    'cont' (continuous draws); diag 'table' or a number (every diagonal that
    value); zero_diag_rows: rows whose diagonal is then set to 0.0;
    extra_rows: identity rows appended after the nodes (n % 3 != 0)."""
    hubs = dict(hubs or {})
    csr_kinds = dict(csr_kinds or {})
    g = np.random.default_rng(seed)
    sets = _node_sets(nb, reach, hubs, set(diag_only), g)
    rows = []
    for t in range(nb):
        rows += _rows_of(t, sets[t], csr_kinds.get(t), nb)
    n = 3 * nb + extra_rows
    rows += [[r] for r in range(3 * nb, n)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    col = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows])
    gv = np.random.default_rng(seed + 1)
    table = np.concatenate([[0.0, -0.0], gv.uniform(-1.0, 1.0, 98)])
    if values == "table":
        val = table[gv.integers(0, table.size, col.size)]
        dv = 4.0 + np.abs(table[gv.integers(0, table.size, n)])
    else:
        val = gv.uniform(-1.0, 1.0, col.size)
        dv = 4.0 + np.abs(gv.uniform(-1.0, 1.0, n))
    if diag != "table":
        dv = np.full(n, float(diag))
    val[rowptr[:-1]] = dv
    for r in zero_diag_rows:
        val[rowptr[r]] = 0.0
    return Case(nb=nb, n=n, rowptr=rowptr, col=col, val=val, hubs=hubs, diag_only=tuple(diag_only),
                csr_kinds=csr_kinds, table=table, zero_diag_rows=tuple(zero_diag_rows))


# ---- the main case and its variants ------------------------------------------------------------
NB = 1291            # 1291 % 21 = 10, 1291 % 64 = 11: the last slice is partial in both forms
NB_ALIGNED = 1344    # a multiple of 21 and of 64
HUB, HUB_LAST_BLOCKS = 500, 130
DIAG_ONLY = (7, 640)
SHORT, SHIFTED, DIFFSET = (150, 900), (300,), (1100,)
RUNS = ((21, 42), (704, 768))  # a whole 21-slice; a whole 64-slice and two whole 21-slices


def main_kinds(nb):
    kinds = {t: "ident" for t in range(6, nb, 97)}  # nodes 0..5 block: the diagonal block first .. sixth
    kinds.update({t: "short" for t in SHORT})
    kinds.update({t: "shifted" for t in SHIFTED})
    kinds.update({t: "diffset" for t in DIFFSET})
    for lo, hi in RUNS:  # every kind inside the all-CSR slices
        kinds.update({t: KINDS[t % 4] for t in range(lo, hi)})
    return kinds


# zero diagonals of variant 'zerodiag': blocked rows (an ordinary one, the 255-block hub, the
# partial last slice) and CSR-form rows that are not identity rows (short, shifted, inside a run)
ZERO_DIAG_ROWS = (3 * 250 + 1, 3 * HUB + 0, 3 * 1288 + 2, 3 * 150 + 0, 3 * 300 + 2, 3 * 29 + 1, 3 * 731 + 0)
BROKEN_DIAG_ROW = 3 * 911 + 1  # variant 'unidiag_broken': this diagonal is 5.0, the rest 6.0
VARIANTS = ("main", "cont", "unidiag", "unidiag_broken", "zerodiag", "aligned")


def make(variant="main"):
    """main: 199 distinct values (value-indexed);  cont: continuous values (fp64 blocks);
    unidiag: every diagonal 6.0 (the fast division);  unidiag_broken: one of them 5.0;
    zerodiag: a few zero diagonals;  aligned: nb a multiple of both slice sizes."""
    assert variant in VARIANTS, variant
    nb = NB_ALIGNED if variant == "aligned" else NB
    kw = dict(hubs={HUB: 255, nb - 1: HUB_LAST_BLOCKS}, diag_only=DIAG_ONLY, csr_kinds=main_kinds(nb))
    if variant == "cont":
        kw["values"] = "cont"
    if variant.startswith("unidiag"):
        kw["diag"] = 6.0
    if variant == "zerodiag":
        kw["zero_diag_rows"] = ZERO_DIAG_ROWS
    A = build(nb, **kw)
    if variant == "unidiag_broken":
        A.val[A.rowptr[BROKEN_DIAG_ROW]] = 5.0
    A.variant = variant
    return A


def boundary(which):
    """Small operators on the selection boundaries: (Case, diag_first flag)."""
    every = lambda nb, k: {int(t): "ident" for t in np.linspace(3, nb - 4, k).astype(int)}
    if which == "ninety_exact":      # 90 of 100 block rows block: blocked * 10 == 9 * nb
        return build(100, csr_kinds=every(100, 10)), 1
    if which == "ninety_below":      # 89 of 100
        return build(100, csr_kinds=every(100, 11)), 1
    if which == "sparse":            # t-3..t+3: every block row blocks, but nnz < 24 n
        return build(100, reach=3), 1
    # node 155 holds its diagonal block only and shares a slice (of 21 and of 64) with the hub
    if which == "hub255":
        return build(300, hubs={150: 255}, diag_only=(155,)), 1
    if which == "hub256":            # one block row over the stored count's limit: all CSR
        return build(300, hubs={150: 256}, diag_only=(155,)), 1
    if which == "not_mod3":          # one more row: n % 3 == 1
        return build(100, extra_rows=1), 1
    if which == "not_diag_first":    # registered with diag_first = 0
        return build(100), 0
    raise KeyError(which)


BOUNDARIES = ("ninety_exact", "ninety_below", "sparse", "hub255", "hub256", "not_mod3", "not_diag_first")


# ---- build_bsr3's selection rule, restated -----------------------------------------------------
def block_row_nodes(rowptr, col, t):
    """The node set of block row t when it blocks (its three rows are equally
    long, each diagonal first then strictly ascending, and hold exactly the
    columns 3j, 3j+1, 3j+2 of one common node set), else None."""
    want = None
    for c in range(3):
        r = 3 * t + c
        cols = col[rowptr[r]:rowptr[r + 1]].astype(np.int64)
        if cols.size < 3 or cols.size % 3 or cols[0] != r:
            return None
        rest = cols[1:]
        if np.any(np.diff(rest) <= 0) or np.any(rest == r):
            return None
        full = np.sort(cols)
        nodes = full[::3] // 3
        if not np.array_equal(full, (3 * nodes[:, None] + np.arange(3)).ravel()):
            return None
        if want is None:
            want = nodes
        elif not np.array_equal(want, nodes):
            return None
    return want


def bsr3_counts(n, ncols, rowptr, col, diag_first=1, enabled=True):
    """Per block row the stored block count (0: the block row stays in CSR
    form), or None when the whole matrix stays CSR."""
    nnz = int(rowptr[n])
    if not enabled or n % 3 or n != ncols or not diag_first or n < 3 or nnz < 24 * n:
        return None
    nb = n // 3
    counts = np.zeros(nb, dtype=np.int64)
    for t in range(nb):
        nodes = block_row_nodes(rowptr, col, t)
        if nodes is not None:
            assert t in nodes
            counts[t] = nodes.size
    if int(np.count_nonzero(counts)) * 10 < 9 * nb:  # fewer than 90% of the block rows block
        return None
    if counts.max() > 255:
        return None
    return counts.astype(np.uint8)


def distinct_values(val):
    return int(np.unique(np.ascontiguousarray(val, dtype=np.float64).view(np.uint64)).size)


def bsr3_form(counts, val, ctx_form=2, value_index=1):
    """(amg_mat_bsr3, amg_mat_bsr3_slice) of a registration under amg_set_bsr3(ctx_form)
    and amg_set_value_index(value_index)."""
    if counts is None or not ctx_form:
        return 0, 0
    vi = bool(value_index) and distinct_values(val) <= 256
    return (1, 64 if ctx_form == 2 else 21) if vi else (2, 21)


def all_csr_slices(counts, sl):
    """Slices (of sl block rows) made only of CSR-form block rows."""
    nb = counts.size
    return [s for s in range((nb + sl - 1) // sl) if not np.any(counts[s * sl:min(nb, (s + 1) * sl)])]
