"""CPU: the classical setup's phases on their own (amg_csr_strength,
amg_csr_transpose, amg_cf_pmis, amg_classical_interp), host path (device -1):
  * strength against the numpy restatement of test_classical.py;
  * PMIS against a Python restatement of the rule in include/amg_mi355x.h
    (splitmix64 measure, rounds read from the state of the round's start);
  * the four entries chained reproduce cf_marker(0), P_0 and R_0 of a two-level
    ClassicalAMG bit for bit;
  * extended+i / direct interpolation against a Python-float restatement on the
    crafted edge operator below, whose edge cases are asserted present;
  * setup_on_device without a device, and bad operands, are refused.
tests/test_gpu_setup_phases.py holds the device path against this one."""
import numpy as np
import pytest

from test_classical import aniso, strength_np
from test_truncation import DEFAULT_SEED, assert_csr_bitwise, problem

M64 = (1 << 64) - 1


# ---- restatements --------------------------------------------------------------
def splitmix64(x):
    x = (x + 0x9e3779b97f4a7c15) & M64
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & M64
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & M64
    return x ^ (x >> 31)


def transpose_np(n, m, rp, cj):
    """(rowptr, col, source entry) of the transpose: ascending source rows, a
    row's entries in storage order (a stable sort by column)."""
    cj = np.asarray(cj)
    order = np.argsort(cj, kind="stable")
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    trp = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(cj, minlength=m), out=trp[1:])
    return trp, rows[order].astype(np.int32), order


def pmis_np(n, srp, scj, seed):
    """(cf, rounds) by the rule of amg_cf_pmis"""
    trp, tcj, _ = transpose_np(n, n, srp, scj)
    meas = [int(trp[i + 1] - trp[i]) + (splitmix64(seed ^ ((i * 0x2545f4914f6cdd1d) & M64)) >> 11) * 2.0 ** -53
            for i in range(n)]
    cf = [0 if m >= 1.0 else -1 for m in meas]
    nbrs = [np.concatenate((scj[srp[i]:srp[i + 1]], tcj[trp[i]:trp[i + 1]])).tolist() for i in range(n)]
    rounds = 0
    while 0 in cf:
        start = list(cf)
        newc = [i for i in range(n) if start[i] == 0
                and not any(start[j] == 0 and meas[j] >= meas[i] for j in nbrs[i])]
        if not newc:
            break
        for c in newc:
            cf[c] = 1
        for c in newc:
            for j in tcj[trp[c]:trp[c + 1]]:
                if cf[j] == 0:
                    cf[j] = -1
        rounds += 1
    return np.array([-1 if c == 0 else c for c in cf], dtype=np.int32), rounds


def interp_np(n, rp, cj, v, srp, scj, cf, itype, nfun):
    """((rowptr, col, val), facts): the formulas at the head of
    csrc/amg_classical.cpp in Python floats, every sum in storage order.  facts
    per F row i: (|C^_i|, [d_k of the strong F neighbours reached], atil or None)."""
    cidx = np.cumsum(cf == 1) - 1
    rows = [(cj[rp[i]:rp[i + 1]].tolist(), v[rp[i]:rp[i + 1]].tolist()) for i in range(n)]
    S = [scj[srp[i]:srp[i + 1]].tolist() for i in range(n)]

    def first(k, l):
        for c, x in zip(*rows[k]):
            if c == l:
                return x
        return 0.0

    orp, ocj, ov, facts = [0], [], [], {}
    for i in range(n):
        if cf[i] == 1:
            ocj.append(int(cidx[i]))
            ov.append(1.0)
            orp.append(len(ocj))
            continue
        strong = set(S[i])
        chat = {j for j in S[i] if cf[j] == 1}
        if itype == 6:
            for k in S[i]:
                if cf[k] != 1:
                    chat |= {j for j in S[k] if cf[j] == 1}
        num = {j: 0.0 for j in chat}
        aii = first(i, i)
        dks, atil = [], None
        if itype == 3:
            sum_all = sum_c = 0.0
            for j, a in zip(*rows[i]):
                if j == i or j % nfun != i % nfun:
                    continue
                sum_all += a
                if j in chat:
                    num[j] += a
                    sum_c += a
            if sum_c != 0.0 and aii != 0.0:
                alpha = sum_all / sum_c
                for j in sorted(chat):
                    ocj.append(int(cidx[j]))
                    ov.append(-alpha * num[j] / aii)
        else:
            atil = aii
            for j, a in zip(*rows[i]):
                if j == i or j % nfun != i % nfun:
                    continue
                if j in chat:
                    num[j] += a
                elif j in strong and cf[j] == -1:
                    akk = first(j, j)
                    dk = 0.0
                    for l, akl in zip(*rows[j]):
                        if (l == i or l in chat) and akl * akk < 0.0:
                            dk += akl
                    dks.append(dk)
                    if dk == 0.0:
                        atil += a
                        continue
                    for l, akl in zip(*rows[j]):
                        if akl * akk >= 0.0:
                            continue
                        if l == i:
                            atil += a * akl / dk
                        elif l in chat:
                            num[l] += a * akl / dk
                else:
                    atil += a
            if atil != 0.0:
                for j in sorted(chat):
                    ocj.append(int(cidx[j]))
                    ov.append(-num[j] / atil)
        facts[i] = (len(chat), dks, atil)
        orp.append(len(ocj))
    return (np.array(orp, dtype=np.int32), np.array(ocj, dtype=np.int32).reshape(-1),
            np.array(ov, dtype=np.float64).reshape(-1)), facts


# ---- the crafted edge operator -----------------------------------------------------
EDGE_THETA = 0.25
HUBS = (63, 64, 65, 129, 300)


def edge_operator(nfun):
    """(n, rowptr, col, val, cf): a non-symmetric operator of dyadic values whose
    rows hit the setup's edge cases (test_edge_operator_has_its_cases asserts each
    one), with a crafted C/F marker for the interpolation entry.  A g x g
    five-point grid (g = 40 for one function, 30 for three; C on the
    checkerboard) is followed by gadget nodes; with nfun = 3 every node becomes
    three unknowns 3 node + f whose rows are scaled by 1 + f / 4 and strongly
    coupled to the next function (couplings the setup must leave out)."""
    g = np.random.default_rng(2027 + nfun)
    gx = 40 if nfun == 1 else 30
    G = gx * gx
    rows, cf = [], []
    for y in range(gx):
        for x in range(gx):
            i = x + gx * y
            c, w = [i], [4.0 + float(g.integers(0, 5)) / 4.0]
            for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                if 0 <= x + dx < gx and 0 <= y + dy < gx:
                    c.append(i + dx + gx * dy)
                    w.append(float(g.choice([-2.0, -1.0, -0.5, -0.25])))
            rows.append((c, w))
            cf.append(1 if (x + y) % 2 == 0 else -1)
    cgrid = [i for i in range(G) if cf[i] == 1]
    fgrid = [i for i in range(G) if cf[i] == -1]

    def add(cols, vals, mark):
        rows.append((cols, vals))
        cf.append(mark)
        return len(rows) - 1

    add([], [], -1)                                           # empty rows
    add([], [], -1)
    i = len(rows)
    add([i, cgrid[3], fgrid[3]], [4.0, 1.0, 0.5], -1)         # positive off-diagonals: nothing strong
    i = len(rows)
    add([i, cgrid[5], fgrid[5], cgrid[6]], [4.0, -1.0, 2.0, -0.125], -1)  # mixed signs
    i = len(rows)
    add([i, cgrid[8], fgrid[8], cgrid[9]], [-4.0, 1.0, 2.0, -1.0], -1)    # negative diagonal
    i = len(rows)
    add([i, cgrid[11], fgrid[11]], [0.0, -1.0, -1.0], -1)     # stored zero diagonal
    add([cgrid[12], fgrid[12]], [-1.0, -2.0], -1)             # no diagonal at all
    # an F triangle: strong neighbours all F, no C within distance two -> empty P row
    t = len(rows)
    for a in range(3):
        add([t + a, t + (a + 1) % 3, t + (a + 2) % 3], [4.0, -1.0, -2.0], -1)
    # d_k = 0: i (F) -> k (F, strong) and c (C, strong); k's negatives go to F points outside C^_i
    i = len(rows)
    add([i, i + 1, cgrid[20]], [4.0, -1.0, -2.0], -1)
    add([i + 1, fgrid[20], fgrid[21], cgrid[20]], [4.0, -1.0, -1.0, 0.5], -1)
    # atil = 0: 4 - 2 - 2 with one strong C neighbour
    i = len(rows)
    add([i, cgrid[25], fgrid[25], fgrid[26]], [4.0, -8.0, -2.0, -2.0], -1)
    # repeated columns: an off-diagonal twice (strong and weak), the diagonal twice
    i = len(rows)
    add([i, cgrid[30], fgrid[30], cgrid[30], fgrid[31]], [4.0, -2.0, -1.0, -0.25, -2.0], -1)
    i = len(rows)
    add([i, cgrid[33], i, fgrid[33]], [4.0, -1.0, 0.5, -2.0], -1)
    # a row that repeats a column, reached as a strong F neighbour
    i = len(rows)
    add([i, i + 1, cgrid[35]], [4.0, -2.0, -1.0], -1)
    add([i + 1, cgrid[35], cgrid[36], cgrid[35], i], [4.0, -1.0, -2.0, -0.5, -1.0], -1)
    # hubs: k strong neighbours each; the 300 hub's are all C (|C^_i| > 256), the others mixed
    hub = {}
    for k in HUBS:
        i = len(rows)
        pool = cgrid if k == 300 else list(range(G))
        nb = [int(x) for x in g.choice(pool, size=k, replace=False)]
        add([i] + nb, [float(k)] + [-1.0 - float(x % 2) for x in nb], -1)
        hub[k] = i
    # F rows that reach the 129 and the 300 hub as strong F neighbours (rows of several chunks)
    for k in (129, 300):
        i = len(rows)
        add([i, hub[k], cgrid[40], fgrid[40]], [4.0, -2.0, -1.0, -0.25], -1)
    # C points among the gadgets, one with a strong F neighbour
    i = len(rows)
    add([i, t, cgrid[41]], [4.0, -1.0, -1.0], 1)
    N = len(rows)
    if nfun == 1:
        out = rows
    else:
        out = []
        for node in range(N):
            for f in range(nfun):
                c, w = rows[node]
                cc = [nfun * j + f for j in c]
                ww = [x * (1.0 + f / 4.0) for x in w]
                if c:  # another function: half the row scale, strong if it counted
                    mn = min([x for j, x in zip(c, ww) if j != node] + [0.0])
                    cc.append(nfun * node + (f + 1) % nfun)
                    ww.append(0.5 * mn if mn < 0 else -1.0)
                out.append((cc, ww))
        cf = [m for m in cf for _ in range(nfun)]
    rp, cj, cv = [0], [], []
    for c, w in out:
        cj += c
        cv += w
        rp.append(len(cj))
    return (len(out), np.array(rp, dtype=np.int32), np.array(cj, dtype=np.int32), np.array(cv, dtype=np.float64),
            np.array(cf, dtype=np.int32))


@pytest.fixture(scope="module", params=[1, 3])
def edge(request, amg):
    nfun = request.param
    n, rp, cj, v, cf = edge_operator(nfun)
    srp, scj = amg.classical.strength(n, rp, cj, v, EDGE_THETA, num_functions=nfun)
    return dict(nfun=nfun, n=n, rp=rp, cj=cj, v=v, cf=cf, srp=srp, scj=scj)


def test_edge_operator_has_its_cases(amg, edge):
    e = edge
    n, rp, cj, v, cf, srp, scj, nfun = (e[k] for k in ("n", "rp", "cj", "v", "cf", "srp", "scj", "nfun"))
    assert 1500 <= n <= 3000 and n % nfun == 0
    assert set(np.unique(cf)) == {-1, 1}
    ln, sl = np.diff(rp), np.diff(srp)
    row_of = np.repeat(np.arange(n), ln)
    trp, tcj, _ = transpose_np(n, n, srp, scj)
    tl = np.diff(trp)
    isdiag = cj == row_of
    ndiag = np.bincount(row_of[isdiag], minlength=n)
    # the host's diagonal for strength: the last entry of column i
    dlast = np.zeros(n)
    dlast[row_of[isdiag]] = v[isdiag]
    same = (cj % nfun) == (row_of % nfun)
    assert np.any(ln == 0), "empty rows"
    assert np.any((ln > 1) & (sl == 0)), "rows with no strong connection"
    assert np.any(tl == 0) and np.any((tl == 0) & (sl == 0)), "isolated points"
    pos_off = np.bincount(row_of[~isdiag & same & (v > 0)], minlength=n)
    assert np.any((pos_off > 0) & (dlast > 0)), "positive off-diagonals"
    assert np.any(dlast < 0), "negative diagonal"
    assert np.any((ndiag > 0) & (dlast == 0.0) & (sl > 0)), "stored zero diagonal"
    assert np.any((ndiag == 0) & (ln > 0)), "row without a diagonal"
    assert np.any(ndiag == 2), "repeated diagonal"
    rep = [i for i in range(n) if len(set(cj[rp[i]:rp[i + 1]].tolist())) < ln[i]]
    assert len(rep) >= 3 * nfun, "rows that repeat a column"
    strong_f_of = {int(k) for i in range(n) if cf[i] == -1 for k in scj[srp[i]:srp[i + 1]] if cf[k] == -1}
    assert any(k in strong_f_of for k in rep), "a repeated column in a strong F neighbour's row"
    for k in HUBS:
        assert np.any(sl == k), f"a row of {k} strong neighbours"
    if nfun > 1:
        cross = ~same & (v < 0)
        scale = np.minimum.reduceat(np.where(same & ~isdiag, v, 0.0), rp[:-1][ln > 0])
        thr = np.zeros(n)
        thr[ln > 0] = EDGE_THETA * scale
        assert np.any(cross & (v < thr[row_of]) & (dlast[row_of] > 0)), "cross-function couplings that would be strong"
        assert np.all((scj % nfun) == (np.repeat(np.arange(n), sl) % nfun))
    _, facts = interp_np(n, rp, cj, v, srp, scj, cf, 6, nfun)
    F = [i for i in range(n) if cf[i] == -1]
    assert any(sl[i] > 0 and facts[i][0] == 0 and all(cf[k] == -1 for k in scj[srp[i]:srp[i + 1]]) for i in F), \
        "an F row whose strong neighbours are all F without a common C"
    assert any(0.0 in facts[i][1] and facts[i][0] > 0 for i in F), "a strong F neighbour with d_k = 0"
    assert any(facts[i][2] == 0.0 and facts[i][0] > 0 and ndiag[i] > 0 and dlast[i] != 0 for i in F), "atil = 0"
    assert max(facts[i][0] for i in F) > 256, "|C^_i| > 256"
    assert any(facts[i][0] > 64 and len(facts[i][1]) > 0 for i in F), "a long C^_i with strong F neighbours"
    assert any(ln[k] > 128 and k in strong_f_of for k in range(n)), "a strong F neighbour's row of several chunks"


# ---- the host entries ------------------------------------------------------------
def named(amg, oracle, name):
    """(n, rowptr, col, val, theta, num_functions)"""
    if name == "aniso":
        A = aniso(oracle, 40, 0.01)
        return A.nrows, A.rowptr, A.col, A.val, 0.25, 1
    n, rp, cj, v, kw, nfun = problem(amg, oracle, name)
    return n, rp, cj, v, kw["strong_threshold"], nfun


@pytest.mark.parametrize("name", ["lap12", "aniso", "elast2"])
def test_strength_matches_restatement(amg, oracle, name):
    n, rp, cj, v, theta, nfun = named(amg, oracle, name)
    srp, scj = amg.classical.strength(n, rp, cj, v, theta, num_functions=nfun)
    ref = strength_np(oracle.Csr(n, n, rp, cj, v), theta, nfun)
    assert np.array_equal(np.diff(srp), [len(r) for r in ref])
    assert np.array_equal(scj, np.array([j for r in ref for j in r], dtype=np.int32))


def test_strength_on_edge_operator(amg, oracle, edge):
    """rows with one diagonal entry (strength_np sums repeated diagonals, the
    library keeps the last: those rows are pinned by the device comparison)"""
    e = edge
    ref = strength_np(oracle.Csr(e["n"], e["n"], e["rp"], e["cj"], e["v"]), EDGE_THETA, e["nfun"])
    row_of = np.repeat(np.arange(e["n"]), np.diff(e["rp"]))
    once = np.bincount(row_of[e["cj"] == row_of], minlength=e["n"]) <= 1
    for i in np.nonzero(once)[0]:
        assert e["scj"][e["srp"][i]:e["srp"][i + 1]].tolist() == ref[i], i
    # max_row_sum < 1 only ever removes whole rows
    srp2, scj2 = amg.classical.strength(e["n"], e["rp"], e["cj"], e["v"], EDGE_THETA, 0.5, e["nfun"])
    l1, l2 = np.diff(e["srp"]), np.diff(srp2)
    assert np.all((l2 == l1) | (l2 == 0)) and np.any((l2 == 0) & (l1 > 0)) and np.any((l2 > 0))


def test_transpose_matches_restatement(amg, edge):
    e = edge
    trp, tcj, order = transpose_np(e["n"], e["n"], e["rp"], e["cj"])
    got = amg.classical.transpose(e["n"], e["n"], e["rp"], e["cj"], e["v"])
    assert_csr_bitwise(got, (trp, tcj, e["v"][order]), "valued")
    got = amg.classical.transpose(e["n"], e["n"], e["srp"], e["scj"])
    srp_t, scj_t, _ = transpose_np(e["n"], e["n"], e["srp"], e["scj"])
    assert got[2] is None
    assert np.array_equal(got[0], srp_t) and np.array_equal(got[1], scj_t)


@pytest.mark.parametrize("seed", [DEFAULT_SEED, 1, 2 ** 63 + 12345])
def test_pmis_matches_restatement(amg, oracle, edge, seed):
    e = edge
    ref, rounds = pmis_np(e["n"], e["srp"], e["scj"], seed)
    assert rounds >= 2
    assert np.array_equal(amg.classical.pmis(e["n"], e["srp"], e["scj"], seed), ref)
    if e["nfun"] == 1:
        n, rp, cj, v, theta, _ = named(amg, oracle, "lap12")
        srp, scj = amg.classical.strength(n, rp, cj, v, theta)
        assert np.array_equal(amg.classical.pmis(n, srp, scj, seed), pmis_np(n, srp, scj, seed)[0])


@pytest.mark.parametrize("itype", [6, 3])
def test_interp_matches_restatement(amg, edge, itype):
    e = edge
    ref, _ = interp_np(e["n"], e["rp"], e["cj"], e["v"], e["srp"], e["scj"], e["cf"], itype, e["nfun"])
    got = amg.classical.interp(e["n"], e["rp"], e["cj"], e["v"], e["srp"], e["scj"], e["cf"], itype, e["nfun"])
    assert got[0] == e["n"] and got[1] == int((e["cf"] == 1).sum())
    assert_csr_bitwise(got[2:], ref, f"P, interp_type {itype}")


@pytest.mark.parametrize("name", ["lap12", "elast2"])
@pytest.mark.parametrize("ct,it", [(9, 6), (8, 6), (9, 3)])
def test_chained_entries_reproduce_the_setup(amg, oracle, name, ct, it):
    n, rp, cj, v, theta, nfun = named(amg, oracle, name)
    H = amg.classical.ClassicalAMG(n, rp, cj, v, coarsen_type=ct, interp_type=it, strong_threshold=theta,
                                   num_functions=nfun, max_levels=2)
    assert H.L == 2
    cl = amg.classical
    srp, scj = cl.strength(n, rp, cj, v, theta, 1.0, nfun)
    cf = cl.pmis(n, srp, scj, DEFAULT_SEED + (0x9e37 if ct == 8 else 0))
    assert np.array_equal(cf, H.cf_marker(0))
    P = cl.interp(n, rp, cj, v, srp, scj, cf, it, nfun)
    hp, hr = H.get(amg.AMG_GEN_P, 0), H.get(amg.AMG_GEN_R, 0)
    assert P[:2] == hp[:2]
    assert_csr_bitwise(P[2:], hp[2:], "P0")
    assert_csr_bitwise(cl.transpose(P[0], P[1], *P[2:]), hr[2:], "R0")


def test_setup_on_device_needs_a_device(amg, oracle):
    n, rp, cj, v, theta, _ = named(amg, oracle, "lap12")
    assert amg.classical.default_opts().setup_on_device == 0
    with pytest.raises(amg.AmgError, match="setup_on_device"):
        amg.classical.ClassicalAMG(n, rp, cj, v, coarsen_type=9, setup_on_device=1, device=-1)
    with pytest.raises(amg.AmgError, match="setup_on_device"):
        amg.classical.ClassicalAMG(n, rp, cj, v, coarsen_type=9, setup_on_device=2, device=0)


def test_bad_operands_are_refused(amg):
    cl = amg.classical
    rp = np.array([0, 2, 3, 4], dtype=np.int32)
    cj = np.array([0, 1, 1, 2], dtype=np.int32)
    v = np.array([2.0, -1.0, 2.0, 2.0])
    srp, scj = cl.strength(3, rp, cj, v, 0.25)
    assert (srp.tolist(), scj.tolist()) == ([0, 1, 1, 1], [1])
    cf = np.array([-1, 1, -1], dtype=np.int32)
    down = np.array([0, 3, 2, 4], dtype=np.int32)
    far = np.array([0, 1, 3, 2], dtype=np.int32)
    for bad_rp, bad_cj, what in ((down, cj, "rowptr decreases"), (rp, far, "column 3")):
        with pytest.raises(amg.AmgError, match=what):
            cl.strength(3, bad_rp, bad_cj, v, 0.25)
        with pytest.raises(amg.AmgError, match=what):
            cl.transpose(3, 3, bad_rp, bad_cj, v)
        with pytest.raises(amg.AmgError, match=what):
            cl.pmis(3, bad_rp, bad_cj, 1)
        with pytest.raises(amg.AmgError, match=what):
            cl.interp(3, bad_rp, bad_cj, v, srp, scj, cf)
        with pytest.raises(amg.AmgError, match=what):
            cl.interp(3, rp, cj, v, bad_rp, bad_cj, cf)
    with pytest.raises(amg.AmgError, match="column 2"):
        cl.transpose(3, 2, rp, cj)
    with pytest.raises(amg.AmgError, match=r"cf\[2\] = 0"):
        cl.interp(3, rp, cj, v, srp, scj, np.array([-1, 1, 0], dtype=np.int32))
    with pytest.raises(amg.AmgError, match="interp_type"):
        cl.interp(3, rp, cj, v, srp, scj, cf, interp_type=4)
    with pytest.raises(amg.AmgError, match="slots"):
        cl.set_setup_scratch(-1)
    cl.set_setup_scratch(0)
