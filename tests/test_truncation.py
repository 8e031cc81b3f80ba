"""CPU: interpolation truncation (amg_csr_truncate, P_max_elmts / trunc_factor of
the classical setup) and the explicit smoothed transfers
(amg_classical_smooth_transfers with add_P_max_elmts / add_trunc_factor).

The truncation rule restates hypre_BoomerAMGInterpTruncation; hypre is not in
the reference tree, so agreement with hypre is parity unpinned.  What is pinned:
  * the rule, bit for bit against a numpy / Python-float restatement with
    serial sums (trunc_np below), ties to the smaller column;
  * a pass that drops nothing returns its input bit for bit;
  * the truncated hierarchy equals one built level by level from two-level
    setups, trunc_np and the oracle's transpose / Gustavson product;
  * smoothed transfers equal oracle.smooth_transfer bit for bit, and with the
    add_* options P~ is trunc_np of the oracle's P~ and R~ its exact transpose."""
import numpy as np
import pytest

PAIRS = [(0.3, 0), (0.0, 3), (0.2, 4), (0.0, 1)]
DEFAULT_SEED = 2747  # amg_classical_opts_default


def _ssum(xs):
    s = 0.0
    for x in xs:
        s += x
    return s


def trunc_np(n, rowptr, col, val, tf, mx):
    """The rule of include/amg_mi355x.h (amg_csr_truncate), literally: Python
    floats are IEEE doubles, sums run in storage order, one division and one
    multiply per entry."""
    rp, oc, ov = [0], [], []
    for r in range(n):
        c = [int(x) for x in col[rowptr[r]:rowptr[r + 1]]]
        w = [float(x) for x in val[rowptr[r]:rowptr[r + 1]]]
        if tf > 0:
            s = _ssum(w)
            m = max([abs(x) for x in w], default=0.0)
            thr = tf * m
            kept = [i for i in range(len(w)) if not abs(w[i]) < thr]
            c, w = [c[i] for i in kept], [w[i] for i in kept]
            k = _ssum(w)
            if k != 0:
                f = s / k
                w = [x * f for x in w]
        if mx > 0 and len(w) > mx:
            s = _ssum(w)
            order = sorted(range(len(w)), key=lambda i: (-abs(w[i]), c[i], i))
            kept = sorted(order[:mx])
            c, w = [c[i] for i in kept], [w[i] for i in kept]
            k = _ssum(w)
            if k != 0:
                f = s / k
                w = [x * f for x in w]
        oc += c
        ov += w
        rp.append(len(oc))
    return (np.array(rp, dtype=np.int32), np.array(oc, dtype=np.int32).reshape(-1),
            np.array(ov, dtype=np.float64).reshape(-1))


def crafted_rows():
    """(n, rowptr, col, val): an empty row, a single entry, equal magnitudes
    (sorted and unsorted columns: the tie goes to the smaller column, not the
    earlier position), rows whose kept sum is 0 under the threshold and under
    the count pass, rows of 63 / 64 / 65 / 128 / 200 entries (one and several
    wavefront-sized chunks on the device), repeated magnitudes in the long rows."""
    g = np.random.default_rng(7)
    rows = [([], []),
            ([5], [0.75]),
            ([1, 3, 4, 6, 8, 9], [0.5, -0.5, 0.5, 0.5, -0.5, 0.5]),
            ([9, 2, 7, 4, 11, 0], [0.5, -0.5, 0.5, 0.5, -0.5, 0.5]),
            ([0, 1, 2, 3, 4], [3.0, -3.0, 2.0, -2.0, 0.5]),
            ([0, 1, 2, 3, 4], [3.0, -3.0, 2.0, -2.0, 1.9]),
            ([2, 5], [1.0, 1e-3]),
            ([], [])]
    for ln in (63, 64, 65, 128, 200):
        c = np.sort(g.choice(1000, size=ln, replace=False))
        v = g.uniform(-1.0, 1.0, size=ln)
        v[g.integers(0, ln, size=ln // 4)] = 0.25  # ties across chunks
        v[g.integers(0, ln, size=ln // 8)] = -0.25
        rows.append((c.tolist(), v.tolist()))
    rows.append(([3], [1.0]))
    rp, cj, cv = [0], [], []
    for c, v in rows:
        cj += c
        cv += v
        rp.append(len(cj))
    return len(rows), np.array(rp, dtype=np.int32), np.array(cj, dtype=np.int32), np.array(cv)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_csr_bitwise(a, b, what=""):
    """a, b: (rowptr, col, val)"""
    for x, y, nm in zip(a, b, ("rowptr", "col", "val")):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape, (what, nm, x.shape, y.shape)
        assert np.array_equal(bits(x), bits(y)), (what, nm)


def levels_of(amg, H):
    return {"A": [H.get(amg.AMG_GEN_A, l) for l in range(H.L)],
            "P": [H.get(amg.AMG_GEN_P, l) for l in range(H.L - 1)],
            "R": [H.get(amg.AMG_GEN_R, l) for l in range(H.L - 1)]}


def assert_levels_bitwise(la, lb):
    assert len(la["A"]) == len(lb["A"])
    for w in ("A", "P", "R"):
        assert len(la[w]) == len(lb[w])
        for l, (x, y) in enumerate(zip(la[w], lb[w])):
            assert x[0] == y[0] and x[1] == y[1], (w, l)
            assert_csr_bitwise(x[2:], y[2:], f"{w}{l}")


def problem(amg, oracle, name):
    """(n, rowptr, col, val, setup keywords, num_functions)"""
    if name == "lap12":
        A = oracle.laplace_7pt(12)
        return A.nrows, A.rowptr, A.col, A.val, dict(coarsen_type=10, strong_threshold=0.25), 1
    if name == "lap16":
        A = oracle.laplace_7pt(16)
        return A.nrows, A.rowptr, A.col, A.val, dict(coarsen_type=10, strong_threshold=0.25), 1
    n, rp, cj, v, _ = amg.classical.elasticity(2)
    return n, rp, cj, v, dict(coarsen_type=9, strong_threshold=0.5), 3


@pytest.fixture(scope="module")
def lap12_P(amg, oracle):
    n, rp, cj, v, kw, _ = problem(amg, oracle, "lap12")
    H = amg.classical.ClassicalAMG(n, rp, cj, v, **kw)
    return H.get(amg.AMG_GEN_P, 0)


@pytest.mark.parametrize("tf,mx", PAIRS)
def test_rule_matches_restatement(amg, lap12_P, tf, mx):
    n, rp, cj, v = crafted_rows()
    assert_csr_bitwise(amg.classical.truncate_rows(n, rp, cj, v, tf, mx), trunc_np(n, rp, cj, v, tf, mx), "crafted")
    pn, _, prp, pcj, pv = lap12_P
    assert np.diff(prp).max() > 4
    got = amg.classical.truncate_rows(pn, prp, pcj, pv, tf, mx)
    assert_csr_bitwise(got, trunc_np(pn, prp, pcj, pv, tf, mx), "P of 12^3")
    if mx:
        assert np.diff(got[0]).max() <= mx


def test_tie_and_zero_sum_rows(amg):
    n, rp, cj, v = crafted_rows()
    orp, ocj, ov = amg.classical.truncate_rows(n, rp, cj, v, 0.0, 3)
    # equal magnitudes: the three smallest columns stay, in storage order
    assert list(ocj[orp[2]:orp[3]]) == [1, 3, 4]
    assert list(ocj[orp[3]:orp[4]]) == [2, 4, 0]
    orp, ocj, ov = amg.classical.truncate_rows(n, rp, cj, v, 0.3, 0)
    # kept sum 3 - 3 + 2 - 2 = 0: no rescale
    assert list(ov[orp[4]:orp[5]]) == [3.0, -3.0, 2.0, -2.0]
    orp, ocj, ov = amg.classical.truncate_rows(n, rp, cj, v, 0.2, 4)
    assert list(ov[orp[5]:orp[6]]) == [3.0, -3.0, 2.0, -2.0]


def test_noop_is_bitwise(amg, oracle, lap12_P):
    n, rp, cj, v = crafted_rows()
    longest = int(np.diff(rp).max())
    for tf, mx in ((0.0, 0), (0.0, longest), (0.0, longest + 7)):
        assert_csr_bitwise(amg.classical.truncate_rows(n, rp, cj, v, tf, mx), (rp, cj, v), (tf, mx))
    pn, _, prp, pcj, pv = lap12_P
    assert_csr_bitwise(amg.classical.truncate_rows(pn, prp, pcj, pv, 0.0, int(np.diff(prp).max())), (prp, pcj, pv))
    N, arp, acj, av, kw, _ = problem(amg, oracle, "lap12")
    a = amg.classical.ClassicalAMG(N, arp, acj, av, **kw)
    b = amg.classical.ClassicalAMG(N, arp, acj, av, P_max_elmts=0, trunc_factor=0.0, **kw)
    assert_levels_bitwise(levels_of(amg, a), levels_of(amg, b))


def expected_hierarchy(amg, oracle, n, rp, cj, v, kw, nfun, tf, mx):
    """The truncated hierarchy without the setup's own truncation: two-level
    setups, trunc_np, oracle transpose and Gustavson products."""
    As, Ps, Rs = [oracle.Csr(n, n, rp, cj, v)], [], []
    for l in range(24):
        A = As[-1]
        if A.nrows <= 9:  # max_coarse_size default
            break
        nf = nfun if A.nrows % nfun == 0 else 1  # the setup's fall-back to one function
        H2 = amg.classical.ClassicalAMG(A.nrows, A.rowptr, A.col, A.val, max_levels=2, num_functions=nf,
                                        seed=DEFAULT_SEED + 7919 * l, **kw)
        if H2.L < 2:
            break
        pn, pm, prp, pcj, pv = H2.get(amg.AMG_GEN_P, 0)
        P = oracle.Csr(pn, pm, *trunc_np(pn, prp, pcj, pv, tf, mx))
        R = oracle.transpose(P)
        Ps.append(P)
        Rs.append(R)
        As.append(oracle.spgemm(R, oracle.spgemm(A, P)))
    f = lambda M: (M.nrows, M.ncols, M.rowptr, M.col, M.val)  # noqa: E731
    return {"A": [f(M) for M in As], "P": [f(M) for M in Ps], "R": [f(M) for M in Rs]}


@pytest.mark.parametrize("name", ["lap12", "elast2"])
def test_truncated_hierarchy_by_recursion(amg, oracle, name):
    n, rp, cj, v, kw, nfun = problem(amg, oracle, name)
    H = amg.classical.ClassicalAMG(n, rp, cj, v, num_functions=nfun, P_max_elmts=4, trunc_factor=0.2, **kw)
    assert H.L >= 3
    assert_levels_bitwise(levels_of(amg, H), expected_hierarchy(amg, oracle, n, rp, cj, v, kw, nfun, 0.2, 4))


def test_properties(amg, oracle):
    n, rp, cj, v, kw, _ = problem(amg, oracle, "lap12")
    Hu = amg.classical.ClassicalAMG(n, rp, cj, v, **kw)
    Ht = amg.classical.ClassicalAMG(n, rp, cj, v, P_max_elmts=4, trunc_factor=0.2, **kw)
    lt = levels_of(amg, Ht)
    for P, R in zip(lt["P"], lt["R"]):
        assert np.diff(P[2]).max() <= 4
        T = oracle.transpose(oracle.Csr(*P))
        assert_csr_bitwise((T.rowptr, T.col, T.val), R[2:], "R == P^T")
    # level 0 shares A_0, so its untruncated P is Hu's
    _, _, urp, _, uv = Hu.get(amg.AMG_GEN_P, 0)
    _, _, trp, _, tv = lt["P"][0]
    assert np.diff(urp).max() > 4
    for i in range(n):
        su, st = _ssum(uv[urp[i]:urp[i + 1]]), _ssum(tv[trp[i]:trp[i + 1]])
        assert abs(st - su) <= 1e-14 * abs(su), i
    # operator complexity, PMIS theta 0.5
    kw8 = dict(coarsen_type=8, strong_threshold=0.5)
    oc = []
    for extra in ({}, {"P_max_elmts": 4}):
        H = amg.classical.ClassicalAMG(n, rp, cj, v, **kw8, **extra)
        nz = [H.get(amg.AMG_GEN_A, l)[2][-1] for l in range(H.L)]
        oc.append(sum(int(x) for x in nz) / int(nz[0]))
    print(f"operator complexity 12^3 PMIS 0.5: {oc[0]:.3f} -> {oc[1]:.3f} with P_max_elmts = 4")
    assert oc[1] < oc[0]


def test_truncated_hierarchy_converges(amg, oracle):
    n, rp, cj, v, kw, _ = problem(amg, oracle, "lap12")
    H = amg.classical.ClassicalAMG(n, rp, cj, v, P_max_elmts=4, trunc_factor=0.2, **kw)
    lv = levels_of(amg, H)
    OH = oracle.Hier(*[[oracle.Csr(*m) for m in lv[w]] for w in ("A", "P", "R")],
                     oracle.make_opts(smooth_weight=0.8, num_cycles=12))
    _, hist, k = OH.solve(oracle.rhs_rand(n))
    print(f"V(1,1) Jacobi(0.8) on the (0.2, 4) hierarchy: relres {hist[12] / hist[0]:.3e} after 12 cycles")
    assert k == 12 and hist[12] < 1e-3 * hist[0]


def test_smoothed_transfers_host(amg, oracle):
    n, rp, cj, v, kw, _ = problem(amg, oracle, "lap12")
    H = amg.classical.ClassicalAMG(n, rp, cj, v, **kw)
    with pytest.raises(amg.AmgError, match="no operator"):
        H.get(amg.AMG_GEN_PS, 0)
    with pytest.raises(amg.AmgError, match="no operator"):
        H.get(amg.AMG_GEN_RS, 0)
    lv = levels_of(amg, H)
    H.smooth_transfers(0.8)
    ref = []
    for l in range(H.L - 1):
        ps, rs = oracle.smooth_transfer(oracle.Csr(*lv["A"][l]), oracle.Csr(*lv["P"][l]), 0.8)
        ref.append(ps)
        g = H.get(amg.AMG_GEN_PS, l)
        assert (g[0], g[1]) == (ps.nrows, ps.ncols)
        assert_csr_bitwise(g[2:], (ps.rowptr, ps.col, ps.val), f"PS{l}")
        g = H.get(amg.AMG_GEN_RS, l)
        assert (g[0], g[1]) == (rs.nrows, rs.ncols)
        assert_csr_bitwise(g[2:], (rs.rowptr, rs.col, rs.val), f"RS{l}")
    with pytest.raises(amg.AmgError):
        H.get(amg.AMG_GEN_PS, H.L - 1)
    assert max(np.diff(p.rowptr).max() for p in ref) > 8
    H.smooth_transfers(0.8, add_P_max_elmts=8)  # replaces the stored pair
    for l in range(H.L - 1):
        g = H.get(amg.AMG_GEN_PS, l)
        assert np.diff(g[2]).max() <= 8
        ps = ref[l]
        assert_csr_bitwise(g[2:], trunc_np(ps.nrows, ps.rowptr, ps.col, ps.val, 0.0, 8), f"truncated PS{l}")
        T = oracle.transpose(oracle.Csr(*g))
        r = H.get(amg.AMG_GEN_RS, l)
        assert (r[0], r[1]) == (T.nrows, T.ncols)
        assert_csr_bitwise(r[2:], (T.rowptr, T.col, T.val), f"RS{l} == PS{l}^T")
    H.smooth_transfers(0.8, add_P_max_elmts=8, add_trunc_factor=0.1)
    ps = ref[0]
    assert_csr_bitwise(H.get(amg.AMG_GEN_PS, 0)[2:], trunc_np(ps.nrows, ps.rowptr, ps.col, ps.val, 0.1, 8))


def test_bad_parameters(amg, oracle):
    n, rp, cj, v = crafted_rows()
    for tf, mx in ((-0.1, 0), (1.5, 0), (0.0, -1)):
        with pytest.raises(amg.AmgError, match="trunc_factor"):
            amg.classical.truncate_rows(n, rp, cj, v, tf, mx)
    N, arp, acj, av, kw, _ = problem(amg, oracle, "lap12")
    for extra in ({"P_max_elmts": -1}, {"trunc_factor": -0.5}, {"trunc_factor": 1.01}):
        with pytest.raises(amg.AmgError, match="trunc_factor"):
            amg.classical.ClassicalAMG(N, arp, acj, av, **kw, **extra)
    H = amg.classical.ClassicalAMG(N, arp, acj, av, **kw)
    for args in ((0.8, -1, 0.0), (0.8, 0, -0.1), (0.8, 0, 1.5)):
        with pytest.raises(amg.AmgError, match="add_trunc_factor"):
            H.smooth_transfers(*args)
    with pytest.raises(amg.AmgError):  # a failed call leaves no operators behind
        H.get(amg.AMG_GEN_PS, 0)


def test_generator_rejects_smoothed_codes(amg):
    g = amg.Gen(8)
    for code in (amg.AMG_GEN_PS, amg.AMG_GEN_RS):
        assert amg.lib.amg_gen_nnz(g.h, code, 0, 0, 1) < 0
        with pytest.raises(amg.AmgError, match="bad operator"):
            g.host_csr(code, 0)
    g.free()
