"""GPU: the device side of the classical setup on its own -- spgemm_ub_k,
spgemm_row_k, spgemm_pack_k and the batching of spgemm_dev through
amg_csr_spgemm, smooth_factor_k through smooth_transfers -- bit-identical to
the host path, which tests/test_spgemm.py pins against a Python-float
restatement, the oracle and a dense product.  The case table (hash collisions
that wrap, hub rows, empty rows, repeated columns, cancelling sums, square
results from rectangular operands) is test_spgemm.cases."""
import numpy as np
import pytest

from test_spgemm import (CASE_NAMES, CRAFTED_KW, batches_of, cap_of, cases, crafted_operator, ub_of)
from test_truncation import assert_csr_bitwise, assert_levels_bitwise, levels_of, problem

pytestmark = pytest.mark.gpu

BATCHED = ["rand", "hub", "collide", "empty"]


@pytest.fixture(scope="module")
def table(amg, oracle):
    return cases(amg, oracle)


@pytest.fixture(scope="module")
def host_products(amg, table):
    return {nm: amg.classical.spgemm(c["A"], c["B"], device=-1) for nm, c in table.items()}


def assert_product_bitwise(got, ref, what):
    assert (got[0], got[1]) == (ref[0], ref[1]), what
    assert_csr_bitwise(got[2:], ref[2:], what)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_product_matches_host(amg, table, host_products, name):
    c = table[name]
    assert_product_bitwise(amg.classical.spgemm(c["A"], c["B"], device=0), host_products[name], name)


@pytest.mark.parametrize("slots", [256, 1])
def test_device_product_in_batches(amg, table, host_products, slots):
    caps = {nm: cap_of(ub_of(table[nm]["A"], table[nm]["B"])) for nm in BATCHED}
    nb = {nm: batches_of(caps[nm], slots) for nm in BATCHED}
    print(f"budget {slots}: (batches, rows over the budget) {nb}")
    if slots == 256:
        assert max(b for b, _ in nb.values()) >= 8
        assert max(o for _, o in nb.values()) >= 1, "no row whose table alone exceeds the budget"
    else:  # every row its own batch, every row over the budget
        assert all(nb[nm] == (len(caps[nm]), len(caps[nm])) for nm in BATCHED)
    try:
        amg.classical.set_spgemm_scratch(slots)
        for nm in BATCHED:
            c = table[nm]
            assert_product_bitwise(amg.classical.spgemm(c["A"], c["B"], device=0), host_products[nm],
                                   f"{nm} at {slots} slots")
    finally:
        amg.classical.set_spgemm_scratch(0)


def test_galerkin_product_in_batches(amg, oracle):
    n, rp, cj, v, kw, nfun = problem(amg, oracle, "elast2")
    kw = dict(kw, num_functions=nfun)
    Hh = amg.classical.ClassicalAMG(n, rp, cj, v, device=-1, **kw)
    assert Hh.L >= 3
    try:
        amg.classical.set_spgemm_scratch(4096)
        Hd = amg.classical.ClassicalAMG(n, rp, cj, v, device=0, **kw)
    finally:
        amg.classical.set_spgemm_scratch(0)
    assert_levels_bitwise(levels_of(amg, Hd), levels_of(amg, Hh))


def smoothed_of(amg, H):
    return [(H.get(amg.AMG_GEN_PS, l), H.get(amg.AMG_GEN_RS, l)) for l in range(H.L - 1)]


@pytest.fixture(scope="module")
def smoothing_hierarchies(amg, oracle):
    n, rp, cj, v, kw, nfun = problem(amg, oracle, "elast2")
    He = amg.classical.ClassicalAMG(n, rp, cj, v, num_functions=nfun, **kw)
    assert nfun == 3 and np.diff(rp).max() == 81
    n, rp, cj, v = crafted_operator()
    Hc = amg.classical.ClassicalAMG(n, rp, cj, v, **CRAFTED_KW)
    assert Hc.L == 2
    _, _, arp, _, av = Hc.get(amg.AMG_GEN_A, 0)
    diag = av[arp[:-1]]
    assert diag.min() != diag.max() and np.diff(arp).max() > 128
    return {"elast2": He, "crafted": Hc}


@pytest.mark.parametrize("w", [0.8, 1.0])
@pytest.mark.parametrize("name", ["elast2", "crafted"])
def test_device_smoothing_factors(amg, oracle, smoothing_hierarchies, name, w):
    H = smoothing_hierarchies[name]
    lv = levels_of(amg, H)
    _, _, arp, _, av = lv["A"][0]
    assert len(set(av[arp[:-1]].tolist())) > 1, "uniform diagonal: g and gt would be the same numbers"
    H.smooth_transfers(w, device=0)
    for l, (ps, rs) in enumerate(smoothed_of(amg, H)):
        ops, ors = oracle.smooth_transfer(oracle.Csr(*lv["A"][l]), oracle.Csr(*lv["P"][l]), w)
        assert (ps[0], ps[1], rs[0], rs[1]) == (ops.nrows, ops.ncols, ors.nrows, ors.ncols)
        assert_csr_bitwise(ps[2:], (ops.rowptr, ops.col, ops.val), f"{name} PS{l} w={w}")
        assert_csr_bitwise(rs[2:], (ors.rowptr, ors.col, ors.val), f"{name} RS{l} w={w}")
    H.smooth_transfers(w, add_P_max_elmts=8, add_trunc_factor=0.1, device=0)
    dev = smoothed_of(amg, H)
    H.smooth_transfers(w, add_P_max_elmts=8, add_trunc_factor=0.1, device=-1)
    for l, ((dp, dr), (hp, hr)) in enumerate(zip(dev, smoothed_of(amg, H))):
        assert dp[:2] == hp[:2] and dr[:2] == hr[:2]
        assert np.diff(dp[2]).max() <= 8
        assert_csr_bitwise(dp[2:], hp[2:], f"{name} truncated PS{l} w={w}")
        assert_csr_bitwise(dr[2:], hr[2:], f"{name} truncated RS{l} w={w}")


def test_bad_column_leaves_the_device_usable(amg, table, host_products):
    A, B = table["dyadic"]["A"], table["dyadic"]["B"]
    bad = B[3].copy()
    bad[len(bad) // 2] = B[1]
    with pytest.raises(amg.AmgError, match="B: column"):
        amg.classical.spgemm(A, (B[0], B[1], B[2], bad, B[4]), device=0)
    bad = A[3].copy()
    bad[0] = -1
    with pytest.raises(amg.AmgError, match="A: column"):
        amg.classical.spgemm((A[0], A[1], A[2], bad, A[4]), B, device=0)
    assert_product_bitwise(amg.classical.spgemm(A, B, device=0), host_products["dyadic"], "after the errors")
