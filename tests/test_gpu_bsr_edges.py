"""The 3x3 block kernels (bsr3_kernel, bsr3_row_kernel; build_bsr3) on the crafted
operators of tests/bsr_cases.py, bit for bit against the host oracle.

tests/test_gpu_bsr.py runs the generated elasticity operator (8..27 blocks per
row, identity rows as the only CSR-form rows) and compares the block kernels
with the device's own CSR kernels.  Here every device result is compared with
the oracle on the same arrays (and, second, with the device's plain-CSR form),
on operators holding what that fixture lacks: block rows of 1, 130 and 255
blocks, CSR-form block rows that are no identity rows, slices made only of
CSR-form rows, a partial last slice, fp64 blocks chosen by the value count,
zero diagonals, a uniform diagonal (the reciprocal division and its fallback),
the selection boundaries, and the instantiations only an environment variable
reaches (AMG_BSR3_XS / AMG_BSR3_U / AMG_BSR3_RU: fresh child processes).

Every comparison is bitwise: the kernels promise each row's CSR summation
order, which is the oracle's.  tests/test_bsr_cases.py (CPU) pins that the
operators hold these cases; Mat.bsr3_counts() pins that the device stored them
as blocks (a row that fell back to CSR form would pass everything else).

The operands planted for the uniform-diagonal division (-0.0, +0.0, 1e300,
1e-300) all reach the fallback, but for the diagonal 6.0 none of them can show
a wrong division: the reciprocal path is exact at omega * 1e300 and
omega * 1e-300 (div_rcp of tests/div_cases.py, asserted), and a -0.0 quotient cannot show in a
sweep's output (u_i + q is -0.0 only for u_i = -0.0, which makes the residual
+0.0).  What tells the two divisions apart is an operand whose quotient is
subnormal (TINY below), planted next to them.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import bsr_cases as bc
from div_cases import div_rcp  # csrc/amg_kernels.hip div_rcp restated in exact arithmetic
from test_gpu_bsr import reg  # registers under given switches and restores the context's
from test_gpu_kernels import assert_bitwise, _vecs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
AB = [(1, 0), (-1, 0), (2.5, 0), (1, -1), (-1, 1), (0.5, -0.5), (1, 1), (-1, -1), (3, 3), (1, 0.3), (-1, 0.7),
      (1.7, -0.4)]  # test_spgemv_branches' pairs
FORMS = {"triplet": 1, "row": 2}  # amg_set_bsr3: three lanes per block row (21-slices), a lane per block row (64)


# ---- the same operations on the device and in the oracle --------------------------------------
class Dev:
    def __init__(self, amg, ctx, M):
        self.amg, self.ctx, self.M, self.s, self.n = amg, ctx, M, amg.smem, M.nrows

    def l1norms(self):
        out = self.ctx.vec(self.n)
        self.s.L1_row_norm(self.ctx, self.M, out)
        return out.download()

    def matvec(self, x):
        y = self.ctx.vec(self.n)
        self.s.SMEM_Sync_Parfor_MatVec(self.ctx, self.M, self.ctx.vec(x), y)
        return y.download()

    def spgemv(self, x, b, alpha, beta, y0, rb, re, alias=False):
        y = self.ctx.vec(y0)
        self.s.SMEM_SpGEMV(self.ctx, self.M, self.ctx.vec(x), y if alias else self.ctx.vec(b), alpha, beta, y, rb, re)
        return y.download()

    def residual(self, b, x, y0, r0, rb, re):
        y, r = self.ctx.vec(y0), self.ctx.vec(r0)
        self.s.SMEM_Residual(self.ctx, self.M, self.ctx.vec(b), self.ctx.vec(x), y, r, rb, re)
        return y.download(), r.download()

    def jacobi(self, f, u0, w, sweeps, zero, rb, re, seq=False):
        u, p = self.ctx.vec(u0), self.ctx.vec(self.n)
        if seq:
            self.s.SEQ_Jacobi(self.ctx, self.M, self.ctx.vec(f), u, p, sweeps, zero, w)
        else:
            self.s.SMEM_Sync_Jacobi(self.ctx, self.M, self.ctx.vec(f), u, p, sweeps, zero, w, rb, re)
        return u.download(), p.download()

    def l1jacobi(self, f, u0, l1, sweeps, zero, rb, re):
        u, p = self.ctx.vec(u0), self.ctx.vec(self.n)
        self.amg.check(self.amg.lib.amg_l1_jacobi(self.ctx.h, self.M.h, self.ctx.vec(f).h, u.h, p.h,
                                                  self.ctx.vec(l1).h, sweeps, zero, rb, re, 0))
        return u.download(), p.download()

    def sym(self, f, u0, w, l1, sweeps, zero):
        u, y, r = self.ctx.vec(u0), self.ctx.vec(self.n), self.ctx.vec(self.n)
        if l1 is None:
            self.s.SMEM_Sync_SymmetricJacobi(self.ctx, self.M, self.ctx.vec(f), u, y, r, sweeps, zero, w, 0, self.n)
        else:
            self.s.SMEM_Sync_SymmetricL1Jacobi(self.ctx, self.M, self.ctx.vec(f), u, y, r, self.ctx.vec(l1), sweeps,
                                               zero, 0, self.n)
        return u.download(), r.download()


class Ora:
    def __init__(self, oracle, A):
        self.o, self.A, self.n = oracle, A, A.nrows

    def l1norms(self):
        return self.o.l1_norms(self.A)

    def matvec(self, x):
        return self.o.smem_matvec(self.A, x, np.zeros(self.n))

    def spgemv(self, x, b, alpha, beta, y0, rb, re, alias=False):
        y = y0.copy()
        return self.o.smem_spgemv(self.A, x, y.copy() if alias else b, alpha, beta, y, rb, re)

    def residual(self, b, x, y0, r0, rb, re):
        y, r = y0.copy(), r0.copy()
        self.o.smem_residual(self.A, b, x, y, r, rb, re)
        return y, r

    def jacobi(self, f, u0, w, sweeps, zero, rb, re, seq=False):
        # amg_jacobi copies the whole u to u_prev; the oracle's slice copies [rb, re): u_prev is
        # compared on the full range only (it starts as zeros there, as on the device)
        u, p = u0.copy(), (np.zeros(self.n) if (rb, re) == (0, self.n) else u0.copy())
        if seq:
            self.o.seq_jacobi(self.A, f, u, p, w, sweeps, zero)
        else:
            self.o.smem_jacobi(self.A, f, u, p, w, sweeps, zero, rb, re)
        return u, p

    def l1jacobi(self, f, u0, l1, sweeps, zero, rb, re):
        u, p = u0.copy(), (np.zeros(self.n) if (rb, re) == (0, self.n) else u0.copy())
        self.o.smem_l1jacobi(self.A, f, u, p, l1, sweeps, zero, rb, re)
        return u, p

    def sym(self, f, u0, w, l1, sweeps, zero):
        u, y, r = u0.copy(), np.zeros(self.n), np.zeros(self.n)
        if l1 is None:
            self.o.smem_sym_jacobi(self.A, f, u, y, r, w, sweeps, zero)
        else:
            self.o.smem_sym_l1jacobi(self.A, f, u, y, r, l1, sweeps, zero)
        return u, r


def row_ranges(cnt, sl):
    """Row ranges from the slice size: block-served (slice-aligned) and two that are not."""
    nb = cnt.size
    n, ns, empty = 3 * nb, (nb + sl - 1) // sl, bc.all_csr_slices(cnt, sl)
    return [(0, 3 * sl),                                       # one slice
            (3 * sl * empty[0], 3 * sl * (empty[-1] + 1)),     # starts and ends on all-CSR slices
            (3 * sl * (ns - 2), n),                            # into the last (partial) slice, the 130-block hub
            (3, n - 6), (1, n - 2)]                            # unaligned: the CSR kernels


def all_ops(B, l1, ranges, sym_weighted=True):
    """Every operation of this suite on backend B: [(name, array)].  sym_weighted False leaves
    the weighted symmetric Jacobi out: it divides by the diagonal unguarded (as the reference
    does), so with a zero diagonal it has no finite result to compare."""
    n = B.n
    full = (0, n)
    x, b, f, u0, y0, r0 = (_vecs(n, s) for s in (71, 72, 73, 74, 75, 76))
    out = [("l1 norms", B.l1norms()), ("matvec", B.matvec(x))]
    for al, be in AB:
        out.append((f"spgemv {al} {be}", B.spgemv(x, b, al, be, np.zeros(n), *full)))
    out.append(("spgemv b aliases y", B.spgemv(x, None, 1.0, 1.0, y0, *full, alias=True)))
    for name, (rb, re) in [("full", full)] + [(f"rows [{a}, {e})", (a, e)) for a, e in ranges]:
        y, r = B.residual(b, x, y0, r0, rb, re)
        out += [(f"residual y {name}", y), (f"residual r {name}", r)]
        if (rb, re) != full:
            out.append((f"spgemv -1 1 {name}", B.spgemv(x, b, -1.0, 1.0, y0, rb, re)))
            out.append((f"spgemv alias {name}", B.spgemv(x, None, 1.0, 1.0, y0, rb, re, alias=True)))
        for zero in (0, 1):
            for w in (0.8, 1.0):
                u, p = B.jacobi(f, u0, w, 3, zero, rb, re)
                out.append((f"jacobi zero={zero} w={w} {name}", u))
                if (rb, re) == full:
                    out.append((f"jacobi u_prev zero={zero} w={w}", p))
            u, p = B.l1jacobi(f, u0, l1, 3, zero, rb, re)
            out.append((f"l1 jacobi zero={zero} {name}", u))
            if (rb, re) == full:
                out.append((f"l1 jacobi u_prev zero={zero}", p))
    for zero in (0, 1):
        u, p = B.jacobi(f, u0, 0.8, 3, zero, *full, seq=True)
        out += [(f"seq jacobi zero={zero}", u), (f"seq jacobi u_prev zero={zero}", p)]
        for tag, ll in (("sym jacobi", None), ("sym l1 jacobi", l1))[0 if sym_weighted else 1:]:
            u, r = B.sym(f, u0, 0.9, ll, 2, zero)
            out += [(f"{tag} u zero={zero}", u), (f"{tag} r zero={zero}", r)]
    return out


@pytest.fixture(scope="module")
def crafted(oracle):
    """variant -> (Case, restated counts, oracle CSR, l1 norms): built once, never modified."""
    out = {}
    for v in bc.VARIANTS:
        A = bc.make(v)
        OA = oracle.Csr(A.n, A.n, A.rowptr, A.col, A.val)
        out[v] = (A, bc.bsr3_counts(A.n, A.n, A.rowptr, A.col), OA, oracle.l1_norms(OA))
    return out


_REF = {}


def oracle_ops(oracle, crafted, variant, sl):
    if (variant, sl) not in _REF:
        A, cnt, OA, l1 = crafted[variant]
        _REF[variant, sl] = all_ops(Ora(oracle, OA), l1, row_ranges(cnt, sl), variant != "zerodiag")
    return _REF[variant, sl]


def check_registration(amg, M, A, cnt, form, vi=1):
    want = bc.bsr3_form(cnt, A.val, form, vi)
    assert (M.bsr3, amg.lib.amg_mat_bsr3_slice(M.h)) == want, (M.bsr3, amg.lib.amg_mat_bsr3_slice(M.h), want)
    if want[0]:
        got = M.bsr3_counts()
        assert got.dtype == np.uint8 and np.array_equal(got, cnt), np.nonzero(got != cnt)[0][:10]
    return want


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("variant", bc.VARIANTS)
def test_crafted_operator_bitwise(amg, oracle, ctx, crafted, variant, form):
    """Every operation on the blocked registration equals the oracle's bits; the plain-CSR
    registration gives the same.  'cont' takes fp64 blocks with value indexing left on."""
    A, cnt, OA, l1 = crafted[variant]
    Mb = reg(ctx, *A.arrays, FORMS[form], 1)
    Mp = reg(ctx, *A.arrays, 0, 0)
    try:
        kind, sl = check_registration(amg, Mb, A, cnt, FORMS[form])
        assert kind == (2 if variant == "cont" else 1) and sl == (64 if form == "row" and kind == 1 else 21)
        assert Mb.value_index == (0 if variant == "cont" else bc.distinct_values(A.val))
        assert Mp.bsr3 == 0 and amg.lib.amg_mat_bsr3_slice(Mp.h) == 0 and Mp.value_index == 0
        with pytest.raises(amg.AmgError, match="not in 3x3 block form"):
            Mp.bsr3_counts()
        ranges = row_ranges(cnt, sl)
        ref = oracle_ops(oracle, crafted, variant, sl)
        got = all_ops(Dev(amg, ctx, Mb), l1, ranges, variant != "zerodiag")
        plain = all_ops(Dev(amg, ctx, Mp), l1, ranges, variant != "zerodiag")
        assert [k for k, _ in got] == [k for k, _ in ref] == [k for k, _ in plain]
        for (name, g), (_, r), (_, p) in zip(got, ref, plain):
            assert np.all(np.isfinite(r)), name
            assert_bitwise(g, r, f"{variant} {form} blocks vs oracle: {name}")
            assert_bitwise(p, g, f"{variant} {form} plain CSR vs blocks: {name}")
    finally:
        Mb.free()
        Mp.free()


def test_fp64_blocks_forced(amg, oracle, ctx, crafted):
    """The value-indexable operator with value indexing off: fp64 blocks (21-slices)."""
    A, cnt, OA, l1 = crafted["main"]
    M = reg(ctx, *A.arrays, 2, 0)
    try:
        assert check_registration(amg, M, A, cnt, 2, 0) == (2, 21)
        ref = oracle_ops(oracle, crafted, "main", 21)
        for (name, g), (_, r) in zip(all_ops(Dev(amg, ctx, M), l1, row_ranges(cnt, 21)), ref):
            assert_bitwise(g, r, f"fp64 blocks: {name}")
    finally:
        M.free()


# ---- the uniform diagonal's reciprocal division and its fallback -------------------------------
# omega -> f whose operand omega * f of the division by 6.0 is normal, below 2^-960 (so the
# kernels must divide truly) and has a reciprocal-path quotient with another last bit
TINY = {1.0: float.fromhex("0x1.9d2b3ad7f6e0dp-1022"), 0.8: float.fromhex("0x1.cc42c0dcdff14p-1022")}
# block rows: a full wave of blocked rows in both forms (slices [336, 357) and [320, 384)), the
# partial last slice, CSR-form rows (short, inside an all-CSR run, shifted)
PLANT_AT = {"full wave": (340, 342, 344), "last slice": (1283, 1285, 1287), "csr form": (900, 722, 300)}


def planted(A, cnt, omega):
    """f and u (u = 0 up to signs) with the fallback's operands planted: per place six rows of
    three block rows take f = -0.0, +0.0, 1e300, 1e-300, TINY and an operand in range."""
    n = A.n
    f, u = _vecs(n, 77), np.zeros(n)
    vals = [-0.0, 0.0, 1e300, 1e-300, TINY[omega], 0.3]
    rows = {}
    for place, ts in PLANT_AT.items():
        rr = [3 * ts[0], 3 * ts[0] + 1, 3 * ts[1] + 1, 3 * ts[1] + 2, 3 * ts[2], 3 * ts[2] + 2]
        for r, v in zip(rr, vals):
            f[r] = v
        rows[place] = rr
        # the -0.0 row: every product of its sum is +0.0, so that res stays -0.0
        r = rr[0]
        k = slice(A.rowptr[r], A.rowptr[r + 1])
        assert np.all(u[A.col[k]] == 0.0) and not np.any(np.signbit(u[A.col[k]]))
        u[A.col[k]] = np.copysign(0.0, A.val[k])
    return f, u, rows


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("variant", ["unidiag", "unidiag_broken"])
def test_uniform_diagonal_division(amg, oracle, ctx, crafted, variant, form):
    """Every diagonal 6.0 (the reciprocal division; 'broken': one diagonal 5.0, so the true
    division everywhere): operands outside the reciprocal's range planted in a full wave of
    blocked rows, in the partial last slice and in CSR-form rows."""
    A, cnt, OA, l1 = crafted[variant]
    sl = 64 if form == "row" else 21
    for place, ts in PLANT_AT.items():  # the places are what they are named after
        if place == "csr form":
            assert all(cnt[t] == 0 for t in ts) and [A.csr_kinds[t] for t in ts] == ["short", "shifted", "shifted"]
        else:
            s = ts[0] // sl
            assert all(t // sl == s for t in ts) and np.all(cnt[s * sl:(s + 1) * sl] > 0)
            assert (cnt[s * sl:(s + 1) * sl].size == sl) == (place == "full wave")
    Mb = reg(ctx, *A.arrays, FORMS[form], 1)
    Mp = reg(ctx, *A.arrays, 0, 0)
    try:
        assert check_registration(amg, Mb, A, cnt, FORMS[form]) == (1, sl)
        for omega in (0.8, 1.0):
            f, u, rows = planted(A, cnt, omega)
            # the operands omega * res of the first sweep, as the kernels and the oracle form them
            res = f.copy()
            for place, rr in rows.items():
                for r in rr:
                    acc = f[r]
                    for k in range(A.rowptr[r], A.rowptr[r + 1]):
                        acc = acc - A.val[k] * u[A.col[k]]
                    res[r] = acc
                num = omega * res[rr]
                assert np.signbit(num[0]) and num[0] == 0.0 and not np.signbit(num[1]) and num[1] == 0.0
                assert num[2] >= 2.0 ** 960 and 0.0 < num[3] < 2.0 ** -960 and 2.0 ** -1022 <= num[4] < 2.0 ** -960
                assert res[rr[4]] == TINY[omega] and div_rcp(num[4], 6.0) != num[4] / 6.0
                assert all(div_rcp(x, 6.0) == x / 6.0 for x in num[[2, 3, 5]]) and np.all(np.isfinite(num))
            for sweeps in (1, 3):
                ref = Ora(oracle, OA).jacobi(f, u, omega, sweeps, 0, 0, A.n)
                assert np.all(np.isfinite(ref[0]))
                for tag, M in (("blocks", Mb), ("plain CSR", Mp)):
                    got = Dev(amg, ctx, M).jacobi(f, u, omega, sweeps, 0, 0, A.n)
                    assert_bitwise(got[0], ref[0], f"{variant} {form} {tag} w={omega} sweeps={sweeps} u")
                    assert_bitwise(got[1], ref[1], f"{variant} {form} {tag} w={omega} sweeps={sweeps} u_prev")
            # slice-aligned range into the partial last slice: the block kernels' partial waves vote
            rb = 3 * sl * ((cnt.size + sl - 1) // sl - 2)
            ref = Ora(oracle, OA).jacobi(f, u, omega, 1, 0, rb, A.n)
            got = Dev(amg, ctx, Mb).jacobi(f, u, omega, 1, 0, rb, A.n)
            assert_bitwise(got[0], ref[0], f"{variant} {form} w={omega} rows [{rb}, n)")
    finally:
        Mb.free()
        Mp.free()


# ---- selection boundaries ----------------------------------------------------------------------
@pytest.mark.parametrize("which", bc.BOUNDARIES)
def test_selection_boundaries(amg, oracle, ctx, which):
    """Small operators on each boundary of build_bsr3's rule: the registration matches the
    restated rule (a refused one reports 0 for form and slice), and MatVec and Jacobi equal
    the oracle's either way."""
    A, diag_first = bc.boundary(which)
    cnt = bc.bsr3_counts(A.n, A.n, A.rowptr, A.col, diag_first)
    assert (cnt is not None) == (which in ("ninety_exact", "hub255"))
    OA = oracle.Csr(A.n, A.n, A.rowptr, A.col, A.val)
    x, f, u0 = _vecs(A.n, 81), _vecs(A.n, 82), _vecs(A.n, 83)
    O = Ora(oracle, OA)
    ref = [O.matvec(x), *O.jacobi(f, u0, 0.8, 3, 0, 0, A.n), *O.jacobi(f, u0, 1.0, 2, 1, 0, A.n)]
    for form in (2, 1):
        M = reg(ctx, *A.arrays, form, 1, diag_first)
        try:
            kind, sl = check_registration(amg, M, A, cnt, form)
            assert (kind, sl) == ((1, 64 if form == 2 else 21) if cnt is not None else (0, 0))
            if cnt is None:
                with pytest.raises(amg.AmgError, match="not in 3x3 block form"):
                    M.bsr3_counts()
            D = Dev(amg, ctx, M)
            got = [D.matvec(x), *D.jacobi(f, u0, 0.8, 3, 0, 0, A.n), *D.jacobi(f, u0, 1.0, 2, 1, 0, A.n)]
            for k, (g, r) in enumerate(zip(got, ref)):
                assert_bitwise(g, r, f"{which} form {form} output {k}")
        finally:
            M.free()
    # a blocked registration after a refused one of the same shape (and the other way round)
    # stores its own layout: nothing of the earlier matrix is left over
    if which == "hub256":
        B, _ = bc.boundary("hub255")
        M = reg(ctx, *B.arrays, 2, 1)
        try:
            assert check_registration(amg, M, B, bc.bsr3_counts(B.n, B.n, B.rowptr, B.col), 2) == (1, 64)
            assert_bitwise(Dev(amg, ctx, M).matvec(x), Ora(oracle, oracle.Csr(B.n, B.n, B.rowptr, B.col, B.val)).matvec(x),
                           "hub255 after hub256")
        finally:
            M.free()


# ---- a two-level solve with the crafted operator as level 0 ------------------------------------
@pytest.mark.parametrize("smoother", ["jacobi", "l1"])
def test_two_level_solve(amg, oracle, ctx, crafted, smoother):
    """Level 0 is the main variant; P aggregates node pairs per component (piecewise constant,
    so the coarse operator keeps three functions), R = P^T, A_1 = R A P by the host SpGEMM.
    Six cycles, tol 0: the iterate equals the oracle's bit for bit.  Arithmetic only: the
    operator is no M-matrix and convergence is not asserted."""
    from test_gpu_solve import compare_solve
    A, cnt, OA, _ = crafted["main"]
    n, nc = A.n, 3 * ((A.nb + 1) // 2)
    rows = np.arange(n)
    P = (n, nc, np.arange(n + 1, dtype=np.int32), (3 * (rows // 6) + rows % 3).astype(np.int32), np.ones(n))
    Pt = oracle.transpose(oracle.Csr(*P))
    R = (nc, n, Pt.rowptr, Pt.col, Pt.val)
    RA = amg.classical.spgemm(R, (n, n, A.rowptr, A.col, A.val))
    A1 = amg.classical.spgemm(RA, P)
    assert A1[0] == A1[1] == nc and np.array_equal(A1[3][A1[2][:-1]], np.arange(nc))  # diagonal first
    host = {"A": [OA, oracle.Csr(*A1)], "P": [oracle.Csr(*P)], "R": [Pt]}
    M0 = ctx.csr(n, n, A.rowptr, A.col, A.val)  # as compare_solve registers it: the context's defaults
    M1 = ctx.csr(*A1)
    try:
        assert M0.bsr3 == 1 and amg.lib.amg_mat_bsr3_slice(M0.h) == 64
        # the coarse operator couples a node pair to 6 or 7 pairs: 18..21 entries per row, under
        # the 24 n gate, so level 1 runs the CSR kernels
        c1 = bc.bsr3_counts(nc, nc, A1[2], A1[3])
        assert (M1.bsr3 > 0) == (c1 is not None)
        print(f"two-level: level 1 {nc} rows, {A1[2][-1] / nc:.1f} entries per row, bsr3 {M1.bsr3}")
    finally:
        M0.free()
        M1.free()
    sm = amg.AMG_JACOBI if smoother == "jacobi" else amg.AMG_L1_JACOBI
    opts = amg.default_opts(smoother=sm, smooth_weight=0.8, num_cycles=6, tol=0.0)
    u, hist = compare_solve(amg, oracle, ctx, host, opts, _vecs(n, 91))
    assert np.all(np.isfinite(u)) and len(hist) == 7


# ---- the instantiations only the environment reaches -------------------------------------------
def child_ops(B, l1):
    n = B.n
    x, b, f, u0 = (_vecs(n, s) for s in (71, 72, 73, 74))
    return [("matvec", B.matvec(x)), ("spgemv -1 0.7", B.spgemv(x, b, -1.0, 0.7, np.zeros(n), 0, n)),
            ("jacobi", B.jacobi(f, u0, 0.8, 3, 0, 0, n)[0]), ("l1 jacobi", B.l1jacobi(f, u0, l1, 3, 0, 0, n)[0])]


CHILD_CASES = (("main", 1), ("main", 2), ("cont", 1))  # value-indexed triplet and row forms, fp64 blocks


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def child_main():
    """One process under the environment's AMG_BSR3_* settings: SHA-256 of each output."""
    from conftest import load_package
    from oracle import pyoracle
    amg = load_package()
    ctx = amg.Context(device=0, nstreams=2)
    for variant, form in CHILD_CASES:
        A = bc.make(variant)
        l1 = pyoracle.l1_norms(pyoracle.Csr(A.n, A.n, A.rowptr, A.col, A.val))
        M = reg(ctx, *A.arrays, form, 1)
        print(f"form {variant} {form} {M.bsr3} {amg.lib.amg_mat_bsr3_slice(M.h)}")
        for name, a in child_ops(Dev(amg, ctx, M), l1):
            print(f"out {variant} {form} {name}: {digest(a)}")
        M.free()
    ctx.close()


ENV_SETTINGS = {
    "triplet": [{"AMG_BSR3_XS": "0"}, {"AMG_BSR3_XS": "0", "AMG_BSR3_U": "9"}, {"AMG_BSR3_XS": "1", "AMG_BSR3_U": "2"},
                {"AMG_BSR3_XS": "1", "AMG_BSR3_U": "3"}, {"AMG_BSR3_XS": "1", "AMG_BSR3_U": "6"},
                {"AMG_BSR3_XS": "1", "AMG_BSR3_U": "14"}, {"AMG_BSR3_XS": "1", "AMG_BSR3_U": "27"}],
    "row": [{"AMG_BSR3_RU": "2"}, {"AMG_BSR3_RU": "4"}, {"AMG_BSR3_RU": "8"}],
}


@pytest.mark.parametrize("group", list(ENV_SETTINGS))
def test_env_only_instantiations(oracle, crafted, group):
    """AMG_BSR3_XS / AMG_BSR3_U (the triplet kernel's x sharing and unroll depth) and
    AMG_BSR3_RU (the row kernel's) are read once per process: one fresh child process per
    setting, one after another, each under its own time limit; the first that fails ends the
    test and nothing is started after it.  Every digest equals the oracle's."""
    want = []
    for variant, form in CHILD_CASES:
        A, cnt, OA, l1 = crafted[variant]
        want.append(f"form {variant} {form} %d %d" % bc.bsr3_form(cnt, A.val, form, 1))
        want += [f"out {variant} {form} {name}: {digest(a)}" for name, a in child_ops(Ora(oracle, OA), l1)]
    for setting in ENV_SETTINGS[group]:
        env = {k: v for k, v in os.environ.items() if not k.startswith("AMG_BSR3")}
        env.update(setting)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, cwd=HERE, timeout=120,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert p.returncode == 0, f"{setting}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}"
        got = [ln for ln in p.stdout.splitlines() if ln.startswith(("form ", "out "))]
        assert got == want, (setting, [(g, w) for g, w in zip(got, want) if g != w] or (len(got), len(want)))


if __name__ == "__main__" and sys.argv[1:] == ["--child"]:
    child_main()
