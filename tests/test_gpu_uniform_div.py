"""The Jacobi epilogues' division by a uniform diagonal (div_rcp, div_rcp_ok,
jac_div1, jac_div2, fast_div_of in csrc/amg_kernels.hip) on every storage rung
that runs EpiJacobi, with the divisors and planted operands of
tests/div_cases.py.

One sweep SMEM_Sync_Parfor_Jacobi(ctx, M, f, u, u_prev, 1, 0, 1.0) with u = +0.0
makes the epilogue's operand exactly f[i] (the sum starts at f[i] and every
product is a zero), so u_out[i] must carry the bits of 0.0 + f[i] / a_ii as
numpy computes it (the 0.0 + matters for a zero quotient only) and the bits of
the oracle's smem_jacobi.  f holds the near-midpoint operands of the divisor,
in runs of 128 rows (a wave of the pair-coded kernels; two of the others):
even runs hold operands in range only, so their waves take the reciprocal; odd
runs hold exactly one operand of div_cases.fallback.  inf, NaN, 2^960, the
double just below 2^-960 and the divisor's tiny operand (whose subnormal
quotient differs between the two divisions) are out of range, so their waves
must divide truly.  The two zeros are there for the output's sign only: +0.0
is in range by rule, and f = -0.0 reaches the epilogue as +0.0 in every row
that holds a negative entry (subtracting its product -0.0 gives +0.0), which
is every row of the stencils; their waves may take either division, with the
same bits.  A second set of sweeps (random u, weights 0.7 and 0.8, 2 and 3 sweeps) goes
against the oracle alone.

Each operator is asserted to sit on its rung through the form getters, and each
divisor to be admitted or refused by div_cases.admitted (the library has no
getter for "reciprocal taken"; test_fast_div_off_same_bits compares a process
with AMG_FAST_DIV=0 instead).

EpiResJacobi and the fused level-0 marches (mz_sweep_outer_kernel,
mz_two_sweep_kernel) are reachable only through a solve: test_solve_divisors
runs them with the diagonals 3, 5, 7 and (2^30 - 1) 2^-27 on random right-hand
sides.  They see planted operands nowhere; nor does the 3x3 block rung here
(tests/test_gpu_bsr_edges.py plants its own for the diagonal 6.0).
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import div_cases as dc
from test_gpu_kernels import assert_bitwise, _vecs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RUN = 128  # rows per run of the planted layout
LEVELS = np.linspace(-1.0, 1.0, 64) * (1.0 + 1.0 / 3.0)  # the quantised operators' 64 values


# ---- host operators: a template per structure, the diagonal filled in per divisor ---------------
def random_rows(n, k, seed, quantised):
    """n rows of exactly k entries: the diagonal first, then k - 1 other columns ascending"""
    g = np.random.default_rng(seed)
    col = np.empty((n, k), dtype=np.int32)
    for i in range(n):
        c = g.choice(n - 1, size=k - 1, replace=False)
        col[i, 0], col[i, 1:] = i, np.sort(c + (c >= i))
    val = LEVELS[g.integers(0, LEVELS.size, size=(n, k))] if quantised else g.uniform(-1, 1, size=(n, k))
    return np.arange(0, n * k + 1, k, dtype=np.int32), col.ravel(), val.ravel()


def stencil7(oracle, nx, ny, nz):
    L = oracle.laplace_7pt(nx, ny, nz)
    first = np.zeros(L.val.size, bool)
    first[L.rowptr[:-1]] = True
    assert np.all(L.col[first] == np.arange(L.nrows)) and np.all(L.val[~first] == -1.0)
    return L.rowptr, L.col, L.val.copy()


def with_diagonal(oracle, tpl, diag):
    """the template with its diagonal (every row's first entry) set to diag (scalar or per row)"""
    rp, cj, v = tpl
    v = v.copy()
    v[rp[:-1]] = diag
    assert np.all(np.isfinite(v))
    return oracle.Csr(rp.size - 1, rp.size - 1, rp, cj, v)


class Switches:
    """context switches for one registration, put back afterwards"""
    DEFAULTS = {"value_index": 1, "dict_index": 1, "row_pattern": 1, "pair_pattern": 1, "master_pattern": 1}

    def __init__(self, ctx, **off):
        self.ctx, self.off = ctx, off

    def __enter__(self):
        for k, v in self.off.items():
            getattr(self.ctx, "set_" + k)(v)

    def __exit__(self, *exc):
        for k in self.off:
            getattr(self.ctx, "set_" + k)(self.DEFAULTS[k])


class March:
    """The plane march's chunk length and workgroup order (zc, xcd), which the kernels read from
    the context at every launch: held over the registration and the sweeps inside, then put
    back.  None: the context's own."""

    def __init__(self, ctx, setting):
        self.ctx, self.setting = ctx, setting

    def __enter__(self):
        if self.setting:
            self.ctx.set_plane_march(1, *self.setting)

    def __exit__(self, *exc):
        if self.setting:
            self.ctx.set_plane_march(1, -1, 1)


def register(ctx, A, **off):
    with Switches(ctx, **off):
        return ctx.csr(A.nrows, A.ncols, A.rowptr, A.col, A.val)


def forms(M):
    return M.value_index, M.dict_index, M.row_pattern, M.pair_pattern


def on_tile(M, lo, hi, vi):
    """a tile-kernel rung: no dictionary, entries per row in [lo, hi), value index as asked"""
    return (M.dict_index == 0 and M.bsr3 == 0 and lo * M.nrows <= M.nnz < hi * M.nrows
            and (M.value_index > 0) == vi)


# operator -> (template builder, [(tag, registration switches, rung check)], row ranges)
def _variants(name):
    if name == "plain_tile":
        return [("plain", dict(value_index=0), lambda M: forms(M) == (0, 0, 0, 0) and on_tile(M, 0, 64, False))]
    if name == "short_vi":
        return [("vi short", {}, lambda M: on_tile(M, 0, 12, True))]
    if name == "prod_vi":
        return [("vi prod", {}, lambda M: on_tile(M, 12, 64, True))]
    if name == "long":
        return [("long", dict(value_index=0), lambda M: on_tile(M, 64, 1 << 30, False))]
    if name == "long_vi":
        return [("long vi", {}, lambda M: on_tile(M, 64, 1 << 30, True))]
    if name == "stencil":
        return [
            ("dictionary", dict(row_pattern=0), lambda M: M.dict_index > 0 and M.row_pattern == 0),
            ("row pattern", dict(pair_pattern=0), lambda M: M.row_pattern > 0 and M.pair_pattern == 0),
            ("pairs", dict(master_pattern=0), lambda M: M.pair_pattern > 0 and M.master_pattern == 0),
            ("master", {}, lambda M: M.master_pattern == -7 and M.plane_march == 0),
            ("plain", dict(value_index=0), lambda M: forms(M) == (0, 0, 0, 0) and M.master_pattern == 0),
        ]
    if name == "march7":
        return [("march", {}, lambda M: M.march_points == 7 and M.plane_march == 512 and M.master_pattern == -7)]
    raise KeyError(name)


def march_settings(name):
    """(zc, xcd) held over an operator's sweeps: the 7-pt march in one-plane chunks in plain
    workgroup order, and in one chunk that holds the first and the last plane, XCD order"""
    return [(1, 0), (64, 1)] if name == "march7" else [None]


def template(oracle, name):
    if name in ("plain_tile", "short_vi"):
        return random_rows(777, 7, 5, name == "short_vi")
    if name == "prod_vi":
        return random_rows(777, 20, 6, True)
    if name in ("long", "long_vi"):
        return random_rows(300, 90, 7, name == "long_vi")
    if name == "stencil":
        return stencil7(oracle, 13, 7, 5)  # 455 rows: a half pair at the end
    if name == "march7":
        return stencil7(oracle, 32, 16, 3)
    raise KeyError(name)


def row_ranges(name, n):
    return [(0, n), (2, n - 3), (1, n - 2)] if name == "stencil" else [(0, n)]


# ---- the planted right-hand sides ----------------------------------------------------------------
def planted_passes(n, d):
    """right-hand sides of n rows that between them hold every planted operand of d and, one
    per odd run of 128 rows, every fallback operand"""
    xs = dc.operands(d)
    fb = dc.fallback(d)
    odd = [g for g in range((n + RUN - 1) // RUN) if g & 1]
    npass = max(-(-xs.size // n), -(-len(fb) // len(odd)))
    out, k = [], 0
    for p in range(npass):
        f = xs[(p * n + np.arange(n)) % xs.size].copy()
        for g in odd:
            lo, hi = g * RUN, min(n, (g + 1) * RUN)
            f[lo + (37 * g + 11 * p) % (hi - lo)] = fb[k % len(fb)]
            k += 1
        out.append(f)
    assert k >= len(fb) and npass * n >= xs.size
    return out


def check_layout(fs):
    """even runs hold operands in range only, odd runs exactly one that is out of range or +0.0"""
    for f in fs:
        for g in range((f.size + RUN - 1) // RUN):
            run = f[g * RUN:(g + 1) * RUN]
            special = [x for x in run if not dc.in_range(x) or x == 0.0]
            assert len(special) == (g & 1), (g, special)


def quotients(f, diag, rb, re):
    """what one sweep from u = +0.0 with weight 1 must leave: 0.0 + f / a_ii on [rb, re)"""
    want = np.zeros(f.size)
    with np.errstate(all="ignore"):
        want[rb:re] = 0.0 + f[rb:re] / np.broadcast_to(diag, f.shape)[rb:re]
    return want


def sweep(amg, ctx, M, f, u0, w, sweeps, rb, re):
    n = M.nrows
    fv, u, p = ctx.vec(f), ctx.vec(u0), ctx.vec(n)
    try:
        if (rb, re) == (0, n):
            amg.smem.SMEM_Sync_Parfor_Jacobi(ctx, M, fv, u, p, sweeps, 0, w)
        else:
            amg.smem.SMEM_Sync_Jacobi(ctx, M, fv, u, p, sweeps, 0, w, rb, re)
        return u.download()
    finally:
        for v in (fv, u, p):
            v.free()


def oracle_sweep(oracle, A, f, u0, w, sweeps, rb, re):
    # amg_jacobi copies the whole u to u_prev, the oracle's row range only [rb, re): start it equal
    u, p = u0.copy(), u0.copy()
    oracle.smem_jacobi(A, f, u, p, w, sweeps, 0, rb, re)
    return u


def planted_sweeps(amg, ctx, oracle, A, Ms, d, diag, ranges, what):
    """The planted one-sweep runs of the registrations Ms = [(tag, Mat)] of the host operator A
    (divisor d; diag: every row's own diagonal): each output against the quotients and the
    oracle.  Returns the outputs."""
    n = A.nrows
    zero = np.zeros(n)
    fs = planted_passes(n, d)
    check_layout(fs)
    outs = []
    for rb, re in ranges:
        for k, f in enumerate(fs):
            want = quotients(f, diag, rb, re)
            ref = oracle_sweep(oracle, A, f, zero, 1.0, 1, rb, re)
            assert_bitwise(ref, want, f"{what} d={d!r} rows [{rb}, {re}) pass {k}: oracle vs f / d")
            for tag, M in Ms:
                got = sweep(amg, ctx, M, f, zero, 1.0, 1, rb, re)
                assert_bitwise(got, want, f"{what} {tag} d={d!r} rows [{rb}, {re}) pass {k}: f / d")
                outs.append(got)
    return outs


def random_sweeps(amg, ctx, oracle, A, Ms, d, ranges, what):
    """random u, weights 0.7 and 0.8, 2 and 3 sweeps: the products and omega * res, against the oracle"""
    n = A.nrows
    f, u0 = _vecs(n, 61), _vecs(n, 62)
    for rb, re in ranges:
        for w, sweeps in ((0.7, 2), (0.8, 3)):
            ref = oracle_sweep(oracle, A, f, u0, w, sweeps, rb, re)
            assert np.all(np.isfinite(ref)), (what, d)
            for tag, M in Ms:
                got = sweep(amg, ctx, M, f, u0, w, sweeps, rb, re)
                assert_bitwise(got, ref, f"{what} {tag} d={d!r} rows [{rb}, {re}) w={w} sweeps={sweeps}")


def run_operator(amg, ctx, oracle, name, divisors, want_admitted, only=None, random_too=True):
    """Every divisor on every registration of one operator, under each of its march settings;
    the planted outputs.  A divisor's first mismatch ends that divisor only: the others still
    run, and the failure names every divisor that missed."""
    tpl = template(oracle, name)
    outs, missed = [], []
    for d in divisors:
        assert dc.admitted(d) == want_admitted, d
        A = with_diagonal(oracle, tpl, d)
        for setting in march_settings(name):
            Ms = []
            what = name if setting is None else f"{name} zc={setting[0]} xcd={setting[1]}"
            try:
                with March(ctx, setting):
                    for tag, sw, on_rung in _variants(name):
                        if only and tag not in only:
                            continue
                        M = register(ctx, A, **sw)
                        Ms.append((tag, M))
                        assert on_rung(M), (name, tag, d, forms(M), M.master_pattern, M.plane_march, M.march_points,
                                            M.nnz)
                    ranges = row_ranges(name, A.nrows)
                    outs += planted_sweeps(amg, ctx, oracle, A, Ms, d, d, ranges, what)
                    if random_too:
                        random_sweeps(amg, ctx, oracle, A, Ms, d, ranges, what)
            except AssertionError as e:
                missed.append(f"d={d!r} ({what}): {str(e)[:300]}")
            finally:
                for _, M in Ms:
                    M.free()
    assert not missed, f"{len(missed)} divisor runs missed:\n" + "\n".join(missed)
    return outs


@pytest.mark.parametrize("name", ["plain_tile", "short_vi", "prod_vi", "long", "long_vi", "stencil", "march7"])
def test_admitted_divisors(amg, oracle, ctx, name):
    """Every admitted divisor on the rung: the planted sweeps give the division's bits, with the
    reciprocal in the runs that hold operands in range only and the division in the others."""
    run_operator(amg, ctx, oracle, name, dc.ADMITTED, True)


@pytest.mark.parametrize("name,only", [("plain_tile", None), ("stencil", ("master",)), ("march7", None)])
def test_refused_divisors(amg, oracle, ctx, name, only):
    """The divisors that fast_div_of refuses (odd part, exponent window): the division itself
    everywhere.  2^-100 overflows the reciprocal form at 2^959, and 3 * 2^100 rounds its
    subnormal ties another way (div_cases.beyond_window)."""
    run_operator(amg, ctx, oracle, name, dc.REFUSED, False, only)


def test_zero_diagonal_keeps_u(amg, oracle, ctx):
    """a uniform diagonal 0.0 (not normal: refused): a != 0 fails on every row and u stays"""
    A = with_diagonal(oracle, template(oracle, "plain_tile"), 0.0)
    assert not dc.admitted(0.0)
    M = register(ctx, A, value_index=0)
    try:
        f, u0 = _vecs(A.nrows, 63), _vecs(A.nrows, 64)
        got = sweep(amg, ctx, M, f, u0, 1.0, 1, 0, A.nrows)
        assert_bitwise(got, u0, "zero diagonal: u")
        assert_bitwise(oracle_sweep(oracle, A, f, u0, 1.0, 1, 0, A.nrows), u0, "zero diagonal: oracle")
    finally:
        M.free()


# ---- the 27-pt march: a uniform diagonal, and boundary planes with their own ---------------------
@pytest.mark.parametrize("variant", ["uniform", "boundary_planes"])
def test_march27(amg, oracle, ctx, variant):
    """box_27pt(32, 16, 5) with the diagonal d everywhere, or d on the interior planes and d + 1
    on the planes z = 0 and z = nz - 1: there the dominant pattern's diagonal is d, and the
    boundary planes' waves must divide by their own (jac_div2's a == dq test).  Planted operands
    lie in both kinds of plane; the expected quotient uses each row's own diagonal."""
    from test_gpu_march import box_27pt
    nx, ny, nz = 32, 16, 5
    B = box_27pt(oracle, nx, ny, nz)
    tpl = (B.rowptr, B.col, B.val)
    z = np.arange(B.nrows) // (nx * ny)
    edge = (z == 0) | (z == nz - 1)
    for d in dc.ADMITTED:
        assert dc.admitted(d)
        diag = np.where(edge, d + 1.0, d) if variant == "boundary_planes" else np.full(B.nrows, d)
        assert variant == "uniform" or np.all(diag[edge] != d)
        A = with_diagonal(oracle, tpl, diag)
        M = register(ctx, A)
        try:
            assert M.march_points == 27 and M.plane_march == nx * ny and abs(M.master_pattern) == 27, \
                (d, forms(M), M.master_pattern, M.plane_march)
            fs = planted_passes(B.nrows, d)
            # both kinds of plane hold operands in range and fallback operands
            for rows in (edge, ~edge):
                assert any(not dc.in_range(x) for f in fs for x in f[rows])
                assert sum(dc.in_range(x) for x in fs[0][rows]) >= 1000
            planted_sweeps(amg, ctx, oracle, A, [("march27", M)], d, diag, [(0, B.nrows)], variant)
            random_sweeps(amg, ctx, oracle, A, [("march27", M)], d, [(0, B.nrows)], variant)
        finally:
            M.free()


# ---- EpiResJacobi and the fused level-0 marches: whole solves ------------------------------------
SOLVE_DIVISORS = [3.0, 5.0, 7.0, dc.M30 * 2.0 ** -27]  # the last: about 8, so that the sweeps stay tame
CYCLES = 3  # no iterate overflows within 3 cycles for any of the four (asserted: finite)


def _solve(ctx, amg, host, f, fo, reuse):
    """amg_solve over CYCLES cycles, then solve_start + iterate batches of 1 and 2 + get_u"""
    n = f.size
    ctx.set_fuse_outer(fo)
    dev = {k: [ctx.csr(M.nrows, M.ncols, M.rowptr, M.col, M.val) for M in v] for k, v in host.items()}
    opts = amg.default_opts(smooth_weight=0.8, num_cycles=CYCLES, tol=0.0, reuse_outer_residual=reuse)
    H = amg.Hier(ctx, dev["A"], dev["P"], dev["R"], opts)
    fv, uv = ctx.vec(f), ctx.vec(np.zeros(n))
    try:
        assert dev["A"][0].march_points == 7 and dev["A"][0].master_pattern == -7
        sol = H.solve(f)
        hist = [H.solve_start(fv, uv)]
        for b in (1, 2):
            H.iterate(b)
            hist.append(H.resnorm())
        H.get_u(uv)
        return H.fused_outer, sol, uv.download(), np.array(hist)
    finally:
        H.free()
        fv.free()
        uv.free()
        for v in dev.values():
            for M in v:
                M.free()


@pytest.mark.parametrize("reuse", [2, 1])
@pytest.mark.parametrize("d", SOLVE_DIVISORS, ids=["3", "5", "7", "m30"])
def test_solve_divisors(ctx, amg, oracle, d, reuse):
    """The hierarchy of amg.Gen(512, 2, 5) with level 0's operator replaced by the 7-pt stencil
    of diagonal d (off-diagonals -1; the levels are then not Galerkin-consistent: only bit
    equality is asked).  fuse_outer 4 (mz_two_sweep_kernel), 3 (slabs: EpiJacobi + EpiResJacobi
    marches), 1 (mz_sweep_outer_kernel) and 0: iterate and norm history bitwise equal across
    the modes, the iterate bitwise equal to the oracle's, the history to 1e-12 of the oracle's
    (the device sums per-tile partials, as in tests/test_gpu_two_sweep.py).  Random right-hand
    sides only."""
    from oracle import pyoracle as po
    from test_gpu_two_sweep import DEFAULT_FUSE_OUTER, _hierarchy
    assert dc.admitted(d)
    dims = (512, 2, 5)
    host = _hierarchy(amg, dims)
    A0 = host["A"][0]
    first = np.zeros(A0.val.size, bool)
    first[A0.rowptr[:-1]] = True
    assert np.all(A0.col[first] == np.arange(A0.nrows)) and np.all(A0.val[~first] == -1.0)
    A0.val[first] = d
    f = amg.rhs_rand(0, A0.nrows)
    ctx.set_plane_march(1, 1, 1)
    ctx.set_outer_slab(2)
    res = {}
    try:
        for fo in (4, 3, 1, 0):
            res[fo] = _solve(ctx, amg, host, f, fo, reuse)
    finally:
        ctx.set_plane_march(1, -1, 1)
        ctx.set_outer_slab(32)
        ctx.set_fuse_outer(DEFAULT_FUSE_OUTER)
    OH = po.Hier(host["A"], host["P"], host["R"], po.make_opts(smooth_weight=0.8, num_cycles=CYCLES))
    u_cpu, hist_cpu, _ = OH.solve(f)
    assert np.all(np.isfinite(u_cpu)) and np.all(np.isfinite(hist_cpu))
    fo0, (u0, h0, k0), ui0, hi0 = res[0]
    assert fo0 == 0 and k0 == CYCLES
    print(f"d={d!r} reuse={reuse}: |u|max {np.abs(u_cpu).max():.3e}, history vs oracle rel "
          f"{np.max(np.abs(h0[:k0 + 1] - hist_cpu[:k0 + 1]) / hist_cpu[:k0 + 1]):.3e}")
    assert_bitwise(u0, u_cpu, "unfused vs oracle iterate")
    np.testing.assert_allclose(h0[:k0 + 1], hist_cpu[:k0 + 1], rtol=1e-12)
    for fo in (4, 3, 1):
        got, (u1, h1, k1), ui1, hi1 = res[fo]
        assert got == fo and k1 == CYCLES, (fo, got, k1)
        assert_bitwise(u1, u_cpu, f"fuse_outer {fo} vs oracle iterate")
        assert_bitwise(u1, u0, f"fuse_outer {fo} vs unfused iterate")
        assert_bitwise(h1[:k1 + 1], h0[:k0 + 1], f"fuse_outer {fo} norm history")
        assert_bitwise(ui1, u_cpu, f"fuse_outer {fo} iterate batches vs oracle")
        assert_bitwise(ui1, ui0, f"fuse_outer {fo} iterate batches vs unfused")
        assert_bitwise(hi1, hi0, f"fuse_outer {fo} norm history (iterate batches)")


# ---- the fast division off: a fresh process, the same bits ---------------------------------------
HASHED = [("plain_tile", None), ("stencil", ("master",)), ("march7", None)]


def planted_digest(amg, ctx, oracle):
    """SHA-256 over the planted sweeps' outputs of the plain-tile, master and 7-pt march
    operators, every divisor of the table"""
    h = hashlib.sha256()
    for name, only in HASHED:
        for divisors, adm in ((dc.ADMITTED, True), (dc.REFUSED, False)):
            for a in run_operator(amg, ctx, oracle, name, divisors, adm, only, random_too=False):
                h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def child_main():
    from conftest import load_package
    from oracle import pyoracle
    amg = load_package()
    ctx = amg.Context(device=0, nstreams=2)
    print("digest", planted_digest(amg, ctx, pyoracle))
    ctx.close()


def test_fast_div_off_same_bits(amg, oracle, ctx):
    """AMG_FAST_DIV is read once per process: a fresh child with AMG_FAST_DIV=0 (the division
    itself everywhere), under its own time limit, gives the digest of this process, where the
    reciprocal is on by default."""
    want = planted_digest(amg, ctx, oracle)
    env = dict(os.environ, AMG_FAST_DIV="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, cwd=HERE, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}"
    got = [ln.split()[1] for ln in p.stdout.splitlines() if ln.startswith("digest ")]
    assert got == [want], (got, want)


if __name__ == "__main__" and sys.argv[1:] == ["--child"]:
    child_main()
