"""Level 0's last post-smoothing sweep and the outer residual + the next
cycle's first sweep as one register march (mz_two_sweep_kernel, fuse_outer 4):
a 256-lane workgroup keeps two adjacent lines and their two halo lines of u
and u' in registers, sweep 1 one plane ahead of sweep 2, wave edges through
LDS.  Every output is bit-identical to the two separate marches
(csr_mz_kernel<EpiJacobi> then csr_mz_kernel<EpiResJacobi>) and to the oracle."""
import numpy as np
import pytest

from test_gpu_kernels import assert_bitwise

pytestmark = pytest.mark.gpu

DEFAULT_FUSE_OUTER = 4  # amg_ctx::fuse_outer


def _hierarchy(amg, dims):
    from oracle import pyoracle as po
    g = amg.Gen(*dims, interp=amg.AMG_INTERP_LINEAR)
    return {w: [po.Csr(*g.host_csr(c, l)) for l in range(cnt)]
            for w, c, cnt in (("A", amg.AMG_GEN_A, g.L), ("P", amg.AMG_GEN_P, g.L - 1),
                              ("R", amg.AMG_GEN_R, g.L - 1))}


def _run(ctx, amg, host, f, fo, post, reuse):
    """amg_solve over 6 cycles, then solve_start + iterate batches of 2, 3, 1 + get_u"""
    n = f.size
    ctx.set_fuse_outer(fo)
    dev = {k: [ctx.csr(M.nrows, M.ncols, M.rowptr, M.col, M.val) for M in v] for k, v in host.items()}
    opts = amg.default_opts(smooth_weight=0.8, num_cycles=6, tol=0.0, reuse_outer_residual=reuse,
                            num_post_smooth_sweeps=post)
    H = amg.Hier(ctx, dev["A"], dev["P"], dev["R"], opts)
    try:
        sol = H.solve(f)
        fv, uv = ctx.vec(f), ctx.vec(np.zeros(n))
        hist = [H.solve_start(fv, uv)]
        for b in (2, 3, 1):
            H.iterate(b)
            hist.append(H.resnorm())
        H.get_u(uv)
        return H.fused_outer, sol, uv.download(), np.array(hist)
    finally:
        H.free()
        for v in dev.values():
            for M in v:
                M.free()


# every line has wave edges at x = 128, 256 and 384
@pytest.mark.parametrize("dims,zc,post,reuse", [
    ((512, 2, 5), 1, 1, 2),    # ny = the line group: both sweep-1 halo lines outside the box; one-plane
                               # chunks: both z-halo planes recomputed at every plane
    ((512, 6, 10), 4, 1, 2),   # low, interior and high line groups; chunks 4 + 4 + 2
    ((512, 8, 7), 3, 2, 1),    # r stored; a second post sweep before the deferred one
    ((512, 4, 3), 64, 1, 2),   # one chunk holding the first and the last plane
    ((512, 16, 12), 5, 1, 1),  # many line groups, ragged chunks
])
def test_two_sweep_outer(ctx, amg, oracle, dims, zc, post, reuse):
    """fuse_outer 4 against fuse_outer 0 and the oracle: amg_solve's iterate and
    norm history, and the iterate and norms of iterate batches (u' stored only
    in a batch's last step), bit for bit."""
    from oracle import pyoracle as po
    host = _hierarchy(amg, dims)
    f = amg.rhs_rand(0, dims[0] * dims[1] * dims[2])
    ctx.set_plane_march(1, zc, 1)
    try:
        fo1, (u1, h1, k1), ui1, hi1 = _run(ctx, amg, host, f, 4, post, reuse)
        fo0, (u0, h0, k0), ui0, hi0 = _run(ctx, amg, host, f, 0, post, reuse)
    finally:
        ctx.set_plane_march(1, -1, 1)
        ctx.set_fuse_outer(DEFAULT_FUSE_OUTER)
    assert fo1 == 4 and fo0 == 0, (fo1, fo0)
    OH = po.Hier(host["A"], host["P"], host["R"], po.make_opts(smooth_weight=0.8, num_cycles=6, num_post=post))
    u_cpu, hist_cpu, _ = OH.solve(f)
    assert k1 == 6 and k0 == 6, (k1, k0)
    assert_bitwise(u1, u0, "fused vs unfused iterate")
    assert_bitwise(u1, u_cpu, "fused vs oracle iterate")
    assert_bitwise(h1[:k1 + 1], h0[:k0 + 1], "norm history")
    np.testing.assert_allclose(h1[:k1 + 1], hist_cpu[:k1 + 1], rtol=1e-12)
    assert_bitwise(ui1, ui0, "fused vs unfused iterate (iterate batches)")
    assert_bitwise(ui1, u_cpu, "fused iterate batches vs oracle")
    assert_bitwise(hi1, hi0, "norm history (iterate batches)")


def test_two_sweep_falls_back(ctx, amg, oracle):
    """lines of 64 points are not the register march's: fuse_outer 4 reports 0
    and solves bit-identically to mode 0"""
    host = _hierarchy(amg, (64, 64, 64))
    f = amg.rhs_rand(0, 64 ** 3)
    try:
        fo1, (u1, h1, k1), ui1, hi1 = _run(ctx, amg, host, f, 4, 1, 2)
        fo0, (u0, h0, k0), ui0, hi0 = _run(ctx, amg, host, f, 0, 1, 2)
    finally:
        ctx.set_fuse_outer(DEFAULT_FUSE_OUTER)
    assert fo1 == 0 and fo0 == 0, (fo1, fo0)
    assert_bitwise(u1, u0, "iterate")
    assert_bitwise(h1[:k1 + 1], h0[:k0 + 1], "norm history")
    assert_bitwise(ui1, ui0, "iterate (iterate batches)")
    assert_bitwise(hi1, hi0, "norm history (iterate batches)")
