"""The per-category profile (opts.profile: Hier.profile / DistHier.profile,
what bench.py's breakdown reads) and the event-timed measurement helpers
(amg_matvec_timed, amg_dist_fine_spmv, amg_stream_triad)."""
import ctypes as C
import math
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def check_profile(tag, iterate, profile, sync):
    """iterate(k) runs k cycles of a started solve with opts.profile = 1;
    profile(reset) -> (ms[5], launches[5])"""
    sync()
    profile(True)
    ms0, n0 = profile(True)  # directly after a reset
    assert not np.any(ms0) and not np.any(n0), (ms0, n0)
    out = []
    for k in (3, 6):
        t0 = time.perf_counter()
        iterate(k)
        sync()
        wall_ms = (time.perf_counter() - t0) * 1e3
        ms, n = profile(True)
        assert np.all(np.isfinite(ms))
        assert np.array_equal(ms > 0, n > 0), (ms, n)  # time exactly where there were launches
        assert 0 < ms.sum() <= wall_ms, (ms, wall_ms)
        out.append(n)
    print(f"profile counts {tag}: 3 cycles {out[0].tolist()}, 6 cycles {out[1].tolist()}")
    assert np.array_equal(out[1], 2 * out[0]), out
    assert out[0].sum() > 0
    ms0, n0 = profile(False)
    assert not np.any(ms0) and not np.any(n0), (ms0, n0)


def test_hier_profile(amg, ctx):
    gen = amg.Gen(16)
    L = gen.L
    As = [gen.register(ctx, amg.AMG_GEN_A, l) for l in range(L)]
    Ps = [gen.register(ctx, amg.AMG_GEN_P, l) for l in range(L - 1)]
    Rs = [gen.register(ctx, amg.AMG_GEN_R, l) for l in range(L - 1)]
    opts = amg.default_opts(smooth_weight=0.8, num_cycles=1 << 30, tol=0.0, profile=1)
    H = amg.Hier(ctx, As, Ps, Rs, opts)
    f, u0 = ctx.vec(amg.rhs_rand(0, 16 ** 3)), ctx.vec(16 ** 3)
    H.solve_start(f, u0)
    check_profile("Hier 16^3", H.iterate, H.profile, ctx.sync)
    H.free()
    gen.free()


@pytest.mark.parametrize("n,slab", [(16, False), (32, True)], ids=["rows", "slab"])
def test_dist_profile_and_fine_spmv(amg, n, slab):
    gen = amg.Gen(n)
    opts = amg.default_opts(smooth_weight=0.8, num_cycles=1 << 30, tol=0.0, profile=1)
    c = amg.Context(0, nstreams=2)
    amg.dist.init_rccl(c, 1, 0, lambda b: b)
    D = amg.dist.DistHier(c, gen, opts, slab=slab)
    D.solve_start(amg.rhs_rand(0, n ** 3))
    check_profile(f"DistHier {'slab' if slab else 'rows'} {n}^3", D.iterate, D.profile, c.sync)
    ms = D.fine_spmv_ms(3)
    assert math.isfinite(ms) and ms > 0, ms
    D.free()
    amg.dist.finalize(c)
    c.close()
    gen.free()


def test_matvec_timed_and_triad(amg, ctx):
    gen = amg.Gen(16)
    A = gen.register(ctx, amg.AMG_GEN_A, 0)
    x = ctx.vec(amg.rhs_rand(0, A.ncols))
    y, yt = ctx.vec(A.nrows), ctx.vec(A.nrows)
    amg.check(amg.lib.amg_matvec(ctx.h, A.h, x.h, y.h, 0, A.nrows))
    ms = C.c_double(float("nan"))
    amg.check(amg.lib.amg_matvec_timed(ctx.h, A.h, x.h, yt.h, 3, C.byref(ms)))
    assert math.isfinite(ms.value) and ms.value > 0, ms.value
    assert np.array_equal(yt.download().view(np.uint64), y.download().view(np.uint64))
    gbs = C.c_double(float("nan"))
    amg.check(amg.lib.amg_stream_triad(ctx.h, 1 << 16, 3, C.byref(gbs)))
    assert math.isfinite(gbs.value) and gbs.value > 0, gbs.value
    gen.free()
