"""sha256 digests of the synchronous distributed solve, to compare two commits bit for bit.

For a fixed list of cases of tests/test_gpu_dist.py (row-partitioned form) and
tests/test_gpu_slab.py (z-slab form), plus accelerated MULT at 64^3 on both
forms, prints one line per case: the sha256 of the gathered iterate's bytes and
of the residual-norm history's bytes (float64, one norm per cycle, the initial
one first).  The tests pin the norms to 1e-12 only; the digest also pins the
order in which the norm partials are summed.

    python tools/dist_digest.py > digest.txt      # on either commit, then diff
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from conftest import load_package  # noqa: E402
import test_gpu_dist as td  # noqa: E402
import test_gpu_slab as ts  # noqa: E402

ROWS = (2, 3, 4, 6)     # 4 ranks, ragged 3 ranks, aggregate, reuse_outer_residual 0
SLAB = (0, 3, 4, 5, 8)  # 2 ranks, ragged, not fused, CSR transfers, pre 2 / post 3 sweeps


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def case_opts(amg, cycles, extra):
    kw = dict(extra)
    if kw.pop("smoother", None) == "l1":
        kw["smoother"] = amg.AMG_L1_JACOBI
    return amg.default_opts(num_cycles=cycles, tol=0.0, **kw)


def main():
    amg = load_package()

    def report(tag, u, hist):
        print(f"{tag}: iterate {sha(u)} norms {sha(hist)} last {hist[-1]:.17e}", flush=True)

    for form, cases, picks, cycles in (("rows", td.CASES, ROWS, 8), ("slab", ts.CASES, SLAB, 6)):
        for i in picks:
            dims, interp, nranks, rep, extra = cases[i][:5]
            it = amg.AMG_INTERP_AGGREGATE if interp == "aggregate" else amg.AMG_INTERP_LINEAR
            gen = amg.Gen(dims[0], dims[1], dims[2], interp=it)
            f = amg.rhs_rand(0, dims[0] * dims[1] * dims[2])
            opts = case_opts(amg, cycles, extra)
            if form == "rows":
                u, hist = td.distributed(amg, gen, opts, f, cycles, nranks, rep)
            else:
                u, hist = ts.slab_ranks(amg, gen, opts, f, cycles, nranks, rep)
            report(f"{form} case {i} {dims} {interp} {nranks} ranks {extra}", u, hist)
            gen.free()
    # accelerated MULT (the Richardson update), 64^3, 2 ranks, both forms
    mu, delta = td.cheby_scalars(0.5, 4.0)
    opts = amg.default_opts(num_cycles=5, tol=0.0, smooth_weight=0.8, accel_type=amg.AMG_RICHARD_ACCEL,
                            cheby_mu=mu, cheby_delta=delta)
    gen = amg.Gen(64)
    f = amg.rhs_rand(0, 64 ** 3)
    report("rows accelerated 64^3 2 ranks", *td.distributed(amg, gen, opts, f, 5, 2, 1 << 12))
    report("slab accelerated 64^3 2 ranks", *ts.slab_ranks(amg, gen, opts, f, 5, 2, 1 << 12))
    gen.free()


if __name__ == "__main__":
    main()
