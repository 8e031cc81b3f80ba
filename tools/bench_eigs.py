"""One iteration of the CG-Lanczos eigenvalue estimate (amg_eigs_cg) on one MI355X, beside the
fine SpMV alone and the same recurrence assembled from the public vector entries.

For each size n (the n^3 7-pt operator of the bench's generator) in one process, one JSON line
per size (also written to --out DIR/eigs_<n>.json):

1. fused: ms per iteration of amg_eigs_cg.  A call allocates, forms and uploads the start vector
   and reads the history back, so the iteration is the slope between a call of --long and one of
   --short iterations from the same start (host clock; the call ends in a stream synchronise).
2. fine_spmv: ms per amg_matvec on the same operator.
3. composed: the same recurrence through amg_matvec, amg_vec_dot (a host sync each),
   amg_vec_axpy, amg_vec_scale and amg_vec_ivaxpy -- scale p, p += r ./ d, SpMV, dot, axpy,
   clear z, z += r ./ d, dot: 144 n bytes of vector traffic, what hypre's sequence (copy, dot, p,
   u, SpMV, s, dot, axpy) moves too.  Its alpha history must equal the fused one bit for bit.
4. The byte model: (80 n + SpMV) / (144 n + SpMV) with the SpMV's bytes taken from its time at the
   rate the vector kernels reach (fused - SpMV over 80 n).

The legs alternate in every repetition; min / median / max over the repetitions are reported.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from conftest import load_package  # noqa: E402

FUSED_BYTES_PER_ROW = 80      # p update 32, p.q 16, r update + gamma 32
COMPOSED_BYTES_PER_ROW = 144  # scale 16, p += r./d 32, p.q 16, axpy 24, clear 8, z += r./d 32, r.z 16


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs), "reps": len(xs)}


def wall_ms(ctx, fn):
    ctx.sync()
    t = time.perf_counter()
    out = fn()
    ctx.sync()
    return (time.perf_counter() - t) * 1e3, out


def composed(amg, ctx, A, d, r0, iters):
    """the recurrence of amg_eigs_cg (scale 1) through the public entries; returns alpha"""
    lib, n = amg.lib, A.nrows
    r, p, q, z = (amg.Vec(ctx, n) for _ in range(4))
    out = C.c_double()

    def dot(a, b):
        amg.check(lib.amg_vec_dot(ctx.h, a.h, b.h, C.byref(out)))
        return out.value

    def divide(dst):  # dst = r ./ d on a cleared dst
        amg.check(lib.amg_vec_ivaxpy(ctx.h, r.h, d.h, dst.h))

    amg.check(lib.amg_vec_copy(ctx.h, r0.h, r.h))
    p.set(0.0)
    z.set(0.0)
    divide(z)
    gam, beta, alphas = dot(r, z), 0.0, []
    for _ in range(iters):
        amg.check(lib.amg_vec_scale(ctx.h, beta, p.h))
        divide(p)
        amg.check(lib.amg_matvec(ctx.h, A.h, p.h, q.h, 0, n))
        pq = dot(p, q)
        alpha = gam / pq if pq != 0.0 else 0.0
        amg.check(lib.amg_vec_axpy(ctx.h, -alpha, q.h, r.h))
        z.set(0.0)
        divide(z)
        gnew = dot(r, z)
        beta = gnew / gam if gam != 0.0 else 0.0
        gam = gnew
        alphas.append(alpha)
    ctx.sync()
    for v in (r, p, q, z):
        v.free()
    return np.array(alphas)


def run_size(amg, n, a):
    ctx = amg.Context(device=0, nstreams=4)
    gen = amg.Gen(n, interp=amg.AMG_INTERP_LINEAR)
    A = gen.register(ctx, amg.AMG_GEN_A, 0)
    n0 = A.nrows
    start = 2.0 * amg.lehmer_stream(n0) - 1.0
    r0, x, y, d = ctx.vec(start), ctx.vec(start), ctx.vec(n0), ctx.vec(n0)
    amg.check(amg.lib.amg_a_diag(ctx.h, A.h, 1.0, d.h))
    span = a.long - a.short

    def spmv():
        for _ in range(span):
            amg.check(amg.lib.amg_matvec(ctx.h, A.h, x.h, y.h, 0, n0))

    ms = {"fused": [], "fine_spmv": [], "composed": []}
    alpha_f = alpha_c = None
    for rep in range(a.reps + 1):  # repetition 0 warms every leg up
        t_short, _ = wall_ms(ctx, lambda: ctx.eigs_cg(A, a.short, 1, start))
        t_long, res = wall_ms(ctx, lambda: ctx.eigs_cg(A, a.long, 1, start))
        t_spmv, _ = wall_ms(ctx, spmv)
        c_short, _ = wall_ms(ctx, lambda: composed(amg, ctx, A, d, r0, a.short))
        c_long, alpha_c = wall_ms(ctx, lambda: composed(amg, ctx, A, d, r0, a.long))
        alpha_f = res[2]
        if rep:
            ms["fused"].append((t_long - t_short) / span)
            ms["fine_spmv"].append(t_spmv / span)
            ms["composed"].append((c_long - c_short) / span)
    med = {k: statistics.median(v) for k, v in ms.items()}
    vec_rate = FUSED_BYTES_PER_ROW * n0 / ((med["fused"] - med["fine_spmv"]) * 1e-3)
    spmv_rows = med["fine_spmv"] * 1e-3 * vec_rate / n0  # the SpMV as bytes per row at that rate
    out = {
        "n": n, "rows": n0, "plane_march": A.plane_march, "short": a.short, "long": a.long,
        "workload": f"{n}^3 7-pt Laplacian, amg_eigs_cg scale 1, default start",
        "ms_per_iteration": {k: spread(v) for k, v in ms.items()},
        "fused_over_composed": med["fused"] / med["composed"],
        "fused_over_spmv": med["fused"] / med["fine_spmv"],
        "vector_kernels_GBs": vec_rate / 1e9,
        "byte_model_ratio": (FUSED_BYTES_PER_ROW + spmv_rows) / (COMPOSED_BYTES_PER_ROW + spmv_rows),
        "alpha_bitwise_equal": bool(np.array_equal(alpha_f.view(np.uint64), alpha_c.view(np.uint64))),
        "emax": res[0], "emin": res[1], "k": res[5],
        "timing": "host clock around stream-synchronised calls; per iteration = slope between long and short",
    }
    for v in (r0, x, y, d):
        v.free()
    A.free()
    gen.free()
    ctx.close()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", type=int, nargs="+", default=[256])
    p.add_argument("--short", type=int, default=20)
    p.add_argument("--long", type=int, default=120)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None, help="directory for eigs_<n>.json")
    a = p.parse_args()
    amg = load_package()
    for n in a.sizes:
        out = run_size(amg, n, a)
        print(json.dumps(out), flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, f"eigs_{n}.json"), "w") as fh:
                json.dump(out, fh, indent=1)
                fh.write("\n")


if __name__ == "__main__":
    main()
