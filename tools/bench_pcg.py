"""AMG-preconditioned CG (amg_pcg_*) against the stationary cycle on one MI355X.

For each size n (the bench's n^3 7-pt hierarchy, MULT V(1,1) Jacobi) in one
process, one JSON line per size (also written to --out DIR/pcg_<n>.json):

1. ms per amg_pcg_iterate step, per amg_solve_iterate step (the bench's
   options, reuse_outer_residual 2) and per fine SpMV; the legs alternate in
   every repetition, and min / median / max over the repetitions are reported.
2. PCG's own vector time: step - cycle - SpMV, and the share of the time its
   bytes take at 8 TB/s that it amounts to.  The cycle alone is
   amg_precond_apply less its two vector copies (timed as amg_vec_copy).  Inside
   a PCG step the residual update also writes the cycle's zero-guess sweep of
   level 0 (8 n bytes more: 112 n), and the cycle loses its clear of u (8 n) and
   that sweep (24 n); those 32 n bytes are priced at the copy kernel's rate
   (16 n per copy) and taken off the cycle.
3. The same recurrence driven from Python through amg_precond_apply,
   amg_matvec, amg_vec_dot and amg_vec_axpy / amg_vec_scale (three host syncs
   per iteration), and the ratio fused / composed.
4. Iterations and wall time to relres 1e-9 for PCG and the stationary cycle
   (both reading the norm back every iteration).  The Chebyshev-accelerated
   cycle is left out: bench.py does not estimate mu and delta, so there is no
   bench setting to follow.

Every time is a host clock around work that ends in a stream synchronise (the
library owns its stream), over windows of --steps iterations after a warm-up.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from conftest import load_package  # noqa: E402

HBM_PEAK = 8.0e12
PCG_BYTES_PER_ROW = 104  # p.q 16, x / r update 48, r.z 16, p update 24
FOLD_BYTES_PER_ROW = 8   # the cycle's level-0 zero-guess sweep written by the x / r update


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs), "reps": len(xs)}


def timed(ctx, fn, steps):
    """ms per step of fn(steps), bracketed by stream synchronises"""
    ctx.sync()
    t = time.perf_counter()
    fn(steps)
    ctx.sync()
    return (time.perf_counter() - t) * 1e3 / steps


def composed_pcg(amg, ctx, H, A, f, x, iters):
    """the recurrence through the public vector entry points; returns the norm history"""
    lib, n = amg.lib, A.nrows
    r, z, p, q = (amg.Vec(ctx, n) for _ in range(4))
    out = C.c_double()

    def dot(a, b):
        amg.check(lib.amg_vec_dot(ctx.h, a.h, b.h, C.byref(out)))
        return out.value

    amg.check(lib.amg_spgemv(ctx.h, A.h, x.h, f.h, -1.0, 1.0, r.h, 0, n))
    H.precond_apply(r, z)
    amg.check(lib.amg_vec_copy(ctx.h, z.h, p.h))
    rho = dot(r, z)
    hist = [dot(r, r) ** 0.5]
    for _ in range(iters):
        amg.check(lib.amg_matvec(ctx.h, A.h, p.h, q.h, 0, n))
        pq = dot(p, q)
        alpha = rho / pq if pq != 0.0 else 0.0
        amg.check(lib.amg_vec_axpy(ctx.h, alpha, p.h, x.h))
        amg.check(lib.amg_vec_axpy(ctx.h, -alpha, q.h, r.h))
        hist.append(dot(r, r) ** 0.5)
        H.precond_apply(r, z)
        rho_new = dot(r, z)
        beta = rho_new / rho if rho != 0.0 else 0.0
        rho = rho_new
        amg.check(lib.amg_vec_scale(ctx.h, beta, p.h))
        amg.check(lib.amg_vec_axpy(ctx.h, 1.0, z.h, p.h))
    ctx.sync()
    for v in (r, z, p, q):
        v.free()
    return hist


def run_size(amg, n, a):
    ctx = amg.Context(device=0, nstreams=4)
    gen = amg.Gen(n, interp=amg.AMG_INTERP_LINEAR)
    L = gen.L
    As = [gen.register(ctx, amg.AMG_GEN_A, l) for l in range(L)]
    Ps = [gen.register(ctx, amg.AMG_GEN_P, l) for l in range(L - 1)]
    Rs = [gen.register(ctx, amg.AMG_GEN_R, l) for l in range(L - 1)]
    n0 = As[0].nrows
    stat_opts = amg.default_opts(smooth_weight=a.smooth_weight, num_cycles=1 << 30, tol=0.0,
                                 reuse_outer_residual=2)
    pcg_opts = amg.default_opts(smooth_weight=a.smooth_weight, num_cycles=1 << 30, tol=0.0)
    Hs = amg.Hier(ctx, As, Ps, Rs, stat_opts)
    Hp = amg.Hier(ctx, As, Ps, Rs, pcg_opts)
    f = ctx.vec(amg.rhs_rand(0, n0))
    x0, y, z = ctx.vec(n0), ctx.vec(n0), ctx.vec(n0)
    lib = amg.lib

    def spmv(k):
        for _ in range(k):
            amg.check(lib.amg_matvec(ctx.h, As[0].h, f.h, y.h, 0, n0))

    def apply_m(k):
        for _ in range(k):
            Hp.precond_apply(f, z)

    def vcopy(k):
        for _ in range(k):
            amg.check(lib.amg_vec_copy(ctx.h, f.h, y.h))

    legs = {"pcg_step": Hp.pcg_iterate, "stationary_step": Hs.iterate, "fine_spmv": spmv,
            "precond_apply": apply_m, "vec_copy": vcopy}
    ms = {k: [] for k in legs}
    ms["composed_step"] = []
    for rep in range(a.reps + 1):  # repetition 0 warms every leg up
        x0.set(0.0)
        Hs.solve_start(f, x0)
        Hs.iterate(a.warmup)
        t_stat = timed(ctx, Hs.iterate, a.steps)
        Hp.pcg_start(f, x0)
        Hp.pcg_iterate(a.warmup)
        t = {"stationary_step": t_stat, "pcg_step": timed(ctx, Hp.pcg_iterate, a.steps)}
        for k in ("fine_spmv", "precond_apply", "vec_copy"):
            t[k] = timed(ctx, legs[k], a.steps)
        x0.set(0.0)
        t["composed_step"] = timed(ctx, lambda k: composed_pcg(amg, ctx, Hp, As[0], f, x0, k), a.steps)
        if rep:
            for k, v in t.items():
                ms[k].append(v)
    med = {k: statistics.median(v) for k, v in ms.items()}
    cycle = med["precond_apply"] - 2.0 * med["vec_copy"]
    cycle_in_pcg = cycle - 2.0 * med["vec_copy"]  # MULT Jacobi: the fold applies
    own = med["pcg_step"] - cycle_in_pcg - med["fine_spmv"]
    own_bytes = PCG_BYTES_PER_ROW + FOLD_BYTES_PER_ROW
    ideal = own_bytes * n0 / HBM_PEAK * 1e3

    # time to relres 1e-9, the norm read back every iteration in both
    to_tol = {}
    # (the split forms, so that no vector crosses the bus inside the window)
    for name, start, step, norm in (("pcg", Hp.pcg_start, Hp.pcg_iterate, Hp.pcg_resnorm),
                                    ("stationary", Hs.solve_start, Hs.iterate, Hs.resnorm)):
        walls, its, rel = [], 0, None
        for rep in range(a.reps + 1):
            x0.set(0.0)
            ctx.sync()
            t0 = time.perf_counter()
            r0 = start(f, x0)
            its, rel = 0, 1.0
            while rel >= 1e-9 and its < a.max_iters:
                step(1)
                its += 1
                rel = norm() / r0
            wall = (time.perf_counter() - t0) * 1e3
            if rep:
                walls.append(wall)
        to_tol[name] = {"iterations": its, "relres": rel, "reached": bool(rel < 1e-9), "wall_ms": spread(walls)}
    out = {
        "n": n, "rows": n0, "levels": L, "steps": a.steps, "warmup": a.warmup,
        "workload": f"{n}^3 7-pt Laplacian, MULT V(1,1) Jacobi w={a.smooth_weight}, {L}-level linear hierarchy",
        "ms": {k: spread(v) for k, v in ms.items()},
        "pcg_over_stationary_step": med["pcg_step"] / med["stationary_step"],
        "cycle_ms": cycle,
        "cycle_in_pcg_ms": cycle_in_pcg,
        "pcg_own_vector_ms": own,
        "pcg_own_bytes_per_row": own_bytes,
        "pcg_own_ideal_ms_at_8TBs": ideal,
        "pcg_own_frac_of_peak": ideal / own if own > 0 else None,
        "fused_over_composed": med["pcg_step"] / med["composed_step"],
        "to_relres_1e-9": to_tol,
        "chebyshev": "not run: bench.py sets no mu / delta (it does not call amg_eigs_power)",
        "timing": "host clock around stream-synchronised windows",
    }
    for H in (Hs, Hp):
        H.free()
    for v in (f, x0, y, z):
        v.free()
    for M in As + Ps + Rs:
        M.free()
    gen.free()
    ctx.close()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--max-iters", type=int, default=200)
    p.add_argument("--smooth-weight", type=float, default=0.8)
    p.add_argument("--out", default=None, help="directory for pcg_<n>.json")
    a = p.parse_args()
    amg = load_package()
    for n in a.sizes:
        out = run_size(amg, n, a)
        print(json.dumps(out), flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, f"pcg_{n}.json"), "w") as fh:
                json.dump(out, fh, indent=1)
                fh.write("\n")


if __name__ == "__main__":
    main()
