"""K right-hand sides at once (amg_mrhs_*) against the single-vector cycle on one MI355X.

Cases, all in one process, one JSON line each (also written to --out DIR/<case>.json):

* the n^3 7-pt hierarchy on the general path, built the way bench.py's
  general_csr_vcycle builds it (compressed forms off, CSR transfers): n = 256 by
  default, and 512 at K = 4 with --big;
* the classical hierarchy of the elasticity problem at --refine (default 5).

Per K in {2, 4, 8} three legs alternate in every repetition (tools/bench_pcg.py's
timed / spread pattern; repetition 0 warms every leg up and is dropped):

1. the single-vector V-cycle on plain CSR (every compressed form off),
2. the single-vector V-cycle with the default forms,
3. the K-column cycle (plain CSR always).

A leg is one whole stationary solve of --steps cycles -- InitVectors, the first
outer residual, then per cycle the V-cycle and the outer residual with its norm --
inside one host-clock window that ends in a stream synchronise; ms per cycle is the
window over --steps, so each leg carries its solve's start the same way.  The same
three legs are then timed for the PCG iteration (amg_pcg_* / amg_mrhs_pcg_solve).
Reported: min / median / max ms per cycle, ms per right-hand side, the byte-model
bound at 8 TB/s (plain CSR bytes, gathers excluded), and the gate of the K = 4 cycle:
max(multi) / 4 < min(single, plain CSR).
"""
import argparse
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

HBM_PEAK = 8.0e12
PCG_BYTES_PER_ROW = 104  # p.q 16, x / r update 48, r.z 16, p update 24


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs), "reps": len(xs)}


def timed(ctx, fn, steps):
    """ms per step of fn(), a window of `steps` steps bracketed by stream synchronises"""
    ctx.sync()
    t = time.perf_counter()
    fn()
    ctx.sync()
    return (time.perf_counter() - t) * 1e3 / steps


def plain_context(amg):
    """every compressed form, the plane march, the geometric / fused transfers and the 3x3
    blocks off: each operator plain CSR, as bench.py's general_csr_vcycle sets it"""
    ctx = amg.Context(device=0, nstreams=4)
    for fn in (ctx.set_value_index, ctx.set_dict_index, ctx.set_row_pattern, ctx.set_pair_pattern,
               ctx.set_master_pattern, ctx.set_fuse_transfer, ctx.set_bsr3):
        fn(0)
    ctx.set_plane_march(0)
    return ctx


# ---- the byte model: plain CSR, 12 B per entry + 4 B per row of matrix read once per launch
# for all K columns, 8 B per vector element streamed; gathers of x excluded ----
def op_bytes(M, K, vecs):
    return 12 * M.nnz + 4 * M.nrows + 8 * vecs * M.nrows * K


def cycle_bytes(As, Ps, Rs, K, precond):
    """one V(1,1) cycle: pre sweep (the zero-guess sweep, 16 B per element + a_ii, on levels
    > 0 and on level 0 as a preconditioner), residual, restriction; two sweeps on the
    coarsest level; prolongation + correction, post sweep"""
    L, b = len(As), 0
    for l in range(L - 1):
        zero = l > 0 or precond
        b += (8 * As[l].nrows + 16 * As[l].nrows * K) if zero else op_bytes(As[l], K, 3)
        b += op_bytes(As[l], K, 2)       # r = f - A u
        b += op_bytes(Rs[l], K, 1)       # f_c = R r (r gathered)
        b += op_bytes(Ps[l], K, 2)       # u += P e
        b += op_bytes(As[l], K, 3)       # post sweep
    b += 2 * op_bytes(As[-1], K, 3)
    return b


def solve_cycle_bytes(As, Ps, Rs, K):
    """a cycle of the stationary solve: the V-cycle, the outer residual and its norm"""
    return cycle_bytes(As, Ps, Rs, K, False) + op_bytes(As[0], K, 2) + 8 * As[0].nrows * K


def pcg_iter_bytes(As, Ps, Rs, K):
    """a PCG iteration: q = A p, the recurrence's vector passes, the cleared iterates, M^-1"""
    clear = sum(8 * A.nrows * K for A in As)
    return op_bytes(As[0], K, 1) + PCG_BYTES_PER_ROW * As[0].nrows * K + clear + cycle_bytes(As, Ps, Rs, K, True)


def bound_ms(nbytes):
    return nbytes / HBM_PEAK * 1e3


def run_case(amg, name, workload, register, n0, rhs, widths, a, omega):
    """register(ctx) -> (As, Ps, Rs) on that context; rhs(j) -> right-hand side j (host)"""
    ctx_p, ctx_d = plain_context(amg), amg.Context(device=0, nstreams=4)
    t0 = time.time()
    mp, md = register(ctx_p), register(ctx_d)
    As, Ps, Rs = mp
    assert As[0].value_index == 0 and As[0].plane_march == 0 and As[0].bsr3 == 0
    big = 1 << 30
    stat = dict(smooth_weight=omega, tol=0.0)
    H1 = amg.Hier(ctx_p, *mp, amg.default_opts(num_cycles=big, reuse_outer_residual=2, **stat))
    Hd = amg.Hier(ctx_d, *md, amg.default_opts(num_cycles=big, reuse_outer_residual=2, **stat))
    Hp1 = amg.Hier(ctx_p, *mp, amg.default_opts(num_cycles=big, **stat))
    Hpd = amg.Hier(ctx_d, *md, amg.default_opts(num_cycles=big, **stat))
    Hm = amg.Hier(ctx_p, *mp, amg.default_opts(num_cycles=a.steps, check_resnorm=0, **stat))
    assert H1.fused == 0
    setup_s = time.time() - t0
    f0 = rhs(0)
    f_p, f_d = ctx_p.vec(f0), ctx_d.vec(f0)
    u_p, u_d = ctx_p.vec(n0), ctx_d.vec(n0)
    out = {"case": name, "workload": workload, "rows": n0, "nnz": int(As[0].nnz), "levels": len(As),
           "entries_per_row": As[0].nnz / n0, "steps": a.steps, "reps": a.reps, "setup_s": setup_s,
           "default_forms": {"value_index": md[0][0].value_index, "plane_march": md[0][0].plane_march,
                             "bsr3": md[0][0].bsr3, "fused": Hd.fused},
           "timing": "host clock around one whole solve of `steps` cycles / iterations, stream-synchronised",
           "hbm_peak": HBM_PEAK, "widths": {}}

    def single(H, ctx, f, u, pcg):
        def go():
            u.set(0.0)
            if pcg:
                H.pcg_start(f, u)
                H.pcg_iterate(a.steps)
            else:
                H.solve_start(f, u)
                H.iterate(a.steps)
        return timed(ctx, go, a.steps)

    for K in widths:
        F = ctx_p.mvec(np.ascontiguousarray(np.stack([rhs(j) for j in range(K)], axis=1)))
        U = ctx_p.mvec((n0, K))

        def multi(pcg):
            def go():
                U.set(0.0)
                (Hm.mrhs_pcg_solve if pcg else Hm.mrhs_solve)(F, U)
            return timed(ctx_p, go, a.steps)

        res = {}
        for kind, pcg, Hs, Hdef, nbytes in (("cycle", False, H1, Hd, solve_cycle_bytes),
                                            ("pcg_iteration", True, Hp1, Hpd, pcg_iter_bytes)):
            ms = {"single_plain_csr": [], "single_default_forms": [], "multi": []}
            for rep in range(a.reps + 1):  # repetition 0 warms every leg up
                t = {"single_plain_csr": single(Hs, ctx_p, f_p, u_p, pcg),
                     "single_default_forms": single(Hdef, ctx_d, f_d, u_d, pcg),
                     "multi": multi(pcg)}
                if rep:
                    for k, v in t.items():
                        ms[k].append(v)
            b1, bK = bound_ms(nbytes(As, Ps, Rs, 1)), bound_ms(nbytes(As, Ps, Rs, K)) / K
            per_rhs = [v / K for v in ms["multi"]]
            res[kind] = {
                "ms": {k: spread(v) for k, v in ms.items()},
                "multi_ms_per_rhs": spread(per_rhs),
                "speedup_per_rhs_vs_plain_csr": statistics.median(ms["single_plain_csr"]) / statistics.median(per_rhs),
                "speedup_per_rhs_vs_default_forms": statistics.median(ms["single_default_forms"])
                / statistics.median(per_rhs),
                "beats_plain_csr_in_every_rep": max(per_rhs) < min(ms["single_plain_csr"]),
                "byte_model_bound_ms": {"single_plain_csr": b1, "multi_per_rhs": bK, "ratio": b1 / bK},
                "multi_per_rhs_over_bound": statistics.median(per_rhs) / bK,
                "single_plain_csr_over_bound": statistics.median(ms["single_plain_csr"]) / b1,
            }
        out["widths"][str(K)] = res
        F.free()
        U.free()
    if "4" in out["widths"]:
        out["gate_k4_cycle"] = out["widths"]["4"]["cycle"]["beats_plain_csr_in_every_rep"]
    for H in (H1, Hd, Hp1, Hpd, Hm):
        H.free()
    for v in (f_p, f_d, u_p, u_d):
        v.free()
    for ms_ in (mp, md):
        for lst in ms_:
            for M in lst:
                M.free()
    ctx_p.close()
    ctx_d.close()
    return out


def case_7pt(amg, n, widths, a):
    gen = amg.Gen(n, interp=amg.AMG_INTERP_LINEAR)
    L = gen.L

    def register(ctx):
        return ([gen.register(ctx, amg.AMG_GEN_A, l) for l in range(L)],
                [gen.register(ctx, amg.AMG_GEN_P, l) for l in range(L - 1)],
                [gen.register(ctx, amg.AMG_GEN_R, l) for l in range(L - 1)])

    n0 = n ** 3
    out = run_case(amg, f"7pt_{n}", f"{n}^3 7-pt Laplacian, MULT V(1,1) Jacobi w={a.smooth_weight}, {L}-level linear "
                   "hierarchy, CSR transfers", register, n0, lambda j: amg.rhs_rand(j * n0, (j + 1) * n0), widths, a,
                   a.smooth_weight)
    gen.free()
    return out


def case_elasticity(amg, refine, widths, a):
    n, rp, cj, v, b = amg.classical.elasticity(refine)[:5]
    cl = amg.classical.ClassicalAMG(n, rp, cj, v, coarsen_type=9, strong_threshold=0.5, num_functions=3, device=0,
                                    setup_on_device=1)
    L = cl.L

    def register(ctx):
        return ([cl.register(ctx, amg.AMG_GEN_A, l) for l in range(L)],
                [cl.register(ctx, amg.AMG_GEN_P, l) for l in range(L - 1)],
                [cl.register(ctx, amg.AMG_GEN_R, l) for l in range(L - 1)])

    def rhs(j):  # the problem's load, then random loads
        return b if j == 0 else amg.rhs_rand(j * n, (j + 1) * n)

    out = run_case(amg, f"elasticity_r{refine}", f"elasticity refine {refine} ({n} dofs), classical hierarchy "
                   f"(PMIS, ext+i, theta 0.5, 3 functions), MULT V(1,1) Jacobi w={a.elast_weight}, {L} levels",
                   register, n, rhs, widths, a, a.elast_weight)
    cl.free()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", type=int, nargs="*", default=[256])
    p.add_argument("--big", type=int, default=0, help="also this size (512) at K = 4 alone")
    p.add_argument("--refine", type=int, default=5, help="elasticity refinement (0: skip)")
    p.add_argument("--widths", type=int, nargs="+", default=[2, 4, 8])
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--smooth-weight", type=float, default=0.8)
    p.add_argument("--elast-weight", type=float, default=0.6)
    p.add_argument("--out", default=None, help="directory for <case>.json")
    a = p.parse_args()
    amg = load_package()
    cases = [lambda n=n: case_7pt(amg, n, a.widths, a) for n in a.sizes]
    if a.big:
        cases.append(lambda: case_7pt(amg, a.big, [4], a))
    if a.refine:
        cases.append(lambda: case_elasticity(amg, a.refine, a.widths, a))
    for case in cases:
        out = case()
        print(json.dumps(out), flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, out["case"] + ".json"), "w") as fh:
                json.dump(out, fh, indent=1)
                fh.write("\n")


if __name__ == "__main__":
    main()
