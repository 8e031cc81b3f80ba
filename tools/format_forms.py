"""Which compressed forms a fixed list of operators takes, and how long their
registration takes.

    python tools/format_forms.py --list            one line of form getters per operator
    python tools/format_forms.py --time 1          wall-clock seconds of ctx.csr(...) per operator
    python tools/format_forms.py --time 1 --rungs  the same with the ladder cut off after each rung

The list: A, P and R of every level of the 64^3 box hierarchy with linear and with
aggregate interpolation (through ctx.csr and through the device-side generator),
the 27-pt operators of tests/test_gpu_march.py, the elasticity operator at
refinements 2 and 3 with both block forms, and the matrices of
tests/test_gpu_kernels.py with the default and the forced pair coding.
The timed ones: the 256^3 7-pt operator, its P and R, the 128^3 27-pt Galerkin
operator and the elasticity operator at refinement 5 (profiles/format_build).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from conftest import load_package  # noqa: E402

GETTERS = ("value_index", "dict_index", "row_pattern", "pair_pattern", "pair_anchor16", "master_pattern",
           "plane_march", "march_points", "bsr3")


def show(name, M):
    print(f"{name:24s} {M.nrows:9d} {M.ncols:9d} {M.nnz:10d} " + " ".join(f"{getattr(M, g):5d}" for g in GETTERS),
          flush=True)
    M.free()


def list_forms(amg, ctx):
    from oracle import pyoracle as po
    import test_gpu_kernels
    import test_gpu_march
    print(f"{'operator':24s} {'nrows':>9s} {'ncols':>9s} {'nnz':>10s} " + " ".join(g[:5].rjust(5) for g in GETTERS))
    ops = ((amg.AMG_GEN_A, "A"), (amg.AMG_GEN_P, "P"), (amg.AMG_GEN_R, "R"))
    for tag, interp in (("lin", amg.AMG_INTERP_LINEAR), ("agg", amg.AMG_INTERP_AGGREGATE)):
        g = amg.Gen(64, interp=interp)
        for which, w in ops:
            for lev in range(g.L if which == amg.AMG_GEN_A else g.L - 1):
                nr, nc, rp, cj, cv = g.host_csr(which, lev)
                show(f"{tag}64.{w}{lev}", ctx.csr(nr, nc, rp, cj, cv))
                show(f"{tag}64.{w}{lev}.gen", g.register(ctx, which, lev))
        g.free()
    # (the 32^3 Galerkin operator of that file is lin64.A1 above)
    for dims, per_pattern in (((32, 16, 5), True), ((64, 8, 4), False), ((256, 2, 3), True), ((16, 16, 4), True)):
        A = test_gpu_march.box_27pt(po, *dims, per_pattern=per_pattern)
        show("march27.{}{}x{}x{}".format("pat" if per_pattern else "uni", *dims),
             ctx.csr(A.nrows, A.ncols, A.rowptr, A.col, A.val))
    for r in (2, 3):
        n, rp, cj, v, _ = amg.classical.elasticity(r)
        for mode in (2, 1):
            ctx.set_bsr3(mode)
            show(f"elast.r{r}.bsr3={mode}", ctx.csr(n, n, rp, cj, v))
        ctx.set_value_index(0)
        show(f"elast.r{r}.plain", ctx.csr(n, n, rp, cj, v))
        ctx.set_value_index(1)
    host = test_gpu_kernels.matrices(po, amg)
    for pp in (1, 2):
        ctx.set_pair_pattern(pp)
        for name, A in host.items():
            show(f"kernels.{name}.pp={pp}", ctx.csr(A.nrows, A.ncols, A.rowptr, A.col, A.val))
    ctx.set_pair_pattern(1)


# the ladder cut off after each rung: the setter that turns the next rung off
RUNGS = (("plain", "set_value_index"), ("value", "set_dict_index"), ("dict", "set_row_pattern"),
         ("row", "set_pair_pattern"), ("pair", "set_master_pattern"), ("all", None))


def time_registration(amg, ctx, runs, rungs=False):
    g = amg.Gen(256, interp=amg.AMG_INTERP_LINEAR)
    host = {"A0_7pt_256": g.host_csr(amg.AMG_GEN_A, 0), "P0_256": g.host_csr(amg.AMG_GEN_P, 0),
            "R0_256": g.host_csr(amg.AMG_GEN_R, 0), "A1_27pt_128": g.host_csr(amg.AMG_GEN_A, 1)}
    n, rp, cj, v, _ = amg.classical.elasticity(5)
    host["elast_r5"] = (n, n, rp, cj, v)
    ctx.csr(*g.host_csr(amg.AMG_GEN_A, 3)).free()  # the first launch of every setup kernel
    out = {}
    for name, op in host.items():
        for rung, off in RUNGS if rungs else RUNGS[-1:]:
            key = f"{name}.{rung}" if rungs else name
            out[key] = []
            if off:
                getattr(ctx, off)(0)
            for _ in range(runs):
                ctx.sync()
                t0 = time.perf_counter()
                M = ctx.csr(*op)  # registration synchronises the stream
                out[key].append(round(time.perf_counter() - t0, 5))
                M.free()
            if off:
                getattr(ctx, off)(1)
    print(json.dumps(out))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--list", action="store_true")
    p.add_argument("--time", type=int, default=0, metavar="RUNS")
    p.add_argument("--rungs", action="store_true")
    a = p.parse_args()
    amg = load_package()
    ctx = amg.Context(device=0, nstreams=1)
    if a.list:
        list_forms(amg, ctx)
    if a.time:
        time_registration(amg, ctx, a.time, a.rungs)
    ctx.close()


if __name__ == "__main__":
    main()
