"""AMG-preconditioned CG on the distributed hierarchy (amg_dist_pcg_*) beside the
stationary V-cycle iteration of the same hierarchy: what the two all-gathers per
PCG iteration cost, and what the Krylov acceleration buys.

Per rank count it prints one JSON line: PCG iterations/s and stationary
V-cycles/s (each `--iters` iterations enqueued in one call, timed to the read
of the last norm; the best of `--runs`), and the iterations each needs until
||r|| / ||r0|| < `--tol`.

Ranks are threads of this process on one GPU: one rank over RCCL, several over
the host transport, whose collectives synchronise the stream (so their rates
measure that transport, not the device).  Usage:
    python tools/bench_dist_pcg.py [--n 128] [--ranks 1,2,4] [--iters 20] [--form slab|rows]

Process mode (one process per rank, the production layout): run it under
torchrun, e.g. `python -m torch.distributed.run --nproc-per-node 8 --master-addr
127.0.0.1 tools/bench_dist_pcg.py`; every process drives cuda:LOCAL_RANK (modulo
the visible devices) over RCCL (`--transport rccl`, one rank per GPU) or gloo
(`--transport host`).  Rank 0 prints the JSON line of that one rank count.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def options(amg, a):
    return amg.default_opts(smooth_weight=0.8, num_cycles=a.cap, tol=a.tol, check_resnorm=1)


def measure(D, f, a, barrier):
    """this rank's figures on its hierarchy D (every rank makes the same calls)"""
    fl = f[D.row0:D.row0 + D.n0]

    def timed(start, iterate, resnorm):
        best = None
        for _ in range(a.runs + 1):  # the first run allocates
            start(fl)
            barrier()
            t = time.perf_counter()
            iterate(a.iters)
            rn = resnorm()  # host sync
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
        return a.iters / best, rn

    pcg_rate, _ = timed(D.pcg_start, D.pcg_iterate, D.pcg_resnorm)
    cyc_rate, _ = timed(D.solve_start, D.iterate, D.resnorm)
    _, hist, k_pcg = D.pcg_solve(fl)
    r0 = D.solve_start(fl)
    k_cyc, rel = 0, 1.0
    while k_cyc < a.cap and rel >= a.tol:
        D.iterate(1)
        k_cyc += 1
        rel = D.resnorm() / r0
    return {"pcg_iterations_per_s": pcg_rate, "vcycles_per_s": cyc_rate,
            "pcg_iterations_to_tol": k_pcg, "pcg_relres": float(hist[-1] / hist[0]),
            "vcycles_to_tol": k_cyc, "vcycle_relres": float(rel),
            "reached_tol": [bool(hist[-1] / hist[0] < a.tol), bool(rel < a.tol)]}


def line(a, gen, R, transport, fig, processes=None):
    out = {"metric": "PCG iterations/s beside stationary V-cycles/s on one distributed hierarchy",
           "ranks": R, "transport": transport, "form": a.form,
           "data": "synthetic (7-pt Laplacian, RandDouble(-1,1) RHS after srand(0))",
           "config": {"workload": f"{a.n}^3 7-pt Laplacian, MULT V(1,1) Jacobi w=0.8, {gen.L} levels",
                      "iters_timed": a.iters, "tol": a.tol, "cap": a.cap, "replicate_rows": a.rep}}
    if processes:
        out["processes"] = processes
    out.update(fig)
    return json.dumps(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", "--size", dest="n", type=int, default=128)
    ap.add_argument("--ranks", default="1,2,4", help="thread mode: rank counts, comma separated")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--tol", type=float, default=1e-9)
    ap.add_argument("--cap", type=int, default=200, help="most iterations of a run to tol")
    ap.add_argument("--rep", type=int, default=1 << 12)
    ap.add_argument("--form", choices=("slab", "rows"), default="slab")
    ap.add_argument("--transport", choices=("rccl", "host"), default="rccl",
                    help="process mode: transport between the ranks")
    a = ap.parse_args()
    if "WORLD_SIZE" in os.environ:
        return main_procs(a)
    from conftest import load_package
    from test_gpu_dist import run_ranks
    amg = load_package()
    gen = amg.Gen(a.n)
    f = amg.rhs_rand(0, a.n ** 3)
    opts = options(amg, a)
    for R in [int(x) for x in a.ranks.split(",")]:
        hub = amg.dist.ThreadMailbox(R, timeout=1200.0)

        def rank(r):
            c = amg.Context(0, nstreams=2)
            if R == 1:
                amg.dist.init_rccl(c, 1, 0, lambda b: b)
            else:
                amg.dist.init_host(c, R, r, amg.dist.HostTransport(hub, r))
            amg.dist.set_replicate_rows(c, a.rep)
            D = amg.dist.DistHier(c, gen, opts, slab=a.form == "slab")
            fig = measure(D, f, a, lambda: amg.dist.barrier(c))
            D.free()
            amg.dist.finalize(c)
            c.close()
            return fig

        res = run_ranks(R, rank)
        fig = dict(res[0])
        for key in ("pcg_iterations_per_s", "vcycles_per_s"):  # the slowest rank's
            fig[key] = min(t[key] for t in res)
        print(line(a, gen, R, "rccl" if R == 1 else "host (thread ranks on one GPU)", fig), flush=True)
    gen.free()


def main_procs(a):
    """one process per rank (torchrun)"""
    import torch
    import torch.distributed as tdist
    from conftest import load_package
    world = int(os.environ["WORLD_SIZE"])
    rank = int(os.environ["RANK"])
    local = int(os.environ.get("LOCAL_RANK", rank))
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)  # stdout carries only the JSON line
    tdist.init_process_group("gloo", rank=rank, world_size=world)
    amg = load_package()
    dev = local % max(1, torch.cuda.device_count())
    gen = amg.Gen(a.n)
    f = amg.rhs_rand(0, a.n ** 3)
    c = amg.Context(dev, nstreams=2)
    tr = None
    if a.transport == "rccl":
        def bcast(obj):
            lst = [obj]
            tdist.broadcast_object_list(lst, src=0)
            return lst[0]
        amg.dist.init_rccl(c, world, rank, bcast)
    else:
        tr = amg.dist.HostTransport(amg.dist.TorchGroupHub(), rank)
        amg.dist.init_host(c, world, rank, tr)
    amg.dist.set_replicate_rows(c, a.rep)
    D = amg.dist.DistHier(c, gen, options(amg, a), slab=a.form == "slab")
    fig = measure(D, f, a, tdist.barrier)
    rates = torch.tensor([fig["pcg_iterations_per_s"], fig["vcycles_per_s"]], dtype=torch.float64)
    tdist.all_reduce(rates, op=tdist.ReduceOp.MIN)  # the slowest rank's
    fig["pcg_iterations_per_s"], fig["vcycles_per_s"] = float(rates[0]), float(rates[1])
    D.free()
    amg.dist.finalize(c)
    c.close()
    if tr is not None and tr.error is not None:
        raise tr.error
    if rank == 0:
        os.write(json_fd, (line(a, gen, world, a.transport, fig, processes=world) + "\n").encode())
    gen.free()
    tdist.destroy_process_group()


if __name__ == "__main__":
    main()
