"""Host model of the AMG-preconditioned CG (amg_pcg_*): the device's dot
product restated in numpy and the recurrence with the oracle's cycles as M^-1.

Test infrastructure only.  dev_dot follows partials_k / sum_partials_k /
block_sum_256 of csrc/amg_kernels.hip operation by operation, so its result has
the bits of amg_vec_dot; pcg_model with dot = dev_dot has the bits of the
device recurrence (every statement one rounded fp64 operation).
"""
import math

import numpy as np


# ---- the device reduction -----------------------------------------------------
def _tree64(w):
    """lane 0 of the shfl_down tree over offsets 32 .. 1 of 64 lanes (last axis)"""
    for off in (32, 16, 8, 4, 2, 1):
        w = w[..., :off] + w[..., off:2 * off]
    return w[..., 0]


def _block_sum_256(lanes):
    """block_sum_256: the tree per wave of 64 lanes, then ((w0 + w1) + w2) + w3"""
    w = _tree64(lanes.reshape(lanes.shape[:-1] + (4, 64)))
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def _lane_strided(v, nb):
    """lane t of block b: s = 0.0; s += v[i] for i = 256 b + t, += 256 nb; then the block sums"""
    stride = nb * 256
    k = -(-v.size // stride)
    pad = np.zeros(k * stride)
    pad[:v.size] = v  # a lane past the end adds nothing; + 0.0 leaves a sum that began at +0.0 unchanged
    pad = pad.reshape(k, nb, 256)
    s = np.zeros((nb, 256))
    for j in range(k):
        s = s + pad[j]
    return _block_sum_256(s)


def dev_dot(x, y):
    """x . y with the bits of amg_vec_dot (dot_partials + reduce_partials)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    n = x.size
    nb = max(1, min(1024, -(-n // 2048)))
    partials = _lane_strided(x * y, nb)
    return float(_lane_strided(partials, 1)[0])


# ---- hierarchies ----------------------------------------------------------------
def host_hierarchy(amg, oracle, n, interp=None, levels=None):
    """(L, {"A": [...], "P": [...], "R": [...]}) of the structured generator's hierarchy as oracle.Csr;
    n: the cube's edge, or (nx, ny, nz)"""
    g = amg.Gen(*(n if isinstance(n, tuple) else (n,)), interp=amg.AMG_INTERP_LINEAR if interp is None else interp,
                **({} if levels is None else {"max_levels": levels}))
    L = g.L
    host = {}
    for which, tag, cnt in ((amg.AMG_GEN_A, "A", L), (amg.AMG_GEN_P, "P", L - 1), (amg.AMG_GEN_R, "R", L - 1)):
        host[tag] = [oracle.Csr(*g.host_csr(which, l)) for l in range(cnt)]
    g.free()
    return L, host


def tridiag_hierarchy(oracle, n):
    """one level, A = tridiag(-1, 4, -1), the diagonal first in every row"""
    rp, col, val = [0], [], []
    for i in range(n):
        col.append(i)
        val.append(4.0)
        for j in (i - 1, i + 1):
            if 0 <= j < n:
                col.append(j)
                val.append(-1.0)
        rp.append(len(col))
    A = oracle.Csr(n, n, np.array(rp), np.array(col, dtype=np.int32), np.array(val))
    return 1, {"A": [A], "P": [], "R": []}


def device_hier(amg, ctx, host, opts):
    dev = {k: [ctx.csr(M.nrows, M.ncols, M.rowptr, M.col, M.val) for M in v] for k, v in host.items()}
    return amg.Hier(ctx, dev["A"], dev["P"], dev["R"], opts)


def oracle_hier(oracle, host, opts, num_cycles=None):
    """the oracle's hierarchy under the device options (composed transfers as smooth_transfer says)"""
    oo = oracle.make_opts(solver=opts.solver, smoother=opts.smoother, num_pre=opts.num_pre_smooth_sweeps,
                          num_post=opts.num_post_smooth_sweeps, num_fine=opts.num_fine_smooth_sweeps,
                          num_coarse=opts.num_coarse_smooth_sweeps, smooth_weight=opts.smooth_weight,
                          num_cycles=opts.num_cycles if num_cycles is None else num_cycles, tol=0.0,
                          check_resnorm=1, num_threads=max(opts.num_threads, 1))
    OH = oracle.Hier(host["A"], host["P"], host["R"], oo)
    if opts.smooth_transfer == 1 and opts.solver == oracle.OR_MULTADD:
        OH.set_composed_transfers()
    return OH


def oracle_precond(oracle, host, opts):
    """r -> M^-1 r: one cycle of the oracle's solver from a zero state.  MULT: DMEM_Mult's
    single cycle 0 + 1.0 e (the bits of the oracle's precond_apply); BPX / MULTADD / AFACX:
    one cycle of the stationary solve from u = 0, whose residual f - A 0 is f"""
    OH = oracle_hier(oracle, host, opts, num_cycles=1)
    if opts.solver == oracle.OR_MULT:
        return lambda r: OH.dmem_mult_solve(r, accel=0)[0]
    return lambda r: OH.solve(r)[0]


# ---- the recurrence -------------------------------------------------------------
class PcgRun:
    def __init__(self):
        self.xs, self.rs, self.alpha, self.beta, self.rho, self.hist = [], [], [], [], [], []


def pcg_model(oracle, host, opts, f, iters, dot, x0=None):
    """the recurrence of amg_pcg_solve on the host; xs[k], rs[k], hist[k] after k iterations
    (k = 0: the start), alpha / beta / rho[k - 1] of iteration k"""
    A = host["A"][0]
    M = oracle_precond(oracle, host, opts)
    f = np.ascontiguousarray(f, dtype=np.float64)
    x = np.zeros(A.nrows) if x0 is None else np.array(x0, dtype=np.float64)
    run = PcgRun()
    r = oracle.smem_spgemv(A, x, f, -1.0, 1.0, np.zeros(A.nrows))  # the outer residual form
    z = M(r)
    p = z.copy()
    rho = dot(r, z)
    run.xs.append(x.copy())
    run.rs.append(r.copy())
    run.hist.append(math.sqrt(dot(r, r)))
    for _ in range(iters):
        q = oracle.seq_matvec(A, p)
        pq = dot(p, q)
        alpha = rho / pq if pq != 0.0 else 0.0
        x = x + alpha * p
        r = r - alpha * q
        run.hist.append(math.sqrt(dot(r, r)))
        z = M(r)
        rho_new = dot(r, z)
        beta = rho_new / rho if rho != 0.0 else 0.0
        rho = rho_new
        p = z + beta * p
        run.xs.append(x.copy())
        run.rs.append(r.copy())
        run.alpha.append(alpha)
        run.beta.append(beta)
        run.rho.append(rho)
    run.hist = np.array(run.hist)
    return run
