"""The turn order of the deterministic asynchronous schedules (AmgAsyncTurns,
through amg_async_turns_probe: the generator amg_async_solve and
amg_dist_async_solve issue from) against the oracle's or_set_async_schedule,
on the CPU."""
import ctypes as C

import numpy as np
import pytest

N = 7  # num_cycles
W = 0.8


def turns(amg, sched, k_lo, k_hi, G, conv_global, dur=None, times=None):
    """(sequence, last flags, per-group counts) of the probe"""
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    cap = 64 * G * (N + 2)
    seq, last = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
    cnt, count = np.zeros(G, dtype=np.int32), C.c_int()
    d = t = tn = None
    if dur is not None:
        d = np.ascontiguousarray(dur, dtype=np.float64)
    if times is not None:
        tn = np.array([len(x) for x in times], dtype=np.int32)
        t = np.ascontiguousarray(np.concatenate(list(times) + [np.zeros(1)]), dtype=np.float64)
    ptr = lambda a, ty: a.ctypes.data_as(ty) if a is not None else None
    amg.check(amg.lib.amg_async_turns_probe(sched, k_lo, k_hi, G, N, int(conv_global), ptr(d, dp), ptr(t, dp),
                                            ptr(tn, ip), ptr(seq, ip), ptr(last, ip), cap, C.byref(count),
                                            ptr(cnt, ip)))
    assert count.value <= cap
    return list(seq[:count.value]), list(last[:count.value]), list(cnt)


def timed_end(dur, times, k, j):
    """the oracle's timed_end: correction j (0-based) of group k"""
    if times is None or len(times[k]) == 0:
        return (j + 1) * (dur[k] if dur is not None else 1.0)
    t, n = times[k], len(times[k])
    if j < n:
        return t[j]
    dt = t[n - 1] - t[n - 2] if n > 1 else t[0]
    return t[n - 1] + (j - n + 1) * dt


@pytest.fixture(scope="module", params=[8, 16])
def oracle_hier(request, amg, oracle):
    from test_gpu_solve import hierarchy
    n = request.param
    _, L, host = hierarchy(amg, oracle, n, amg.AMG_INTERP_LINEAR)
    assert L == {8: 3, 16: 4}[n]
    Ps, Rs = [], []
    for lev in range(L - 1):
        ps, rs = oracle.smooth_transfer(host["A"][lev], host["P"][lev], W)
        Ps.append(ps)
        Rs.append(rs)
    o = oracle.make_opts(solver=oracle.OR_ASYNC_MULTADD, smooth_weight=W, num_cycles=N, tol=0.0)
    return oracle.Hier(host["A"], Ps, Rs, o), L, amg.rhs_rand(0, n ** 3)


def oracle_counts(oracle, OH, f, L, res_global, sched, conv_global, dur=None, times=None):
    if times is not None:
        oracle.set_async_times(times)
    else:
        oracle.set_async_durations(dur if dur is not None else np.ones(L))
    oracle.lib().or_set_async_schedule(sched)
    try:
        nt = [0] + [1] * (L - 1) if res_global else [1] * L
        _, _, cnt = OH.async_add(f, nt, async_type=oracle.OR_FULL_ASYNC, res_global=res_global,
                                 converge_type=oracle.OR_CONVERGE_GLOBAL if conv_global else
                                 oracle.OR_CONVERGE_LOCAL)
    finally:
        oracle.lib().or_set_async_schedule(0)
        oracle.set_async_durations(np.ones(L))
    return list(cnt[:L])


@pytest.mark.parametrize("res_global", [False, True], ids=["res_local", "res_global"])
def test_turn_order_matches_oracle(amg, oracle, oracle_hier, res_global):
    """Every schedule, converge test and TIMED speed table: the per-group
    counts equal the oracle's, and the sequence obeys the schedules' rules."""
    OH, L, f = oracle_hier
    # LOCAL residuals: levels [0, L - 1) correct, the coarsest group idles;
    # GLOBAL residuals: groups [1, L), no idle group
    k_lo, k_hi = (1, L) if res_global else (0, L - 1)
    d = np.array([3.0 / 1.9 ** k + 0.05 for k in range(L)])
    timed = [dict(dur=d), dict(dur=d[::-1].copy()), dict(dur=np.ones(L)),
             dict(times=[d[k] * np.arange(1, 4) for k in range(L)])]  # 3 < N: the last interval repeats
    cases = [(s, False, {}) for s in (1, 2, 3)] + [(4, False, t) for t in timed]
    cases += [(3, True, {})] + [(4, True, t) for t in timed]
    for sched, cg, kw in cases:
        seq, last, cnt = turns(amg, sched, k_lo, k_hi, L, cg, **kw)
        tag = (sched, cg, sorted(kw), seq)
        assert cnt[k_lo:k_hi] == oracle_counts(oracle, OH, f, L, res_global, sched, cg, **kw)[k_lo:k_hi], tag
        assert all(k_lo <= k < k_hi for k in seq), tag
        assert [seq.count(k) for k in range(k_lo, k_hi)] == cnt[k_lo:k_hi], tag
        # the last flag: on each group's final correction and no other
        final = {k: max(i for i, q in enumerate(seq) if q == k) for k in range(k_lo, k_hi)}
        assert [i for i, l in enumerate(last) if l] == sorted(final.values()), tag
        if not cg:
            assert cnt[k_lo:k_hi] == [N] * (k_hi - k_lo), tag
        groups = list(range(k_lo, k_hi))
        if sched in (1, 2):  # level after level
            assert seq == [k for k in (groups if sched == 1 else groups[::-1]) for _ in range(N)], tag
        if sched == 3 and not cg:  # cycle-major
            assert seq == groups * N, tag
        if sched == 3 and cg:  # the flag rises in round N + 1, seen by every group in that round
            assert seq == groups * (N + 1), tag
        if sched == 4:
            if "dur" in kw and np.all(kw["dur"] == 1.0):
                assert (seq, last) == turns(amg, 3, k_lo, k_hi, L, cg)[:2], tag
            # whole corrections in the order of their end times, ties to the finer group
            done, ends = {k: 0 for k in groups}, []
            for k in seq:
                ends.append((timed_end(kw.get("dur"), kw.get("times"), k, done[k]), k))
                done[k] += 1
            assert all(a < b for a, b in zip(ends, ends[1:])), tag


def test_turn_order_known_counts(amg):
    """TIMED under converge GLOBAL, LOCAL residuals (the idle coarsest group's
    count is part of the flag): the counts of the 3- and 4-level hierarchies."""
    for L, want in ((3, [7, 14, 25]), (4, [0, 7, 13, 24])):
        d = np.array([3.0 / 1.9 ** k + 0.05 for k in range(L)])
        k_lo, k_hi = (0, L - 1) if L == 3 else (1, L)
        _, _, cnt = turns(amg, 4, k_lo, k_hi, L, True, dur=d)
        assert cnt == want, cnt
