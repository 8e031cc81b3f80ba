"""bench.py's command line: a plain run is the headline only (every other leg
behind --full), --steps sets the timed steps, and --dump-outputs writes the last
step's iterate and residual norms reproducibly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FULL_ONLY = ("cpu_baseline", "cpu_baseline_seq", "parity", "fine_spmv", "fine_spmv_csr", "fine_spmv_csr_vi",
             "roofline_csr", "stream_triad_gbs", "vcycle_general_csr", "async_jacobi_overlap")


@pytest.fixture(scope="module")
def bench():
    import bench
    return bench


def test_plain_is_the_default(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert (a.full, a.dump_outputs) == (True, "d")


def test_dump_outputs_whole_and_sampled(bench, monkeypatch, tmp_path):
    monkeypatch.setattr(bench, "DUMP_MAX_ENTRIES", 1000)
    g = np.random.default_rng(3)
    small, big = g.standard_normal(1000), g.standard_normal(4097)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "big": big, "norms": np.array([2.0, 1.0])})
    s = np.load(tmp_path / "a" / "small.npy")
    b = np.load(tmp_path / "a" / "big.npy")
    assert s.dtype == np.float64 and np.array_equal(s, small)
    # the sample: 1000 entries of big at fixed sorted indices, the same in every run
    assert b.dtype == np.float64 and b.shape == (1000,)
    idx = np.sort(np.random.default_rng(0).integers(0, big.size, 1000))
    assert np.array_equal(b, big[idx])
    assert np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "norms.npy"), [2.0, 1.0])


def _run(args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0]), p.stderr


@pytest.mark.gpu
def test_plain_run_dumps_reproducible_outputs(tmp_path):
    n, steps = 32, 3
    outs = []
    for d in ("a", "b"):
        r, err = _run(["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--n", str(n),
                       "--dump-outputs", str(tmp_path / d)])
        assert r["steps"] == steps and r["warmup"] == 1 and r["full"] is False
        assert r["unit"] == "V-cycle iters/s" and r["higher_is_better"] is True and r["dtype"] == "f64"
        assert r["ms_per_step"] > 0 and abs(r["value"] * r["ms_per_step"] - 1e3) <= 1e-9 * 1e3
        assert not [k for k in FULL_ONLY if k in r], r.keys()
        assert "[cpu]" not in err and "[parity]" not in err and "triad" not in err
        assert sorted(os.listdir(tmp_path / d)) == ["resnorm.npy", "u.npy"]
        u, rn = np.load(tmp_path / d / "u.npy"), np.load(tmp_path / d / "resnorm.npy")
        assert u.dtype == np.float64 and u.shape == (n ** 3,) and rn.dtype == np.float64 and rn.shape == (2,)
        assert np.all(np.isfinite(u)) and np.any(u != 0.0)
        assert rn[1] / rn[0] == r["final_relres"] and rn[1] < rn[0]
        outs.append((u, rn))
    # same arguments, same inputs: the synchronous cycle is deterministic
    assert np.array_equal(outs[0][0].view(np.uint64), outs[1][0].view(np.uint64))
    assert np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.gpu
def test_dumped_iterate_is_the_solve_after_warmup_and_steps(amg, ctx, tmp_path):
    """the dump is what a caller of the timed path holds: the iterate of a solve
    of warmup + steps outer iterations through the library directly"""
    n, steps, warmup = 16, 2, 1
    r, _ = _run(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--n", str(n),
                 "--dump-outputs", str(tmp_path)])
    gen = amg.Gen(n, interp=amg.AMG_INTERP_LINEAR)
    L = gen.L
    As = [gen.register(ctx, amg.AMG_GEN_A, l) for l in range(L)]
    Ps = [gen.register(ctx, amg.AMG_GEN_P, l) for l in range(L - 1)]
    Rs = [gen.register(ctx, amg.AMG_GEN_R, l) for l in range(L - 1)]
    H = amg.Hier(ctx, As, Ps, Rs, amg.default_opts(smooth_weight=0.8, num_cycles=steps + warmup, tol=0.0))
    u, hist, k = H.solve(amg.rhs_rand(0, n ** 3))
    H.free()
    for M in As + Ps + Rs:
        M.free()
    gen.free()
    assert k == steps + warmup
    assert np.array_equal(np.load(tmp_path / "u.npy").view(np.uint64), u.view(np.uint64))
    rn = np.load(tmp_path / "resnorm.npy")
    # norms: the reduction order may differ between the two entry points
    assert abs(rn[0] - hist[0]) <= 1e-12 * hist[0] and abs(rn[1] - hist[-1]) <= 1e-12 * hist[-1]
