"""bench.py --gpus N launches N ranks itself (no torchrun): gloo on CPU, world size 2."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["SHIFU_FORCE_CPU"] = "1"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       env=env, timeout=timeout, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_bench_gpus2_launches_two_ranks():
    out = _run(["--gpus", "2", "--rows", "4000", "--cols", "64", "--steps", "2", "--warmup", "1", "--full",
                "--gbdt-steps", "1", "--gbdt-warmup", "0", "--gbdt-rows", "500"])
    assert out["n_gpus"] == 2
    assert out["config"]["parallelism"] == "dp2"
    assert out["config"]["global_batch"] == 8000
    assert out["value"] > 0 and "gbdt_rounds_per_s" in out
    assert out["gbdt_config"]["parallelism"] == "dp2"
    assert out["rank_step_ms_max"] >= out["rank_step_ms_min"] > 0
    assert out["allreduce_ms_per_step"] >= 0


def test_bench_gpus1_single_process():
    out = _run(["--gpus", "1", "--rows", "2000", "--cols", "64", "--steps", "1", "--warmup", "0",
                "--gbdt-steps", "0"])
    assert out["n_gpus"] == 1 and out["config"]["parallelism"] == "dp1"


def test_bench_plain_run_is_mlp_only_and_dumps_reproducible_outputs(tmp_path):
    """A plain run times the MLP steps alone (the GBDT half needs --full); --dump-outputs writes what
    the timed steps computed, from the same seeded data and weights in every run.  The CPU path sums
    in fp32 over threads in no fixed order, so runs agree to fp32 summation error (2000 rows: well
    inside 1e-4 of the largest gradient entry), not bit for bit; RPROP steps by the gradient's sign,
    so the weights are only checked for shape."""
    import numpy as np
    dirs = [str(tmp_path / d) for d in ("a", "b")]
    for d in dirs:
        out = _run(["--gpus", "1", "--rows", "2000", "--cols", "64", "--steps", "3", "--warmup", "1",
                    "--dump-outputs", d])
        assert out["steps"] == 3 and out["ms_per_step"] > 0
        assert not [k for k in out if k.startswith("gbdt")]
    assert sorted(os.listdir(dirs[0])) == ["gradient.npy", "train_errors.npy", "weights.npy"]
    for f in os.listdir(dirs[0]):
        a, b = np.load(os.path.join(dirs[0], f)), np.load(os.path.join(dirs[1], f))
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all() and a.shape == b.shape
        if f != "weights.npy":
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-4 * np.abs(a).max())
    errs = np.load(os.path.join(dirs[0], "train_errors.npy"))
    assert errs.shape == (3,) and errs[-1] == out["final_train_error"]


def test_bench_launcher_fails_fast_when_a_rank_dies():
    """one rank exits at init -> the launcher stops the others and returns non-zero
    promptly (not after the 1800 s process-group timeout)."""
    import time
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(SHIFU_FORCE_CPU="1", SHIFU_BENCH_FAIL_RANK="1")
    t0 = time.monotonic()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--rows", "4000", "--cols", "64",
                        "--steps", "2", "--warmup", "1", "--gbdt-steps", "0"], capture_output=True, text=True,
                       env=env, timeout=120, cwd=ROOT)
    dt = time.monotonic() - t0
    assert p.returncode != 0, p.stdout
    assert dt < 30, dt
    assert "a rank failed" in p.stderr
