"""bench.py --gpus N starts its own N ranks when no torch.distributed
environment is set (the driver's plain `python bench.py --gpus N`), as the
reference trainer spawns its world itself (train.py:228-234, per-rank batch
train.py:82). Runs the launcher on CPU/gloo (`--device cpu`: the cpu_baseline
step, a plumbing test, never a measurement) with N=2 and checks the one JSON
line rank 0 prints."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=600):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args], cwd=REPO, env=env,
                          capture_output=True, text=True, timeout=timeout)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("config", ["kitti", "sintel_mf"])
def test_bench_spawns_two_ranks_on_gloo(config):
    hw = ["64", "128"] if config == "kitti" else ["128", "256"]  # sintel_mf: its capture size (test_ddp_cpu)
    p = _run(["--device", "cpu", "--gpus", "2", "--steps", "1", "--warmup", "0", "--batch", "1",
              "--hw", *hw, "--config", config])
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout  # rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2
    assert out["config"]["parallelism"] == "dp2"
    assert out["config"]["global_batch"] == 2 and out["config"]["per_gpu_batch"] == 1
    assert out["scaling"] == "weak"
    assert out["value"] > 0 and out["device"].startswith("cpu")
    assert ("Sintel" in out["metric"]) == (config == "sintel_mf")
    assert out["final_loss"] == out["final_loss"]  # finite (not NaN)


@pytest.mark.timeout(600)
def test_bench_dump_outputs_is_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's loss / params / grads as
    float32 .npy; two runs with the same arguments start from the same frames
    and weights, so they write the same arrays. --steps sets the timed steps,
    and a plain run reports none of the --full measurements."""
    import numpy as np

    outs = []
    for d in ("a", "b"):
        p = _run(["--device", "cpu", "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "1",
                  "--hw", "64", "128", "--dump-outputs", str(tmp_path / d)])
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, p.stdout
        outs.append(json.loads(lines[0]))
    out = outs[0]
    assert out["steps"] == 2 and out["warmup"] == 1 and out["full"] is False
    assert out["ms_per_step"] > 0
    assert abs(out["value"] * out["ms_per_step"] / 1e3 - 1.0) < 1e-2  # batch 1: pairs/s x s/step == 1
    for k in ("phases", "levels", "roofline", "cpu_baseline", "survey_configs", "hot_path_us_per_step"):
        assert out[k] is None, k
    assert sorted(f.name for f in (tmp_path / "a").iterdir()) == ["grads.npy", "loss.npy", "params.npy"]
    total = 0
    for name in ("loss", "params", "grads"):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == b.shape and np.isfinite(a).all(), name
        assert np.abs(a).max() > 0, name
        # same inputs, same host code: equal up to the thread-order rounding of fp32 sums
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-6, err_msg=name)
        total += a.nbytes
    assert total <= 64 * 1000 * 1000
    assert np.load(tmp_path / "a" / "params.npy").shape == np.load(tmp_path / "a" / "grads.npy").shape
    assert abs(float(np.load(tmp_path / "a" / "loss.npy")[0]) - out["final_loss"]) <= 1e-5


@pytest.mark.timeout(300)
def test_bench_rejects_mismatched_world():
    """Under an external launcher, --gpus must equal WORLD_SIZE (no silent one-rank run)."""
    p = _run(["--device", "cpu", "--gpus", "2", "--steps", "1", "--warmup", "0", "--batch", "1",
              "--hw", "64", "128"], env_extra={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode == 2
    assert "WORLD_SIZE" in p.stderr
