"""train.py --algo macbf --num-envs B --capture-capped on CPU: the
vectorized engine collects MACBF's neighbour-capped rollouts; without
--capture-capped the run falls back with the reason printed."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--algo", "macbf", "--env", "SimpleCar", "-n", "3", "--steps", "6",
        "--batch-size", "6", "--cpu", "--eval-epi", "0", "--seed", "0",
        "--num-envs", "2"]


def _train(log_root, *extra):
    r = subprocess.run(
        [sys.executable, "train.py", *BASE, "--log-path", log_root, *extra],
        cwd=REPO, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    runs = os.path.join(log_root, "SimpleCar", "macbf")
    (run_dir,) = os.listdir(runs)
    return r.stdout, os.path.join(runs, run_dir)


def test_macbf_num_envs_capture_capped(tmp_path):
    out, run_dir = _train(str(tmp_path), "--capture-capped")
    assert "vectorized rollout engine active (2 scenes" in out
    assert "vectorized rollout unavailable" not in out
    assert os.path.isdir(os.path.join(run_dir, "models", "step_6"))


def test_macbf_num_envs_alone_falls_back(tmp_path):
    out, run_dir = _train(str(tmp_path))
    assert "vectorized rollout unavailable" in out and "MACBF" in out
    assert "vectorized rollout engine active" not in out
    assert os.path.isdir(os.path.join(run_dir, "models", "step_6"))
