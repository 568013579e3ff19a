"""train.py --num-envs on CPU: the flag round-trips through settings.yaml,
and the default leaves the vectorized engine's module unimported."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--env", "SimpleCar", "-n", "3", "--steps", "6", "--batch-size", "6",
        "--cpu", "--eval-epi", "0", "--seed", "0"]

# runs train.py as __main__, then reports whether the module got imported
PROBE = (
    "import runpy, sys\n"
    "sys.argv = ['train.py'] + sys.argv[1:]\n"
    "runpy.run_path('train.py', run_name='__main__')\n"
    "print('VEC_IMPORTED', 'gcbf_amd.vec_rollout' in sys.modules)\n")


def _train(log_root, *extra):
    r = subprocess.run(
        [sys.executable, "-c", PROBE, *BASE, "--log-path", log_root, *extra],
        cwd=REPO, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    runs = os.path.join(log_root, "SimpleCar", "gcbf")
    (run_dir,) = os.listdir(runs)
    return r.stdout, os.path.join(runs, run_dir)


def test_num_envs_round_trips(tmp_path):
    from gcbf_amd.trainer.utils import read_settings
    out, run_dir = _train(str(tmp_path), "--num-envs", "3")
    assert read_settings(run_dir)["num_envs"] == 3
    assert "vectorized rollout engine active (3 scenes" in out
    assert "VEC_IMPORTED True" in out
    assert os.path.isdir(os.path.join(run_dir, "models", "step_6"))


def test_default_leaves_the_engine_unimported(tmp_path):
    from gcbf_amd.trainer.utils import read_settings
    out, run_dir = _train(str(tmp_path))
    assert read_settings(run_dir)["num_envs"] == 1
    assert "VEC_IMPORTED False" in out
    assert "vectorized" not in out


def test_batch_size_must_divide(tmp_path):
    r = subprocess.run(
        [sys.executable, "train.py", *BASE, "--log-path", str(tmp_path),
         "--num-envs", "4"],
        cwd=REPO, capture_output=True, text=True, timeout=900)
    assert r.returncode != 0
    assert "multiple of" in r.stderr
