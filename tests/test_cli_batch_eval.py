"""test.py --batch-epi against the sequential evaluation loop (CPU)."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--env", "SimpleCar", "-n", "4", "--epi", "3", "--cpu"]


def _run(cwd, *extra):
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run(
        [sys.executable, os.path.join(REPO, "test.py"), *BASE, *extra],
        cwd=cwd, env=env, capture_output=True, text=True, timeout=600)


def test_batch_epi_appends_the_same_log_row(tmp_path):
    """Nominal controller (no checkpoint directory): the two paths evaluate
    the same three layouts and append the same test_log.csv row."""
    for extra in (("--no-video",), ("--no-video", "--batch-epi", "3")):
        res = _run(tmp_path, *extra)
        assert res.returncode == 0, res.stderr[-2000:]
        assert "average reward" in res.stdout
    log = tmp_path / "logs" / "SimpleCar" / "test_log.csv"
    rows = log.read_text().splitlines()
    assert len(rows) == 2
    assert rows[0] == rows[1]
    assert rows[0].startswith("4,None,3,None,")


def test_batch_epi_requires_no_video(tmp_path):
    res = _run(tmp_path, "--batch-epi", "3")
    assert res.returncode == 2                     # argparse error
    assert "--no-video" in res.stderr
    assert not (tmp_path / "logs").exists()
