"""Episode-reset microbenchmark: host rejection loop vs device reset path.

    python tools/reset_bench.py [--resets 50] [--warmup 5] [--json OUT]

Median wall time of ``env.reset()`` (with a ``torch.cuda.synchronize()``
inside the timed region) for the host path (``device_reset=False``: the
Python rejection loop on the CPU, unchanged) and the device path
(``device_reset=True``: ops/hip/reset_sample.hip), same process, same
commit.  Scenes: DubinsCar n=16 obs=8, SimpleDrone n=16, and the stress
scene (DubinsCar n=256 obs=32 area 16).  Prints a markdown table.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from gcbf_amd.env import make_env
from gcbf_amd.trainer.utils import set_seed

SCENES = [
    ("DubinsCar n=16 obs=8", "DubinsCar", 16, {"num_obs": 8}),
    ("SimpleDrone n=16", "SimpleDrone", 16, {}),
    ("DubinsCar n=256 obs=32 area 16 (stress)", "DubinsCar", 256,
     {"num_obs": 32, "area_size": 16.0}),
]


def time_resets(env, resets, warmup):
    for _ in range(warmup):
        env.reset()
    if env.device.type == "cuda":
        torch.cuda.synchronize()
    times = []
    for _ in range(resets):
        t0 = time.perf_counter()
        env.reset()
        if env.device.type == "cuda":
            torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--resets", type=int, default=50)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--cpu", action="store_true", default=False)
    p.add_argument("--json", type=str, default=None,
                   help="also write the rows to this file")
    args = p.parse_args()
    assert args.resets >= 50, "use at least 50 resets per measurement"

    dev = torch.device(
        "cuda" if torch.cuda.is_available() and not args.cpu else "cpu")
    rows = []
    for label, name, n, overrides in SCENES:
        params = make_env(name, n, dev).default_params
        params.update(overrides)
        row = {"scene": label}
        for path, on in (("host", False), ("device", True)):
            set_seed(0)
            env = make_env(name, n, dev, params=params, device_reset=on)
            env.train()
            t = time_resets(env, args.resets, args.warmup)
            row[path + "_median_ms"] = statistics.median(t)
            row[path + "_min_ms"] = min(t)
            row[path + "_max_ms"] = max(t)
        row["speedup"] = row["host_median_ms"] / row["device_median_ms"]
        rows.append(row)

    print(f"env.reset() wall time on {dev}, median of {args.resets} resets "
          f"after {args.warmup} warm-up (min-max in brackets)")
    print("| scene | host path ms | device path ms | host/device |")
    print("|---|---|---|---|")
    for r in rows:
        print(f"| {r['scene']} "
              f"| {r['host_median_ms']:.2f} [{r['host_min_ms']:.2f}-"
              f"{r['host_max_ms']:.2f}] "
              f"| {r['device_median_ms']:.2f} [{r['device_min_ms']:.2f}-"
              f"{r['device_max_ms']:.2f}] "
              f"| {r['speedup']:.2f}x |")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
