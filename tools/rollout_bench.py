"""Rollout-only microbenchmark: captured engine step cost, split by path.

    python tools/rollout_bench.py [--env DubinsCar] [-n 16] [--obs 0]
                                  [--algo {gcbf,macbf}] [--max-neighbors K]
                                  [--tail {0,1}] [--glue {0,1}]
                                  [--compare-eager [--rounds 3]]

Times engine.step for forced-policy, forced-explore and mixed (prob 0.5)
streams, without updates — isolates rollout regressions from update noise
in the full bench.

``--compare-eager`` instead alternates, in one process and on the same
weights, the eager loop (``algo.step`` + ``env.step``, what the trainer runs
without an engine) and captured engines with the tail and the actor glue on
and off, ``--rounds`` times each, and reports min..max env-steps/s of the
rollout alone at prob 0.5:

    python tools/rollout_bench.py --algo macbf --env SimpleCar \\
        --max-neighbors 12 --compare-eager
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from gcbf_amd.algo import make_algo
from gcbf_amd.env import make_env
from gcbf_amd.rollout import RolloutEngine
from gcbf_amd.trainer.utils import set_seed
from gcbf_amd.utils.amp import enable_bf16


def run_steps(eng, prob, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        if eng.step(prob=prob):
            eng.reload()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


class EagerLoop:
    """The trainer's loop without an engine, resumable between rounds."""

    def __init__(self, env, algo):
        self.env, self.algo = env, algo
        self.data = env.reset()

    def run(self, prob, n):
        env, algo, data = self.env, self.algo, self.data
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            if data.u_ref is None:
                data.update(u_ref=env.u_ref(data))
            action = algo.step(data, prob=prob)
            next_data, reward, done, info = env.step(action)
            next_data.update(u_ref=env.u_ref(next_data))
            algo.post_step(data, action, reward, done, next_data)
            data = env.reset() if done else next_data
        torch.cuda.synchronize()
        self.data = data
        return (time.perf_counter() - t0) / n * 1e3


def make_scene(args, dev):
    e0 = make_env(args.env, args.num_agents, dev)
    params = e0.default_params
    params["num_obs"] = args.obs
    env = make_env(args.env, args.num_agents, dev, params=params,
                   max_neighbors=args.max_neighbors)
    env.train()
    return env


def make_engine(args, dev, algo, tail, glue):
    """An engine on a scene of its own; the two switches are read when the
    engine is built, so one process holds engines of every kind."""
    for name, val in (("GCBF_AMD_ROLLOUT_TAIL", tail),
                      ("GCBF_AMD_ACTOR_GLUE", glue)):
        if val is not None:
            os.environ[name] = str(val)
    env = make_scene(args, dev)
    env.reset()
    return RolloutEngine(env, algo)


def compare_eager(args, dev, algo):
    runners = {"eager": EagerLoop(make_scene(args, dev), algo).run}
    for tail in (1, 0):
        for glue in (1, 0):
            eng = make_engine(args, dev, algo, tail, glue)
            name = f"engine tail={int(eng._tail)} glue={int(eng._glue)}"
            runners[name] = (lambda prob, n, e=eng: run_steps(e, prob, n))
    for run in runners.values():              # warmup
        run(0.5, 100)
        algo.buffer.clear()
    rates = {k: [] for k in runners}
    for _ in range(args.rounds):
        for name, run in runners.items():
            rates[name].append(1e3 / run(0.5, args.steps))
            algo.buffer.clear()               # rollout only: no replay growth
    head = (f"[{args.algo} {args.env} n={args.num_agents} obs={args.obs} "
            f"max_neighbors={args.max_neighbors} prob=0.5 "
            f"{args.rounds} rounds x {args.steps} steps]")
    print(f"rollout env-steps/s, min..max {head}")
    for name, r in rates.items():
        print(f"  {name:28s} {min(r):9.1f} .. {max(r):9.1f}")
    print(json.dumps({"rollout_env_steps_per_s": {
        k: [round(v, 1) for v in r] for k, r in rates.items()}}))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--env", type=str, default="DubinsCar")
    p.add_argument("-n", "--num-agents", type=int, default=16)
    p.add_argument("--obs", type=int, default=0)
    p.add_argument("--steps", type=int, default=1500)
    p.add_argument("--algo", type=str, choices=("gcbf", "macbf"),
                   default="gcbf")
    p.add_argument("--max-neighbors", type=int, default=None,
                   help="neighbour cap of the scene's graphs (training "
                        "MACBF uses 12); default: none")
    p.add_argument("--tail", type=int, choices=(0, 1), default=None,
                   help="force GCBF_AMD_ROLLOUT_TAIL (one-launch step tail) "
                        "off/on for A/B runs; default: leave the env var")
    p.add_argument("--glue", type=int, choices=(0, 1), default=None,
                   help="force GCBF_AMD_ACTOR_GLUE (padded-bf16 actor chain) "
                        "off/on; default: leave the env var")
    p.add_argument("--compare-eager", action="store_true", default=False,
                   help="alternate the eager loop and captured engines "
                        "(tail and glue on and off) on the same weights")
    p.add_argument("--rounds", type=int, default=3,
                   help="rounds per loop kind under --compare-eager (>= 3)")
    args = p.parse_args()
    if args.compare_eager and args.rounds < 3:
        p.error("--rounds must be at least 3")

    set_seed(0)
    dev = torch.device("cuda")
    env = make_scene(args, dev)
    algo = make_algo(args.algo, env, args.num_agents, env.node_dim,
                     env.edge_dim, env.action_dim, dev, batch_size=512)
    enable_bf16(algo)
    if args.compare_eager:
        compare_eager(args, dev, algo)
        return
    for name, val in (("GCBF_AMD_ROLLOUT_TAIL", args.tail),
                      ("GCBF_AMD_ACTOR_GLUE", args.glue)):
        if val is not None:
            os.environ[name] = str(val)
    env.reset()
    eng = RolloutEngine(env, algo)
    for _ in range(300):                      # warmup
        if eng.step(prob=0.5):
            eng.reload()
    t_pol = run_steps(eng, 0.0, args.steps)   # always policy graph
    t_exp = run_steps(eng, 1.0, args.steps)   # always explore graph
    t_mix = run_steps(eng, 0.5, args.steps)
    extra = "" if args.algo == "gcbf" and args.max_neighbors is None else (
        f" algo={args.algo} max_neighbors={args.max_neighbors} "
        f"glue={int(eng._glue)}")
    print(f"rollout ms/step: policy {t_pol:.4f}  explore {t_exp:.4f}  "
          f"mixed(0.5) {t_mix:.4f}   [{args.env} n={args.num_agents} "
          f"obs={args.obs} tail={int(eng._tail)}{extra}]")


if __name__ == "__main__":
    main()
