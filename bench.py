"""Flagship benchmark: steady-state GCBF training throughput on DubinsCar n=16.

Measures the BASELINE.json headline metric — env-steps/sec (whole node) on
the paper config (DubinsCar, 16 agents, GCBF, batch_size 512) with synthetic
random-init agents/goals (the environment itself is the synthetic data
source; there are no datasets).

Steady-state semantics (any driver-chosen --steps window):
* every training step costs one env rollout step PLUS 1/batch_size of an
  `update` (10 inner iters of GNN forwards + backward + Adam on a ~300-graph
  batch), exactly the cadence `train.py` runs
  (reference gcbf/algo/gcbf.py:141-144: update every batch_size steps);
* exploration is sampled at the 500k-step schedule's midpoint (prob=0.5,
  the mean of the reference's linear 1→0 anneal, trainer/trainer.py:62), so
  ~half the timed steps run the actor GNN and half the zero-action path —
  representative of the whole run, not of its cheap first seconds;
* before timing, the replay buffer is prefilled through a full update cycle
  so the timed region samples the steady-state branch (current buffer +
  replay memory), and one untimed update absorbs one-time hipBLASLt
  algorithm-search / autograd-warmup costs;
* updates that fall inside the timed window run (and are timed) inline;
  the fractional remainder owed for a window shorter than batch_size is
  charged from a separately measured steady-state update (`update_s` in
  the output) — nothing in the training step is skipped or cached.

Launch (driver contract):
  python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W

--dump-outputs DIR writes, after the timed steps, what the last timed step
handed back to its caller as DIR/<name>.npy (float32): the next `states`,
`reward`, `reach`, `collision`, `done`, plus `u_ref` on the captured path or
`action` on the eager path, and `update_info` (float64: the metrics
returned by the last update that ran inside the timed window, if any).
Everything is seeded from --seed, so two runs with the same arguments start
from identical scenes and weights and their dumps can be compared array by
array.  --full is reserved for measurements beyond the headline figure;
the headline is all this benchmark measures today.

Weak scaling: each rank runs its own env replica; gradients all-reduce over
RCCL/xGMI each inner iteration; whole-node value = N · K / max_rank_time.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

from gcbf_amd.algo import make_algo
from gcbf_amd.env import make_env
from gcbf_amd.parallel import (broadcast_modules,
                               cleanup_distributed, init_distributed,
                               make_grad_synchronizer)
from gcbf_amd.trainer.utils import read_params, set_seed

SCHEDULE_TOTAL = 500_000      # the paper run's exploration schedule length
SCHEDULE_MIDPOINT = 250_000   # representative point: prob = 0.5


def _barrier_sync(device):
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
    if device.type == "cuda":
        torch.cuda.synchronize(device)


def _dump_outputs(out_dir, arrays):
    """Write each array as <out_dir>/<name>.npy (float32, or float64 where
    it already is): the timed path's last-step outputs, a few KB in all."""
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        t = t.detach().cpu()
        if t.dtype != torch.float64:
            t = t.float()
        np.save(os.path.join(out_dir, f"{name}.npy"), t.numpy())


def _self_launch_torchrun(args):
    """Driver asked for N>1 GPUs without torchrun: re-exec under
    torch.distributed.run instead of silently reporting 1-GPU numbers."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={args.gpus}", "--standalone",
           "--local-addr", "127.0.0.1", os.path.abspath(__file__),
           ] + sys.argv[1:]
    print(f"# --gpus {args.gpus} without torchrun: re-launching via "
          f"torch.distributed.run", flush=True)
    raise SystemExit(subprocess.call(cmd))


def run(args):
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        _self_launch_torchrun(args)
    env_world = int(os.environ.get("WORLD_SIZE", "1"))
    if env_world != args.gpus:
        # checked BEFORE init_process_group (which would block on the
        # rendezvous): never report numbers under a mislabeled n_gpus
        print(f"# FATAL: WORLD_SIZE={env_world} but --gpus {args.gpus}; "
              f"refusing to report mislabeled numbers", flush=True)
        raise SystemExit(2)
    rank, world_size, local_rank = init_distributed()
    set_seed(args.seed + rank)

    use_cuda = torch.cuda.is_available()
    device = torch.device(
        "cuda", local_rank % torch.cuda.device_count()) if use_cuda \
        else torch.device("cpu")
    if use_cuda:
        torch.cuda.set_device(device)
    dtype = args.dtype or ("bf16" if use_cuda else "fp32")

    params_env = make_env(args.env, args.num_agents, device).default_params
    params_env["num_obs"] = args.obs
    if args.area_size is not None:
        params_env["area_size"] = args.area_size
    env = make_env(args.env, args.num_agents, device, params=params_env)
    env.train()
    hyper = read_params(args.env, "gcbf")
    algo = make_algo("gcbf", env, args.num_agents, env.node_dim,
                     env.edge_dim, env.action_dim, device,
                     batch_size=args.batch_size, hyperparams=hyper)
    if world_size > 1:
        broadcast_modules([algo.cbf, algo.actor])
        algo.grad_sync = make_grad_synchronizer([algo.cbf, algo.actor])
    if dtype == "bf16":
        from gcbf_amd.utils.amp import enable_bf16
        enable_bf16(algo)

    data = env.reset()
    counters = {"policy": 0, "explore": 0, "resets": 0}

    engine = None
    if use_cuda and not args.no_capture:
        from gcbf_amd.rollout import RolloutEngine, engine_supported
        if engine_supported(env, algo):
            try:
                engine = RolloutEngine(env, algo)
                if rank == 0:
                    print("# hipGraph-captured rollout engine active",
                          flush=True)
            except Exception as e:
                engine = None
                if rank == 0:
                    print(f"# rollout capture unavailable ({e}); "
                          f"eager loop", flush=True)

    # probability of the exploration (zero-action) branch at the schedule's
    # representative midpoint; the branch itself is still Bernoulli-sampled
    # per step, exactly like training
    prob = 1 - (SCHEDULE_MIDPOINT - 1) / SCHEDULE_TOTAL
    updates = {"in_region": 0, "update_s": None, "step": 0}

    def rollout_step(count=False, keep=None):
        """One training env step.  `keep` (a dict) receives clones of what
        this step hands back to its caller (--dump-outputs, last step)."""
        nonlocal data
        updates["step"] += 1
        take_explore = np.random.rand() < prob
        if count:
            counters["explore" if take_explore else "policy"] += 1
        if engine is not None:
            # engine.step draws its own Bernoulli: pass prob 1/0 to pin the
            # branch we drew here (identical distribution, lets us count)
            was_eager = engine._eager
            done = engine.step(prob=1.0 if take_explore else 0.0)
            if keep is not None:
                # before reload() overwrites the engine's state buffers
                if was_eager:
                    keep.update(states=env.data.states.clone())
                else:
                    c = engine.cur
                    keep.update(states=engine.states[c].clone(),
                                u_ref=engine.u_ref[c].clone(),
                                reward=engine.reward_buf.clone(),
                                reach=engine.reach_buf.clone(),
                                collision=engine.coll_buf.clone())
                keep["done"] = torch.tensor([float(done)])
            if done:
                engine.reload()
                if count:
                    counters["resets"] += 1
        else:
            data.update(u_ref=env.u_ref(data))
            action = algo.step(data, prob=1.0 if take_explore else 0.0)
            next_data, reward, done, info = env.step(action)
            if keep is not None:
                keep.update(action=action.clone(),
                            states=next_data.states.clone(),
                            reward=reward.clone(),
                            reach=info["reach"].clone(),
                            collision=info["collision"].clone(),
                            done=torch.tensor([float(done)]))
            data = env.reset() if done else next_data

    def run_update():
        return algo.update(updates["step"], None)

    # ---- warmup (untimed, driver contract) ----
    for _ in range(args.warmup):
        rollout_step()

    # ---- prefill to steady state (untimed) ----
    # cycle 1: fill buffer -> update (absorbs one-time hipBLASLt search /
    # autograd warmup; populates replay memory so later samples take the
    # steady-state branch)
    while algo.buffer.size < args.batch_size:
        rollout_step()
    run_update()
    # cycle 2: fill buffer again -> measure one steady-state update (this
    # is the amortization basis for fractional owed updates)
    while algo.buffer.size < args.batch_size:
        rollout_step()
    _barrier_sync(device)
    tu0 = time.perf_counter()
    run_update()
    _barrier_sync(device)
    t_update = time.perf_counter() - tu0
    if torch.distributed.is_initialized():
        t = torch.tensor([t_update], dtype=torch.float64,
                         device=device if use_cuda else "cpu")
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        t_update = float(t.item())
    updates["update_s"] = t_update

    # ---- timed region: EXACTLY --steps training steps ----
    # buffer is empty (post-update), so natural updates fire inside the
    # region after each full batch_size of steps, timed inline
    _barrier_sync(device)
    t0 = time.perf_counter()
    last = {}           # outputs of the last timed step (--dump-outputs)
    update_info = None  # return value of the last update inside the region
    keep_at = args.steps - 1 if args.dump_outputs else -1
    for i in range(args.steps):
        rollout_step(count=True, keep=last if i == keep_at else None)
        if algo.buffer.size >= args.batch_size:
            update_info = run_update()
            updates["in_region"] += 1
    _barrier_sync(device)
    region = time.perf_counter() - t0

    # charge the fractional update still owed for this window
    owed = args.steps / args.batch_size - updates["in_region"]
    owed = max(0.0, owed)
    elapsed = region + owed * t_update

    # max over ranks
    if torch.distributed.is_initialized():
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device=device if use_cuda else "cpu")
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())

    if rank == 0 and args.dump_outputs:
        if update_info is not None:
            last["update_info"] = torch.tensor(
                [update_info[k] for k in sorted(update_info)],
                dtype=torch.float64)
        _dump_outputs(args.dump_outputs, last)

    if rank == 0:
        value = args.gpus * args.steps / elapsed
        print(json.dumps({
            "metric": "env-steps/sec (whole node)",
            "value": round(value, 2),
            "unit": "env-steps/s",
            "n_gpus": args.gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1000, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": dtype,
            "data": "synthetic",
            "config": {
                "model": "GCBF (CBFGNN 12.2M + GNNController 12.2M)",
                "env": args.env,
                "num_agents": args.num_agents,
                "num_obs": args.obs,
                "global_batch": args.batch_size * args.gpus,
                "seq_len": None,
                "parallelism": f"dp{args.gpus}",
            },
            "detail": {
                "schedule_prob": prob,
                "policy_steps": counters["policy"],
                "explore_steps": counters["explore"],
                "episode_resets": counters["resets"],
                "updates_in_region": updates["in_region"],
                "updates_amortized": round(owed, 4),
                "update_s": round(t_update, 4),
                "rollout_region_s": round(region, 4),
            },
        }), flush=True)
    cleanup_distributed()


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    cpu_fallback = not torch.cuda.is_available()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=64 if cpu_fallback else 1024)
    p.add_argument("--warmup", type=int, default=8 if cpu_fallback else 64)
    p.add_argument("--env", type=str, default="DubinsCar")
    p.add_argument("-n", "--num-agents", type=int, default=16)
    p.add_argument("--obs", type=int, default=0)
    p.add_argument("--area-size", type=float, default=None)
    p.add_argument("--batch-size", type=int,
                   default=64 if cpu_fallback else 512)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--dtype", type=str, default=None,
                   choices=[None, "bf16", "fp32"])
    p.add_argument("--no-capture", action="store_true", default=False,
                   help="disable the hipGraph rollout engine")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps, write what the last timed "
                        "step returned (next states, rewards, reach / "
                        "collision flags, done; the last in-window "
                        "update's metrics if one ran) as DIR/<name>.npy")
    p.add_argument("--full", action="store_true", default=False,
                   help="also run the measurements beyond the headline "
                        "figure; a plain run does only set-up, warm-up, "
                        "the timed steps and the result line (today the "
                        "headline is all this benchmark measures, so the "
                        "two runs coincide)")
    run(p.parse_args())
