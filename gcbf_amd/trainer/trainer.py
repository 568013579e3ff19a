"""Training loop (reference gcbf/trainer/trainer.py:15-141).

Additions over the reference:
* an env-steps/sec throughput meter (the headline benchmark metric);
* optional training resume (optimizer + step state in ``trainer_state.pt``,
  a new file beside the reference-compatible checkpoint layout);
* data-parallel awareness: only rank 0 logs/saves; the step loop itself is
  identical on every rank (per-rank envs and buffers, gradient all-reduce
  happens inside ``algo.update`` via the ``grad_sync`` hook).
"""
from __future__ import annotations

import os
import time
from typing import Tuple

import numpy as np
import torch

from ..algo.base import Algorithm
from ..env.base import MultiAgentEnv
from .summary import SummaryWriter, NullWriter


class Trainer:

    def __init__(self, env: MultiAgentEnv, env_test: MultiAgentEnv,
                 algo: Algorithm, log_dir: str, rank: int = 0,
                 world_size: int = 1, eval_batch: bool = False,
                 num_envs: int = 1, capture_capped: bool = False):
        self.env = env
        self.env_test = env_test
        self.algo = algo
        self.log_dir = log_dir
        self.rank = rank
        self.world_size = world_size
        # opt-in: run the eval episodes as one SceneBatch
        self.eval_batch = eval_batch
        # opt-in: let the captured rollout engines (gcbf_amd/rollout.py,
        # and with num_envs > 1 gcbf_amd/vec_rollout.py) take MACBF and
        # neighbour-capped scenes too; off keeps their eager loop
        self.capture_capped = bool(capture_capped)
        # opt-in: collect from num_envs scenes per captured step
        # (gcbf_amd/vec_rollout.py); 1 keeps the single-scene loop
        self.num_envs = int(num_envs)
        if self.num_envs < 1:
            raise ValueError("num_envs must be at least 1")
        if self.num_envs > 1:
            if world_size > 1:
                raise ValueError(
                    "num_envs > 1 together with world_size > 1 is untested "
                    "and refused: use one rank, or num_envs=1")
            batch_size = getattr(algo, "batch_size", None)
            if batch_size is not None and batch_size % self.num_envs != 0:
                raise ValueError(
                    f"batch_size ({batch_size}) must be a multiple of "
                    f"num_envs ({self.num_envs})")

        if rank == 0:
            os.makedirs(log_dir, exist_ok=True)
            self.model_dir = os.path.join(log_dir, "models")
            os.makedirs(self.model_dir, exist_ok=True)
            self.writer = SummaryWriter(log_dir=os.path.join(log_dir,
                                                             "summary"))
        else:
            self.model_dir = os.path.join(log_dir, "models")
            self.writer = NullWriter()

    def _make_engine(self):
        """hipGraph-captured rollout when supported (GPU + HIP ext + GCBF;
        with ``capture_capped`` also MACBF and neighbour-capped scenes)."""
        try:
            from ..rollout import RolloutEngine, engine_supported
            if engine_supported(self.env, self.algo,
                                capped=self.capture_capped):
                if self.env.data is None:
                    self.env.reset()
                return RolloutEngine(self.env, self.algo)
        except Exception as e:
            if self.rank == 0:
                print(f"> rollout capture unavailable ({e}); "
                      f"using the eager loop", flush=True)
        return None

    def train(self, steps: int, eval_interval: int, eval_epi: int,
              start_step: int = 1, capture: bool = True):
        if self.num_envs > 1:
            engine = self._make_vec_engine()
            if engine is not None:
                return self._train_vec(engine, steps, eval_interval,
                                       eval_epi, start_step)
        start_time = time.time()
        data = self.env.reset()
        engine = self._make_engine() if capture else None
        if engine is not None and self.rank == 0:
            print("> hipGraph-captured rollout engine active", flush=True)
        last_report = start_time
        steps_since_report = 0

        verbose = None
        for step in range(start_step, steps + 1):
            if engine is not None:
                done = engine.step(prob=1 - (step - 1) / steps)
                if done:
                    engine.reload()
            else:
                if data.u_ref is None:
                    data.update(u_ref=self.env.u_ref(data))
                action = self.algo.step(data, prob=1 - (step - 1) / steps)
                next_data, reward, done, info = self.env.step(action)
                next_data.update(u_ref=self.env.u_ref(next_data))
                self.algo.post_step(data, action, reward, done, next_data)
                data = self.env.reset() if done else next_data

            if self.algo.is_update(step):
                verbose = self.algo.update(step, self.writer)

            steps_since_report += 1
            now = time.time()
            if now - last_report > 30 and self.rank == 0:
                rate = steps_since_report / (now - last_report)
                self.writer.add_scalar("perf/env_steps_per_sec",
                                       rate * self.world_size, step)
                print(f"step {step}/{steps} | "
                      f"{rate * self.world_size:.1f} env-steps/s (whole job)",
                      flush=True)
                last_report, steps_since_report = now, 0

            if step % eval_interval == 0:
                self._eval_and_save(step, eval_epi, start_time, verbose)

        if self.rank == 0:
            print(f"> Done in {time.time() - start_time:.0f} seconds",
                  flush=True)

    def _eval_and_save(self, step: int, eval_epi: int, start_time: float,
                       verbose):
        if eval_epi > 0 and self.rank == 0:
            reward_mean, eval_info = self.eval(step, eval_epi)
            msg = (f"step: {step}, time: "
                   f"{time.time() - start_time:.0f}s, "
                   f"reward: {reward_mean:.2f}")
            for key, val in eval_info.items():
                msg += f", {key}: {val}"
            print(msg, flush=True)
        if verbose is not None and self.rank == 0:
            print("step: " + str(step) + "".join(
                f", {k}: {v:.3f}" for k, v in verbose.items()),
                flush=True)
        if self.rank == 0:
            self.algo.save(os.path.join(self.model_dir, f"step_{step}"))
            self._save_trainer_state(step)
        self.algo._env = self.env

    # ------------------------------------------------- vectorized collection
    def _make_vec_engine(self):
        """The B-scene engine, or None (with the reason printed) where it
        does not apply: the single-scene path then runs as always.  MACBF
        and neighbour-capped scenes need ``capture_capped`` here too."""
        from ..vec_rollout import (VecRolloutEngine,
                                   vec_engine_unsupported_reason)
        if self.env.data is None:
            self.env.reset()
        reason = vec_engine_unsupported_reason(
            self.env, self.algo, self.num_envs, capped=self.capture_capped)
        if reason is None:
            try:
                return VecRolloutEngine(self.env, self.algo, self.num_envs,
                                        capped=self.capture_capped)
            except Exception as e:
                reason = str(e)
        if self.rank == 0:
            print(f"> vectorized rollout unavailable ({reason}); "
                  f"using the single-scene path", flush=True)
        return None

    def _train_vec(self, engine, steps: int, eval_interval: int,
                   eval_epi: int, start_step: int):
        """The training loop over B scenes per engine step: ``step`` counts
        env steps and advances by B.  The engine's pending snapshots are
        flushed into the buffer before every update, which comes when
        ``step`` reaches a multiple of the algorithm's batch size; eval and
        save when it crosses a multiple of ``eval_interval``."""
        B = engine.B
        start_time = time.time()
        if self.rank == 0:
            print(f"> vectorized rollout engine active ({B} scenes, "
                  f"{'captured' if engine.g is not None else 'plain'} "
                  f"body)", flush=True)
        batch_size = self.algo.batch_size
        last_report = start_time
        steps_since_report = 0
        verbose = None
        step = start_step - 1           # env steps taken so far
        while step < steps:
            # exploration probability of the group's first env step
            engine.step(prob=1 - step / steps)
            prev, step = step, step + B

            if step // batch_size > prev // batch_size:
                engine.flush()
                verbose = self.algo.update(step, self.writer)

            steps_since_report += B
            now = time.time()
            if now - last_report > 30 and self.rank == 0:
                rate = steps_since_report / (now - last_report)
                self.writer.add_scalar("perf/env_steps_per_sec", rate, step)
                print(f"step {step}/{steps} | {rate:.1f} env-steps/s "
                      f"({B} scenes)", flush=True)
                last_report, steps_since_report = now, 0

            if step // eval_interval > prev // eval_interval:
                self._eval_and_save(step, eval_epi, start_time, verbose)

        if self.rank == 0:
            print(f"> Done in {time.time() - start_time:.0f} seconds",
                  flush=True)

    def _save_trainer_state(self, step: int):
        """Resume state (new vs. reference, separate file)."""
        if not hasattr(self.algo, "extra_state"):
            return
        torch.save({"step": step, "algo": self.algo.extra_state()},
                   os.path.join(self.log_dir, "trainer_state.pt"))

    def load_trainer_state(self) -> int:
        """Returns the step to resume from (1 if no state)."""
        path = os.path.join(self.log_dir, "trainer_state.pt")
        if not os.path.exists(path):
            return 1
        state = torch.load(path, map_location=self.algo.device,
                           weights_only=False)
        if hasattr(self.algo, "load_extra_state"):
            self.algo.load_extra_state(state["algo"])
        return state["step"] + 1

    def eval(self, step: int, eval_epi: int) -> Tuple[float, dict]:
        # reference gcbf/trainer/trainer.py:95-141
        if self.eval_batch:
            return self._eval_batched(step, eval_epi)
        rewards = []
        safe_rate = []
        reach = torch.zeros(self.env_test.num_agents)
        self.algo._env = self.env_test
        for _ in range(eval_epi):
            safe_agent = torch.ones(self.env_test.num_agents).bool()
            data = self.env_test.reset()
            epi_reward = 0.0
            while True:
                data.update(u_ref=self.env_test.u_ref(data))
                action = self.algo.apply(data)
                data, reward, done, info = self.env_test.step(action)
                epi_reward += float(reward.float().mean())
                if "collision" in info:
                    safe_agent[info["collision"].cpu()] = False
                if "reach" in info:
                    reach = info["reach"]
                if done:
                    break
            rewards.append(epi_reward)
            safe_rate.append(safe_agent.sum().item()
                             / self.env_test.num_agents)

        self.writer.add_scalar("test/reward", float(np.mean(rewards)), step)
        self.writer.add_scalar("test/safe_rate", float(np.mean(safe_rate)),
                               step)
        return float(np.mean(rewards)), {
            "safe": round(float(np.mean(safe_rate)), 2),
            "reach": round(float(torch.mean(reach.float())), 2)}

    def _eval_batched(self, step: int, eval_epi: int) -> Tuple[float, dict]:
        """The eval episodes as one SceneBatch; same scalars and returned
        dict as the sequential loop.  The layouts are drawn from seeds taken
        off the global RNG, and "reach" is the last episode's, as there."""
        from .utils import eval_ctrl_batched
        self.algo._env = self.env_test
        seeds = [int(np.random.randint(100000)) for _ in range(eval_epi)]
        rewards, _, info = eval_ctrl_batched(
            self.algo.apply, self.env_test, seeds, verbose=False)
        self.writer.add_scalar("test/reward", float(np.mean(rewards)), step)
        self.writer.add_scalar("test/safe_rate",
                               float(np.mean(info["safe"])), step)
        return float(np.mean(rewards)), {
            "safe": round(float(np.mean(info["safe"])), 2),
            "reach": round(float(info["reach"][-1]), 2)}
