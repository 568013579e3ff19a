"""SceneBatch: B episodes of one point-agent env stepped together.

The env objects hold one scene (goal, obstacles, step counter, graph).  A
``SceneBatch`` wraps one of them and owns ``states (B, N, S)``,
``goal (B, n, G)``, ``t (B,)``, ``active (B,)`` and the current
``GraphBatch`` of B graphs.  One ``step`` is one ``ops.env_step_batched``
launch (ops/hip/env_step_batched.hip) plus one batched ``ops.build_graph``
over all B·N nodes; scenes that finished are parked by the ``active`` flags
and contribute nothing further.  ``step`` returns device tensors and never
syncs the host — ``all_done()`` is the one small readback and the caller
decides how often to ask.

Policies see the batch through the wrapped env: inside ``scenes()`` the
env's ``u_ref``, ``forward_graph``, ``dynamics`` and masks use the per-scene
goals and obstacles (including the freeze of reached agents, which the envs
otherwise apply to their single scene only).  Outside the context the env
is exactly what it was.
"""
from __future__ import annotations

from contextlib import contextmanager
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from .. import ops
from ..graph import GraphBatch
from .point_agent import PointAgentEnv
from .utils import device_rejection_sample


class SceneBatch:

    def __init__(self, env: PointAgentEnv, B: int):
        if not isinstance(env, PointAgentEnv):
            raise NotImplementedError(
                "SceneBatch needs a point-agent env (SimpleCar, DubinsCar, "
                "SimpleDrone)")
        if env._mode not in ("train", "test", "demo_2"):
            raise NotImplementedError(
                f"SceneBatch does not support the box-world mode "
                f"{env._mode!r}: its node count varies per scene and step")
        if B < 1:
            raise ValueError("SceneBatch needs at least one scene")
        self.env = env
        self.B = int(B)
        self.states: Optional[Tensor] = None
        self.goal: Optional[Tensor] = None
        self.t: Optional[Tensor] = None
        self.active: Optional[Tensor] = None
        self.data: Optional[GraphBatch] = None
        self._published = False

    # ----------------------------------------------------------------- sizes
    @property
    def num_agents(self) -> int:
        return self.env.num_agents

    @property
    def nodes_per_scene(self) -> int:
        return self.states.shape[1]

    # ----------------------------------------------------------------- reset
    def reset(self, seeds: Sequence[int]) -> GraphBatch:
        """Start B fresh episodes.  Host path: scene b is, bit for bit, the
        layout ``set_seed(seeds[b]); env.reset()`` produces.  With the env's
        ``device_reset`` on, all scenes are drawn on the device at once
        (seeded by ``seeds[0]``)."""
        from ..trainer.utils import set_seed
        env = self.env
        assert len(seeds) == self.B, "one seed per scene"
        if env._use_device_reset():
            set_seed(int(seeds[0]))
            states, goal, x, agent_mask = self._draw_device()
        else:
            per_scene = []
            for seed in seeds:
                set_seed(int(seed))
                data = env.reset()
                per_scene.append((data.states, env._goal))
            states = torch.stack([s for s, _ in per_scene])
            goal = torch.stack([g for _, g in per_scene])
            x, agent_mask = env.data.x, env.data.agent_mask
        B, N = self.B, states.shape[1]
        dev = states.device
        self.states, self.goal = states.contiguous(), goal.contiguous()
        self._x = x.repeat(B, 1)
        self._agent_mask = None if agent_mask is None else agent_mask.repeat(B)
        self._ptr = torch.arange(B + 1, device=dev) * N
        self.t = torch.zeros(B, dtype=torch.int32, device=dev)
        self.active = torch.ones(B, dtype=torch.int32, device=dev)
        n = env.num_agents
        # per-agent accounting, masked by `active`
        self.collided = torch.zeros(B, n, dtype=torch.bool, device=dev)
        self.reach_last = torch.zeros(B, n, dtype=torch.bool, device=dev)
        self.reward_sum = torch.zeros(B, dtype=torch.float64, device=dev)
        self.length = torch.zeros(B, dtype=torch.int32, device=dev)
        self.data = self._link(self.states)
        with self.scenes():
            self.data.update(u_ref=env.u_ref(self.data))
        return self.data

    def _draw_device(self) -> Tuple[Tensor, Tensor, Tensor, Optional[Tensor]]:
        """All scenes from the device RNG: the obstacles in one call, the
        starts and goals as 2B problems of ops.reset_sample (problems
        0..B-1 the starts, B..2B-1 the goals) with per-problem avoid sets,
        one launch per candidate pool."""
        env, B = self.env, self.B
        n, p, dev = env.num_agents, env.pos_dim, env.device
        par = env.params
        side, r = par["area_size"], env.agent_radius
        kind = env._step_kind
        goal_sep = 5 * r if kind == "dubins" else 4 * r
        obs = None
        if kind == "dubins":
            obs = torch.rand(B, env._num_obs, env.state_dim, device=dev)
            obs[..., :2] *= side
            obs[..., 2] *= torch.pi * 2
            obs[..., 3] *= par["obs_speed_limit"]
        elif kind == "drone":
            # reference quirk: always num_agents obstacles
            obs = torch.cat([
                torch.rand(B, n, 3, device=dev) * side,
                torch.zeros(B, n, env.state_dim - 3, device=dev)], dim=-1)
        avoid, clearance = None, 0.0
        if obs is not None:
            avoid = obs[..., :p].repeat(2, 1, 1).contiguous()
            clearance = 2 * r + 2 * par["obs_point_r"]
        pts = device_rejection_sample(
            n, p, side, (4 * r,) * B + (goal_sep,) * B, avoid, clearance, dev)
        rest = torch.zeros(2 * B, n, env.state_dim - p, device=dev)
        if kind == "dubins":   # headings, starts before goals
            rest[..., 0] = torch.rand(2 * B, n, device=dev) * 2 * torch.pi \
                - torch.pi
        full = torch.cat([pts, rest], dim=-1)
        starts, goal = full[:B], full[B:]
        if kind == "car":
            return starts, goal[..., :p], torch.zeros_like(starts[0]), None
        states = torch.cat([starts, obs], dim=1)
        n_obs = obs.shape[1]
        x = torch.cat([torch.zeros(n, env.node_dim, device=dev),
                       torch.ones(n_obs, env.node_dim, device=dev)])
        agent_mask = torch.zeros(n + n_obs, dtype=torch.bool, device=dev)
        agent_mask[:n] = True
        return states, goal, x, agent_mask

    def _link(self, states: Tensor) -> GraphBatch:
        """Freshly linked GraphBatch of all B scenes: one batched graph
        build over the B·N nodes."""
        flat = states.reshape(-1, states.shape[-1])
        data = GraphBatch(x=self._x, pos=flat[:, :self.env.pos_dim],
                          states=flat, agent_mask=self._agent_mask,
                          ptr=self._ptr)
        return self.env.add_communication_links(data)

    # ------------------------------------------------------------------ step
    def step(self, action: Tensor) -> Tuple[GraphBatch, Tensor, Tensor, dict]:
        """Advance every active scene by one step with the (B·n, A) residual
        ``action``.  Returns ``(data, reward (B, n), done (B,), info)``, all
        on the device; ``info`` holds ``reach``, ``collision`` (B, n) and
        ``active`` (B,), the flags this step ran with."""
        env, B, n = self.env, self.B, self.env.num_agents
        ran = self.active
        new_states, u_ref_next, reward, reach, collision, reach_all = \
            ops.env_step_batched(*env.batched_step_args(
                self.states, self.goal, action.reshape(B, n, -1), ran))
        live = ran.bool()
        self.t = self.t + ran
        self.length = self.length + ran
        self.collided = self.collided | collision
        self.reach_last = torch.where(live.unsqueeze(1), reach,
                                      self.reach_last)
        self.reward_sum = self.reward_sum + reward.double().mean(dim=1)
        done = reach_all | (self.t >= env.max_episode_steps)
        self.active = ran * torch.logical_not(done).to(ran.dtype)
        self.states = new_states
        self.data = self._link(new_states)
        self.data.update(u_ref=u_ref_next.reshape(B * n, -1))
        if self._published:
            self._publish()
        return self.data, reward, done, {
            "reach": reach, "collision": collision, "active": live}

    def all_done(self) -> bool:
        """True once no scene is active (one small host readback)."""
        return not bool(self.active.any())

    # ---------------------------------------------------------------- scenes
    def _publish(self):
        env, n = self.env, self.env.num_agents
        env._goal = self.goal
        env._obs = None if self._agent_mask is None else \
            self.states[:, n:].reshape(-1, self.states.shape[-1])
        env._scenes = self.B
        env._live_rows = self.active.bool().repeat_interleave(n).unsqueeze(1)

    @contextmanager
    def scenes(self):
        """Inside, the wrapped env answers for the whole scene batch:
        per-scene goals and obstacles in ``u_ref``, ``forward_graph`` and
        ``dynamics`` (with the freeze of reached agents)."""
        env = self.env
        saved = (env._goal, env._obs, env._scenes, env._live_rows)
        was_published = self._published
        self._published = True
        self._publish()
        try:
            yield self
        finally:
            self._published = was_published
            env._goal, env._obs, env._scenes, env._live_rows = saved
