"""Shared concrete layer of the point-agent environments.

SimpleCar, DubinsCar and SimpleDrone are the same environment — agents are
discs/spheres of one radius, optional obstacle nodes follow the agent rows,
agents receive edges from everything within the communication radius — with
different dynamics, reference controller and constants.  Everything but
those lives here, once; an env declares its constants as class attributes
and implements ``default_params``, the dimensions, ``dynamics``, ``u_ref``,
the draw part of ``reset``, ``state_lim`` and ``render``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import ops
from ..graph import GraphBatch
from .base import MultiAgentEnv


class PointAgentEnv(MultiAgentEnv):

    # ---- per-env declarations -------------------------------------------
    pos_dim: int                      # leading state columns that are position
    _radius_key: str                  # params key of the agent radius
    _step_kind: str                   # fused-step kernel (ops/hip/env_step.hip)
    _env_kind: int                    # fused-mask kernel (ops/hip/masks.hip)
    _attr_kind: int = ops.ATTR_DIFF   # edge_attr of the fused graph builder
    _action_limit: float              # |u| bound, every action component
    # eager step rewards: per step, per collision, per newly reached goal,
    # per unit action norm (per agent, or summed over all agents)
    _reward_step: float
    _reward_collision: float
    _reward_reach: float
    _action_cost: float
    _action_cost_summed: bool = False
    # mask thresholds in agent radii: safe_mask distance, unsafe_mask warn
    # zone, and the unsafe_mask diagonal offset (k·r + 1)
    _safe_radii: int
    _warn_radii: int
    _unsafe_diag_radii: int = 4

    def __init__(self, num_agents: int, device: torch.device, dt: float = 0.03,
                 params: Optional[dict] = None,
                 max_neighbors: Optional[int] = None):
        super().__init__(num_agents, device, dt, params, max_neighbors)
        self._K: Optional[Tensor] = None     # LQR gain, built by u_ref
        self._goal: Optional[Tensor] = None
        self._obs: Optional[Tensor] = None   # obstacle states; None: no rows
        self._xy_min = None
        self._xy_max = None
        # points whose plot limits are still owed (device-reset path)
        self._plot_pts: Optional[Tensor] = None
        # set by SceneBatch.scenes(): number of scenes whose (B, n, G) goals
        # and flat obstacle rows the env currently holds, and the (B*n, 1)
        # mask of agents in scenes that are still running
        self._scenes = 1
        self._live_rows: Optional[Tensor] = None

    @property
    def agent_radius(self) -> float:
        return self._params[self._radius_key]

    @property
    def action_lim(self) -> Tuple[Tensor, Tensor]:
        upper = torch.ones(self.action_dim, device=self.device) \
            * self._action_limit
        return -upper, upper

    def _agent_rows(self, data: GraphBatch) -> Tensor:
        """States of the agent nodes of a (batched) graph."""
        if data.agent_index is not None:   # capture-safe integer indexing
            return data.states.index_select(0, data.agent_index)
        if data.agent_mask is not None:
            return data.states[data.agent_mask]
        return data.states

    def _freeze_applies(self, states: Tensor) -> bool:
        """Reached agents freeze only in the graph(s) the env itself holds:
        its single scene, or inside ``SceneBatch.scenes()`` the whole scene
        batch.  The shape check excludes update-path batches exactly like
        the reference's (gcbf/env/dubins_car.py:126-132)."""
        return self._obs is not None and states.shape[0] == \
            self._scenes * self.num_agents + self._obs.shape[0]

    def _reached(self, agent_states: Tensor) -> Tensor:
        p = self.pos_dim
        return torch.less(
            torch.norm(agent_states[:, :p] - self._goal[:, :p], dim=1),
            self._params["dist2goal"])

    # ----------------------------------------------------------------- reset
    def _at_rest(self, pos: Tensor) -> Tensor:
        """Full states at ``pos`` with every other component zero."""
        return torch.cat([pos, torch.zeros(
            pos.shape[0], self.state_dim - self.pos_dim, device=pos.device)],
            dim=1)

    def _sample_goals_near(self, pos: Tensor, min_sep: float) -> Tensor:
        """demo_2 goal sampling: within max_distance of the agent's start
        (reference gcbf/env/simple_car.py:111-121)."""
        side = self._params["area_size"]
        max_d = self._params["max_distance"]
        goals = torch.zeros(self.num_agents, pos.shape[1])
        i = 0
        while i < self.num_agents:
            cand = (torch.rand(pos.shape[1]) * 2 - 1) * max_d + pos[i].cpu()
            if (cand > side).any() or (cand < 0).any():
                continue
            if torch.norm(goals - cand, dim=1).min() <= min_sep:
                continue
            goals[i] = cand
            i += 1
        return goals

    def _build_data(self, agent_states: Tensor) -> GraphBatch:
        """Unlinked graph of the agents followed by the obstacle rows."""
        if self._obs is None:
            return GraphBatch(x=torch.zeros_like(agent_states),
                              pos=agent_states[:, :self.pos_dim],
                              states=agent_states)
        n_obs = self._obs.shape[0]
        x = torch.cat([
            torch.zeros(self.num_agents, self.node_dim),
            torch.ones(n_obs, self.node_dim)], dim=0).type_as(agent_states)
        states = torch.cat([agent_states, self._obs], dim=0)
        agent_mask = torch.zeros(self.num_agents + n_obs, dtype=torch.bool,
                                 device=self.device)
        agent_mask[:self.num_agents] = True
        g = GraphBatch(x=x, pos=states[:, :self.pos_dim], states=states,
                       agent_mask=agent_mask)
        g.agents_first_n = self.num_agents
        return g

    def _finish_reset(self, states: Tensor, goals: Tensor) -> GraphBatch:
        """Reset tail, after the env drew ``states``, ``goals`` and
        ``self._obs``: graph, links, plot limits."""
        self._goal = goals
        self._data = self.add_communication_links(self._build_data(states))
        p = self.pos_dim
        pts = [states[:, :p], goals[:, :p]]
        if self._obs is not None:
            pts.append(self._obs[:, :p])
        self._finish_reset_plot_limits(pts)
        return self._data

    def _finish_reset_plot_limits(self, pts):
        """Host path: limits computed eagerly, as always.  Device path: the
        points are kept on the device and the limits computed at the first
        render (or state_lim) after the reset, so a reset copies no
        positions back to the host."""
        points = torch.cat(pts, dim=0)
        if self._use_device_reset():
            self._plot_pts = points
            self._xy_min = self._xy_max = None
        else:
            self._set_plot_limits(points)

    def _ensure_plot_limits(self):
        if self._plot_pts is not None:
            self._set_plot_limits(self._plot_pts)

    def _set_plot_limits(self, points: Tensor):
        self._plot_pts = None
        pts = points.detach().cpu().numpy()
        r = self.agent_radius
        xy_min = np.min(pts, axis=0) - r * 5
        xy_max = np.max(pts, axis=0) + r * 5
        max_interval = (xy_max - xy_min).max()
        self._xy_min = xy_min - 0.5 * (max_interval - (xy_max - xy_min))
        self._xy_max = xy_max + 0.5 * (max_interval - (xy_max - xy_min))

    # ------------------------------------------------------------------ step
    def _step_u_ref(self) -> Tensor:
        """u_ref for the env's own step: reuse the value the trainer already
        attached this step (same states, same goal — identical), else
        compute (the reference recomputes it each time)."""
        if self._data.u_ref is not None:
            return self._data.u_ref
        return self.u_ref(self._data)

    def _get_K_tensor(self) -> Optional[Tensor]:
        if self._K is None:
            self.u_ref(self._data)  # lazily builds the LQR gain
        return self._K.contiguous()

    def fused_step_args(self, states: Tensor, goal: Tensor, action: Tensor,
                        K: Optional[Tensor] = None) -> list:
        """Argument list of ``ops.env_step_fused`` — the one place that
        knows its order.  ``K`` lets a caller pass its own address-stable
        copy of the LQR gain; envs without a gain leave it out."""
        if K is None:
            K = self._get_K_tensor()
        p = self._params
        return [self._step_kind, states, goal, action] \
            + ([] if K is None else [K]) \
            + [self.dt, p[self._radius_key], p["speed_limit"],
               p["dist2goal"], self._action_limit]

    def batched_step_args(self, states: Tensor, goal: Tensor, action: Tensor,
                          active: Tensor, K: Optional[Tensor] = None) -> list:
        """Argument list of ``ops.env_step_batched`` for ``(B, ·, ·)``
        states, goals and actions and the ``(B,)`` int32 ``active`` flags —
        the one place that knows its order."""
        if K is None:
            K = self._get_K_tensor()
        p = self._params
        return [self._step_kind, states, goal, action, active] \
            + ([] if K is None else [K]) \
            + [self.dt, p[self._radius_key], p["speed_limit"],
               p["dist2goal"], self._action_limit]

    def _advance(self, new_states: Tensor):
        """Make ``new_states`` the env's current, freshly linked graph."""
        data = GraphBatch(
            x=self._data.x, pos=new_states[:, :self.pos_dim],
            states=new_states, agent_mask=self._data.agent_mask)
        if data.agent_mask is not None:
            data.agents_first_n = self.num_agents
            self._obs = new_states[self.num_agents:]
        self._data = self.add_communication_links(data)

    def _step_result(self, reward: Tensor, reach: Tensor, collision: Tensor
                     ) -> Tuple[GraphBatch, Tensor, bool, dict]:
        done = bool(self._t >= self.max_episode_steps or reach.all())
        safe = 1.0 - collision.sum() / self.num_agents
        return self._data, reward, done, {
            "safe": safe, "reach": reach, "collision": collision}

    def _finish_fused_step(self, out) -> Tuple[GraphBatch, Tensor, bool, dict]:
        """Assemble the step return from the fused-kernel outputs."""
        new_states, u_ref_next, reward, reach, collision = out
        self._advance(new_states)
        self._data.u_ref = u_ref_next
        return self._step_result(reward, reach, collision)

    def step(self, action: Tensor) -> Tuple[GraphBatch, Tensor, bool, dict]:
        self._t += 1
        # fused single-kernel path on GPU (ops/hip/env_step.hip)
        out = ops.env_step_fused(*self.fused_step_args(
            self._data.states, self._goal, action))
        if out is not None:
            return self._finish_fused_step(out)

        # eager path, as the reference envs step.  Rewards/info stay on
        # device (one host sync per step, for `done`); callers that need
        # numpy use .cpu().numpy().
        cost = torch.norm(action, dim=1)
        if self._action_cost_summed:
            cost = cost.sum()
        reward_action = -cost * self._action_cost
        action = action + self._step_u_ref()
        lower_lim, upper_lim = self.action_lim
        action = torch.clamp(action, lower_lim, upper_lim)
        prev_reach = self._reached(self._agent_rows(self._data))
        with torch.no_grad():
            state = self.forward(self._data, action)
        self._advance(state)

        reach = self._reached(self._agent_rows(self._data))
        collision = self.collision_mask(self._data)
        reward_collision = -collision.int() * self._reward_collision
        reward_reach = (reach.int() - prev_reach.int()) * self._reward_reach
        reward = reward_reach + reward_collision + self._reward_step \
            + reward_action
        return self._step_result(reward.detach(), reach, collision)

    def forward_graph(self, data: GraphBatch, action: Tensor) -> GraphBatch:
        action = action + self.u_ref(data)
        lower_lim, upper_lim = self.action_lim
        action = torch.clamp(action, lower_lim, upper_lim)
        state = self.forward(data, action)
        return data.replace(
            edge_attr=self.edge_attr(state, data.edge_index),
            pos=state[:, :self.pos_dim],
            states=state,
        )

    # ----------------------------------------------------------------- graph
    def edge_attr(self, state: Tensor, edge_index: Tensor) -> Tensor:
        # edge_attr[e] = state[src] - state[dst]
        return state.index_select(0, edge_index[0]) - \
            state.index_select(0, edge_index[1])

    def add_communication_links(self, data: GraphBatch) -> GraphBatch:
        n_rec = None if data.agent_mask is None else self.num_agents
        edge_index, edge_attr = ops.build_graph(
            data.pos, data.states, n_rec, self._params["comm_radius"],
            self._max_neighbors, data.num_graphs, self._attr_kind,
            self.edge_dim, self.edge_attr)
        data.update(edge_index=edge_index, edge_attr=edge_attr)
        return data

    # uniform node counts make the batched rebuild identical to the per-graph
    # one, so the same call handles both
    add_communication_links_batched = add_communication_links

    # ----------------------------------------------------------------- masks
    def _fused_mask(self, data: GraphBatch, which: str):
        return ops.fused_masks(data.states, data.num_graphs,
                               self._mask_rows(data), self.agent_radius,
                               self._env_kind, which)

    def _mask_rows(self, data: GraphBatch) -> int:
        # receiver rows per graph: all nodes without obstacles, else agents
        if data.agent_mask is None:
            return data.nodes_per_graph
        return self.num_agents

    def _pairwise_agent_rows(self, data: GraphBatch, diag_offset: float
                             ) -> Tuple[Tensor, Tensor]:
        """pos-diff (B, n_agents, N, pos_dim) and distance with the diag
        offset on the agent-self entries."""
        B = data.num_graphs
        N = data.nodes_per_graph
        n = self.num_agents
        p = data.states.view(B, N, -1)[:, :, :self.pos_dim]
        pd = p[:, :n].unsqueeze(2) - p.unsqueeze(1)  # [b, i, j]
        dist = pd.norm(dim=-1)
        eye = torch.eye(N, device=data.device, dtype=dist.dtype)[:n]
        return pd, dist + eye * diag_offset

    def _heading(self, agent_states: Tensor) -> Tensor:
        """(B, n, pos_dim) direction of travel for the unsafe_mask cone."""
        raise NotImplementedError

    def safe_mask(self, data: GraphBatch, return_edge: bool = False) -> Tensor:
        r = self.agent_radius
        if return_edge:
            return data.edge_attr[:, :self.pos_dim].norm(dim=-1) > 4 * r
        m = self._fused_mask(data, "safe")
        if m is not None:
            return m
        _, dist = self._pairwise_agent_rows(data, 4 * r + 1)
        return (dist > self._safe_radii * r).min(dim=2)[0].reshape(-1).bool()

    def unsafe_mask(self, data: GraphBatch, return_edge: bool = False) -> Tensor:
        r = self.agent_radius
        if return_edge:
            return data.edge_attr[:, :self.pos_dim].norm(dim=-1) < 2 * r
        m = self._fused_mask(data, "unsafe")
        if m is not None:
            return m
        pd, dist = self._pairwise_agent_rows(
            data, self._unsafe_diag_radii * r + 1)
        collision = (dist < 2 * r).max(dim=2)[0]

        # heading-into-neighbor cone inside the warn zone
        warn_zone = dist < self._warn_radii * r
        pos_vec = -(pd / (pd.norm(dim=-1, keepdim=True) + 1e-4))  # i -> j
        B, n, N = dist.shape
        theta_vec = self._heading(
            data.states.view(B, N, -1)[:, :n]).unsqueeze(2)
        inner = (pos_vec * theta_vec).sum(dim=-1)
        thr = torch.cos(torch.asin(2 * r / (dist + 1e-7)))
        unsafe = torch.logical_and(inner > thr, warn_zone).max(dim=2)[0]
        return torch.logical_or(collision, unsafe).reshape(-1).bool()

    def collision_mask(self, data: GraphBatch) -> Tensor:
        r = self.agent_radius
        m = self._fused_mask(data, "collision")
        if m is not None:
            return m
        _, dist = self._pairwise_agent_rows(data, 2 * r + 1)
        return (dist < 2 * r).max(dim=2)[0].reshape(-1).bool()
