"""SimpleCar: 2D double-integrator multi-agent environment.

Behavioral equivalent of the reference SimpleCar (gcbf/env/simple_car.py):
state [x, y, vx, vy], action [ax, ay], LQR reference controller, dense
radius graph over agents, pairwise safety masks.  All O(N²) mask work is
batched over the whole graph batch in single vectorized ops (the reference
loops over graphs in Python, gcbf/env/simple_car.py:313-327).
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch
from torch import Tensor

from .. import ops
from ..graph import GraphBatch
from .point_agent import PointAgentEnv
from .utils import lqr, plot_graph, fig_to_rgb_array, \
    rejection_sample_positions, device_rejection_sample


class SimpleCar(PointAgentEnv):

    pos_dim = 2
    _radius_key = "car_radius"
    _step_kind = "car"
    _env_kind = ops.ENV_CAR
    _action_limit = 10.0
    # reference gcbf/env/simple_car.py:146-176
    _reward_step = -0.01
    _reward_collision = 2
    _reward_reach = 4
    _action_cost = 0.0001
    _safe_radii = 4
    _warn_radii = 4

    # ------------------------------------------------------------------ dims
    @property
    def state_dim(self) -> int:
        return 4

    @property
    def node_dim(self) -> int:
        return 4

    @property
    def edge_dim(self) -> int:
        return 4

    @property
    def action_dim(self) -> int:
        return 2

    @property
    def max_episode_steps(self) -> int:
        return 500 if self._mode == "train" else 2500

    @property
    def default_params(self) -> dict:
        # reference gcbf/env/simple_car.py:67-76
        return {
            "m": 1.0,
            "comm_radius": 1.0,
            "car_radius": 0.05,
            "dist2goal": 0.04,
            "speed_limit": 0.8,
            "max_distance": 4.0,
            "area_size": 4.0,
        }

    # -------------------------------------------------------------- dynamics
    def dynamics(self, data: GraphBatch, u) -> Tensor:
        if not torch.is_tensor(u):
            # symbolic/numpy overload for external CBF-QP use (reference
            # gcbf/env/simple_car.py:80-87 with a cvxpy Expression): works
            # with any object supporting "@" (cvxpy Expression, numpy array)
            x = data.states.cpu().detach().numpy()
            A = np.zeros((self.state_dim, self.state_dim))
            A[0, 2] = 1.0
            A[1, 3] = 1.0
            B = np.array([[1, 0], [0, 1], [0, 0], [0, 0]])
            return x @ A.T + u @ B.T
        x = data.states
        return torch.cat([x[:, 2:], u], dim=1)

    # ----------------------------------------------------------------- reset
    def reset(self) -> GraphBatch:
        self._t = 0
        side = self._params["area_size"]
        r = self.agent_radius
        if self._use_device_reset():
            # starts and goals as one B=2 launch (ops/hip/reset_sample.hip)
            pos, goals = device_rejection_sample(
                self.num_agents, 2, side, (4 * r, 4 * r), None, 0.0,
                self.device)
        elif self._mode in ("train", "test", "demo_2"):
            pos = rejection_sample_positions(self.num_agents, 2, side, 4 * r)
            if self._mode == "demo_2":
                goals = self._sample_goals_near(pos, 4 * r)
            else:
                goals = rejection_sample_positions(self.num_agents, 2, side, 4 * r)
        else:
            raise ValueError("Reset environment: unknown type of mode!")
        # no obstacle rows: x = zeros_like(states), no agent_mask
        return self._finish_reset(self._at_rest(pos.to(self.device)),
                                  goals.to(self.device))

    def forward_graph(self, data: GraphBatch, action: Tensor) -> GraphBatch:
        # reference gcbf/env/simple_car.py:178-194 also resets x
        out = super().forward_graph(data, action)
        out.x = torch.zeros_like(out.states)
        return out

    # ---------------------------------------------------------------- limits
    @property
    def state_lim(self) -> Tuple[Tensor, Tensor]:
        self._ensure_plot_limits()
        sl = self._params["speed_limit"]
        low = torch.tensor([self._xy_min[0], self._xy_min[1], -sl, -sl],
                           device=self.device)
        high = torch.tensor([self._xy_max[0], self._xy_max[1], sl, sl],
                            device=self.device)
        return low, high

    # ----------------------------------------------------------------- u_ref
    def u_ref(self, data: GraphBatch) -> Tensor:
        # reference gcbf/env/simple_car.py:270-304
        goal = torch.cat([self._goal, torch.zeros_like(self._goal)], dim=-1)
        states = data.states.reshape(-1, self.num_agents, self.state_dim)
        diff = states - goal

        if self._K is None:
            A = np.array([[0., 0., 1., 0.],
                          [0., 0., 0., 1.],
                          [0., 0., 0., 0.],
                          [0., 0., 0., 0.]]) * self.dt + np.eye(self.state_dim)
            B = np.array([[0., 0.],
                          [0., 0.],
                          [1., 0.],
                          [0., 1.]]) * self.dt
            K_np = lqr(A, B, np.eye(self.state_dim), np.eye(self.action_dim))
            self._K = torch.from_numpy(K_np).type_as(data.states)

        action = -torch.einsum("us,bns->bnu", self._K, diff)
        action = action.reshape(-1, self.action_dim)

        # speed-limit penalty (branch-free: relu gates the over-speed rows,
        # so no data-dependent host sync — reference simple_car.py:296-302)
        states = states.reshape(-1, self.state_dim)
        v = states[:, 2:]
        speed = v.norm(dim=1, keepdim=True)
        penalty = torch.relu(speed - self._params["speed_limit"]) * 50
        v_dir = v / speed.clamp(min=1e-12)
        return action - penalty * v_dir

    def _heading(self, agent_states: Tensor) -> Tensor:
        # velocity direction (reference gcbf/env/simple_car.py:354-365)
        vel = agent_states[..., 2:4]
        return vel / (vel.norm(dim=-1, keepdim=True) + 1e-5)

    # ---------------------------------------------------------------- render
    def render(self, traj=None, return_ax: bool = False, plot_edge: bool = True,
               ax=None):
        import matplotlib.pyplot as plt
        self._ensure_plot_limits()
        return_tuple = True
        if traj is None:
            traj = (self.data,)
            return_tuple = False
        r = self.agent_radius
        gif = []
        for data in traj:
            fig, ax_ = plt.subplots(1, 1, figsize=(10, 10), dpi=80)
            if ax is not None:
                ax_ = ax
            plot_graph(ax_, data, radius=r, color="#FF8C00", with_label=True,
                       plot_edge=plot_edge, alpha=0.8)
            goal_data = GraphBatch(x=self._goal, pos=self._goal[:, :2],
                                   states=self._goal)
            plot_graph(ax_, goal_data, radius=r, color="#3CB371",
                       with_label=True, plot_edge=False, alpha=0.8)
            collision = self.collision_mask(data)
            idx = torch.where(collision)[0].cpu().numpy()
            ax_.text(0., 0.97, f"Collision: {idx}", transform=ax_.transAxes,
                     fontsize=14)
            x_int = self._xy_max[0] - self._xy_min[0]
            y_int = self._xy_max[1] - self._xy_min[1]
            ax_.set_xlim(self._xy_min[0], self._xy_min[0] + max(x_int, y_int))
            ax_.set_ylim(self._xy_min[1], self._xy_min[1] + max(x_int, y_int))
            plt.axis("off")
            if return_ax:
                return ax_
            gif.append(fig_to_rgb_array(fig))
            plt.close(fig)
        return tuple(gif) if return_tuple else gif[0]
