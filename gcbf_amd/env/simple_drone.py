"""SimpleDrone: 3D linear drone dynamics with static point obstacles.

Behavioral equivalent of the reference SimpleDrone (gcbf/env/simple_drone.py):
6D state [x,y,z,vx,vy,vz], 3D action, damped linear dynamics ẋ = Ax + Bu,
LQR reference controller, static obstacles as graph nodes.

Reference quirks reproduced:
* ``reset`` always spawns ``num_agents`` obstacles, ignoring ``num_obs``
  (gcbf/env/simple_drone.py:128-135).
* the unsafe velocity-cone uses [vx/v, vy/v, vz] — vz NOT normalized
  (gcbf/env/simple_drone.py:431-434).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import ops
from ..graph import GraphBatch
from .point_agent import PointAgentEnv
from .utils import lqr, plot_graph_3d, fig_to_rgb_array, \
    rejection_sample_positions, device_rejection_sample


class SimpleDrone(PointAgentEnv):

    pos_dim = 3
    _radius_key = "drone_radius"
    _step_kind = "drone"
    _env_kind = ops.ENV_DRONE
    _action_limit = 10.0
    # reference gcbf/env/simple_drone.py:191-234
    _reward_step = -0.01
    _reward_collision = 1
    _reward_reach = 10
    _action_cost = 0.001
    _safe_radii = 4
    _warn_radii = 4
    _unsafe_diag_radii = 2  # reference quirk (simple_drone.py:423)

    def __init__(self, num_agents: int, device: torch.device, dt: float = 0.03,
                 params: Optional[dict] = None,
                 max_neighbors: Optional[int] = None):
        super().__init__(num_agents, device, dt, params, max_neighbors)
        self._num_obs = self._params["num_obs"]
        self._xyz_min = np.array([0, 0, 0])
        self._xyz_max = np.ones(3) * self._params["area_size"]

    @property
    def state_dim(self) -> int:
        return 6

    @property
    def node_dim(self) -> int:
        return 4

    @property
    def edge_dim(self) -> int:
        return 6

    @property
    def action_dim(self) -> int:
        return 3

    @property
    def max_episode_steps(self) -> int:
        return 500 if self._mode == "train" else 2000

    @property
    def default_params(self) -> dict:
        # reference gcbf/env/simple_drone.py:71-82
        return {
            "area_size": 2.0,
            "speed_limit": 0.6,
            "drone_radius": 0.05,
            "comm_radius": 0.5,
            "dist2goal": 0.02,
            "obs_point_r": 0.05,
            "obs_len_max": 0.5,
            "max_distance": 4.0,
            "num_obs": 4,
        }

    @property
    def _A(self) -> Tensor:
        A = torch.zeros(6, 6, dtype=torch.float, device=self.device)
        A[0, 3] = 1.0
        A[1, 4] = 1.0
        A[2, 5] = 1.0
        A[3, 3] = -1.1
        A[4, 4] = -1.1
        A[5, 5] = -6.0
        return A

    @property
    def _B(self) -> Tensor:
        B = torch.zeros(6, 3, dtype=torch.float, device=self.device)
        B[3, 0] = 1.1
        B[4, 1] = 1.1
        B[5, 2] = 6.0
        return B

    # -------------------------------------------------------------- dynamics
    def dynamics(self, data: GraphBatch, u) -> Tensor:
        # reference gcbf/env/simple_drone.py:103-120
        if not torch.is_tensor(u):
            # symbolic/numpy overload (cvxpy Expression or numpy array)
            A = self._A.cpu().numpy()
            B = self._B.cpu().numpy()
            return data.states.cpu().detach().numpy() @ A.T + u @ B.T
        am = data.agent_mask
        s = data.states
        xdot = s @ self._A.t()
        mask_f = am.to(s.dtype).unsqueeze(1)
        xdot = xdot * mask_f  # obstacles static
        ctrl = torch.zeros_like(xdot)
        if data.agent_index is not None:    # capture-safe integer scatter
            ctrl = ctrl.index_copy(0, data.agent_index, u @ self._B.t())
        else:
            ctrl = ctrl.masked_scatter(
                am.unsqueeze(1).expand(-1, self.state_dim), u @ self._B.t())
        xdot = xdot + ctrl
        if self._freeze_applies(s):
            agent_states = s[am].reshape(-1, self.num_agents, self.state_dim)
            reach = torch.less(
                torch.norm(agent_states[..., :3] - self._goal[..., :3],
                           dim=-1),
                self._params["dist2goal"]).reshape(-1)
            keep = torch.logical_not(reach).to(s.dtype).unsqueeze(1)
            frozen = xdot[am] * keep
            xdot = xdot.masked_scatter(
                am.unsqueeze(1).expand(-1, self.state_dim), frozen)
        return xdot

    # ----------------------------------------------------------------- reset
    def reset(self) -> GraphBatch:
        self._t = 0
        side = self._params["area_size"]
        r = self.agent_radius
        clearance = 2 * r + 2 * self._params["obs_point_r"]
        if self._mode not in ("train", "test"):
            raise NotImplementedError

        # reference quirk: always num_agents obstacles (simple_drone.py:128-135)
        if self._use_device_reset():
            # obstacles from the device RNG; starts and goals as one B=2
            # launch (ops/hip/reset_sample.hip), nothing copied to the host
            obs_pos = torch.rand(self.num_agents, 3, device=self.device) \
                * side
            pos, goals = device_rejection_sample(
                self.num_agents, 3, side, (4 * r, 4 * r), obs_pos,
                clearance, self.device)
        else:
            obs_pos = torch.rand(self.num_agents, 3) * side
            pos = rejection_sample_positions(
                self.num_agents, 3, side, 4 * r,
                avoid=obs_pos, avoid_dist=clearance)
            goals = rejection_sample_positions(
                self.num_agents, 3, side, 4 * r,
                avoid=obs_pos, avoid_dist=clearance)
        self._obs = self._at_rest(obs_pos.to(self.device))
        return self._finish_reset(self._at_rest(pos.to(self.device)),
                                  self._at_rest(goals.to(self.device)))

    def _finish_reset_plot_limits(self, pts):
        pass  # the plot box is the fixed arena, self._xyz_min/_xyz_max

    @property
    def state_lim(self) -> Tuple[Tensor, Tensor]:
        low = torch.tensor([self._xyz_min[0], self._xyz_min[1],
                            self._xyz_min[2], -10, -10, -10],
                           device=self.device)
        high = torch.tensor([self._xyz_max[0], self._xyz_max[1],
                             self._xyz_max[2], 10, 10, 10],
                            device=self.device)
        return low, high

    # ----------------------------------------------------------------- u_ref
    def u_ref(self, data: GraphBatch) -> Tensor:
        # reference gcbf/env/simple_drone.py:349-377
        states = self._agent_rows(data).reshape(
            -1, self.num_agents, self.state_dim)
        diff = states - self._goal

        if self._K is None:
            A = self._A.cpu().numpy() * self.dt + np.eye(self.state_dim)
            B = self._B.cpu().numpy() * self.dt
            K_np = lqr(A, B, np.eye(self.state_dim), np.eye(self.action_dim))
            self._K = torch.from_numpy(K_np).type_as(data.states)

        action = -torch.einsum("us,bns->bnu", self._K, diff)
        action = action.reshape(-1, self.action_dim)

        # branch-free over-speed penalty (reference simple_drone.py:367-375)
        states = states.reshape(-1, self.state_dim)
        v = states[:, 3:]
        speed = v.norm(dim=1, keepdim=True)
        penalty = torch.relu(speed - self._params["speed_limit"]) * 10
        v_dir = v / speed.clamp(min=1e-12)
        return action - penalty * v_dir

    # ----------------------------------------------------------------- masks
    def _heading(self, agent_states: Tensor) -> Tensor:
        vel = agent_states[..., 3:6]
        v = vel.norm(dim=-1, keepdim=True) + 1e-5
        # reference quirk: vz not normalized (simple_drone.py:431-434)
        return torch.cat([vel[..., 0:1] / v, vel[..., 1:2] / v,
                          vel[..., 2:3]], dim=-1)

    def collision_mask(self, data: GraphBatch) -> Tensor:
        if self._mode not in ("train", "test", "demo_2"):
            raise NotImplementedError
        return super().collision_mask(data)

    # ---------------------------------------------------------------- render
    def render(self, traj=None, return_ax: bool = False, plot_edge: bool = True,
               ax=None):
        import matplotlib.pyplot as plt
        return_tuple = True
        if traj is None:
            traj = (self.data,)
            return_tuple = False
        r = self.agent_radius
        gif = []
        for data in traj:
            fig = plt.figure(figsize=(10, 10), dpi=80)
            ax_ = fig.add_subplot(projection="3d")
            plot_graph_3d(ax_, data, radius=r, color="#FF8C00",
                          with_label=True, plot_edge=plot_edge, alpha=0.3)
            goal_data = GraphBatch(x=self._goal, pos=self._goal[:, :3],
                                   states=self._goal)
            plot_graph_3d(ax_, goal_data, radius=r, color="#3CB371",
                          with_label=True, plot_edge=False, alpha=0.3)
            unsafe = self.unsafe_mask(data)
            idx = torch.where(unsafe)[0].cpu().numpy()
            ax_.text2D(0., 0.97, f"Collision: {idx}", transform=ax_.transAxes,
                       fontsize=14)
            ax_.set_xlim(self._xyz_min[0], self._xyz_max[0])
            ax_.set_ylim(self._xyz_min[1], self._xyz_max[1])
            ax_.set_zlim(self._xyz_min[2], self._xyz_max[2])
            ax_.set_aspect("equal")
            if return_ax:
                return ax_
            gif.append(fig_to_rgb_array(fig))
            plt.close(fig)
        return tuple(gif) if return_tuple else gif[0]
