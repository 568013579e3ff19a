"""MACBF baseline algorithm (reference gcbf/algo/macbf.py:20-239).

Pairwise edge CBF (``CBFNet``) + max-aggregation controller; losses share the
GCBF structure but operate on per-edge h with edge masks, and the ḣ loss uses
only the fixed-topology path (no re-link residue).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
import torch.nn as nn
from torch import Tensor
from torch.optim import Adam

from ..controller import MACBFController
from ..env import MultiAgentEnv
from ..graph import GraphBatch
from ..nn import CBFNetLayer
from .buffer import Buffer
from .gcbf import GCBF, _Seq, cbf_losses


class CBFNet(nn.Module):
    """Per-edge CBF values (reference gcbf/algo/macbf.py:20-48)."""

    def __init__(self, num_agents: int, node_dim: int, edge_dim: int):
        super().__init__()
        self._num_agents = num_agents
        self._top_k = 12
        self.net = _Seq(CBFNetLayer(node_dim=node_dim, edge_dim=edge_dim,
                                    output_dim=1))

    def forward(self, data: GraphBatch) -> Tensor:
        return self.net.module_0(data.x, data.edge_attr, data.edge_index)


class MACBF(GCBF):

    def __init__(self, env: MultiAgentEnv, num_agents: int, node_dim: int,
                 edge_dim: int, action_dim: int, device: torch.device,
                 batch_size: int = 500, params: Optional[dict] = None):
        super().__init__(env=env, num_agents=num_agents, node_dim=node_dim,
                         edge_dim=edge_dim, action_dim=action_dim,
                         device=device, batch_size=batch_size, params=params)
        # replace the GCBF networks with the MACBF ones
        self.cbf = CBFNet(num_agents=num_agents, node_dim=node_dim,
                          edge_dim=edge_dim).to(device)
        self.actor = MACBFController(num_agents=num_agents, node_dim=node_dim,
                                     edge_dim=edge_dim, phi_dim=128,
                                     action_dim=action_dim).to(device)
        self.optim_cbf = Adam(self.cbf.parameters(), lr=3e-4)
        self.optim_actor = Adam(self.actor.parameters(), lr=1e-3)
        self.buffer = Buffer()
        self.memory = Buffer()

    def explore_prob(self, prob: float) -> float:
        # the floor :meth:`step` applies (reference macbf.py:109)
        return max(prob, 0.5)

    @torch.no_grad()
    def step(self, data: GraphBatch, prob: float) -> Tensor:
        # exploration probability floored at 0.5 (reference macbf.py:109)
        action = self.actor(data)
        prob = max(prob, 0.5)
        if np.random.rand() < prob:
            action = torch.zeros_like(action)
        is_safe = torch.logical_not(torch.any(self._env.unsafe_mask(data)))
        self.buffer.append(data, is_safe)
        return action

    def update(self, step: int, writer=None) -> dict:
        inner_iter = self.params["inner_iter"]
        logs = []

        for i_inner in range(inner_iter):
            graphs = GraphBatch.from_list(self._sample_batch())
            graphs.edge_attr.requires_grad_(True)
            h = self.cbf(graphs)
            actions = self.actor(graphs)
            # per-edge h and masks (reference macbf.py:144, 156)
            unsafe_mask = self._env.unsafe_mask(graphs, return_edge=True)
            safe_mask = self._env.safe_mask(graphs, return_edge=True)

            # ḣ on the fixed topology only (reference macbf.py:168-173)
            graphs_next = self._env.forward_graph(graphs, actions)
            h_next = self.cbf(graphs_next)

            loss, log7 = cbf_losses(
                h, lambda: (h_next - h) / self._env.dt, actions,
                unsafe_mask, safe_mask, self.params)
            self._zero_grad()
            loss.backward()
            self._optimizer_step()
            logs.append(log7)

        return self._update_tail(step, writer, logs, inner_iter)

    def apply(self, data: GraphBatch, rand: Optional[float] = 0) -> Tensor:
        """Reference MACBF.apply (macbf.py:213-239) runs Adam over a detached
        action tensor whose grad never populates, so the loop observably
        returns the raw actor action (possibly after an early loss==0 break).
        Reproduce the observable behavior directly."""
        with torch.no_grad():
            return self.actor(data)
