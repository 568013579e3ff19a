"""MACBF baseline controller (reference gcbf/controller/macbf_controller.py)."""
from __future__ import annotations

import os

import torch
import torch.nn as nn
from torch import Tensor

from ..graph import GraphBatch
from ..nn import MLP, MACBFControllerLayer
from .base import MultiAgentController


class _Seq(nn.Module):
    def __init__(self, layer: nn.Module):
        super().__init__()
        self.module_0 = layer


class MACBFController(MultiAgentController):

    def __init__(self, num_agents: int, node_dim: int, edge_dim: int,
                 phi_dim: int, action_dim: int):
        super().__init__(num_agents=num_agents, node_dim=node_dim,
                         edge_dim=edge_dim, action_dim=action_dim)
        self.net = _Seq(MACBFControllerLayer(
            node_dim=node_dim, edge_dim=edge_dim, output_dim=action_dim,
            phi_dim=phi_dim))
        self.feat_2_action = MLP(in_channels=2 * action_dim,
                                 out_channels=action_dim,
                                 hidden_layers=(512, 128, 32))

    def forward(self, data: GraphBatch) -> Tensor:
        nm = data.agent_mask
        if data.agent_index is not None:
            nm = data.agent_index      # static LONG indices (capture-safe)
        elif data.agents_first_n is not None:
            nm = data.agents_first_n
        if self._glue_applies(data, nm):
            return self._forward_glue(data, nm)
        x = self.net.module_0(data.x, data.edge_attr, data.edge_index,
                              node_mask=nm, seg_dst=data.seg_dst)
        return self.feat_2_action(torch.cat([x, data.u_ref], dim=1))

    # ------------------------------------------------ no-grad glue path
    def _glue_applies(self, data: GraphBatch, nm) -> bool:
        """The padded-bf16 chain (ops/hip/mlp_glue.hip, macbf_glue.hip)
        serves no-grad GPU inference over padded edge buffers (``seg_dst``)
        with a static agent row layout, on the library-GEMM plans
        ``enable_bf16`` sets up.  ``data.actor_glue`` carries the caller's
        switch (the rollout engine reads GCBF_AMD_ACTOR_GLUE when it is
        built); without one the variable is read here."""
        if torch.is_grad_enabled() or data.seg_dst is None \
                or not data.x.is_cuda:
            return False
        glue = data.actor_glue
        if glue is None:
            glue = os.environ.get("GCBF_AMD_ACTOR_GLUE", "1") != "0"
        if not glue:
            return False
        from ..nn import fused
        from ..nn.gnn import _glue_rows
        rows = _glue_rows(data.x, nm)
        if rows is None:
            return False
        n_rows = rows[0]
        f2a = self.feat_2_action
        return (data.x.dtype == torch.float32
                and data.edge_attr.dtype == torch.float32
                and data.u_ref is not None
                and data.u_ref.dtype == torch.float32
                and data.u_ref.shape[0] == n_rows
                and f2a.fused_mfma
                and fused.plan_is_plain(
                    f2a._plan, -(-n_rows // f2a.BUCKET) * f2a.BUCKET)
                and self.net.module_0.glue_applies(
                    data.x, data.edge_index, nm))

    def _forward_glue(self, data: GraphBatch, nm) -> Tensor:
        """10 GEMMs, their activations, 3 glue kernels and 1 cast; bit-equal
        to :meth:`forward`'s eager composition (tests/test_macbf_glue.py)."""
        from .. import ops
        from ..nn import fused
        from ..nn.gnn import _glue_rows
        n_rows = _glue_rows(data.x, nm)[0]
        feat = self.net.module_0.forward_padded_bf16(
            data.x, data.edge_attr, data.edge_index, nm, data.seg_dst)
        out = fused.run_plan_padded_bf16(
            self.feat_2_action._plan,
            ops.rows_cat_pad_bf16(feat, data.u_ref, n_rows, feat.shape[0]))
        return out[:n_rows].float()
