"""GNN layers as explicit gather → φ → gate → segment-softmax → Σ → γ pipelines.

MI355X-native equivalents of the reference's PyG ``MessagePassing`` layers
(gcbf/nn/gnn.py:14-135).  Instead of PyG's collect/message/aggregate/update
machinery, each layer is a flat pipeline over dst-sorted edge lists whose
segment ops dispatch to HIP kernels on GPU (gcbf_amd/ops).  Submodule names
(``phi``, ``gamma``, ``aggr_module.gate_nn``) match the reference so
state-dicts are interchangeable.

Structural optimization vs. the reference: the per-node update MLP γ is
row-wise, so when the caller only consumes agent rows (obstacle rows are
masked away right after the layer, gcbf/algo/gcbf.py:52-53), γ runs on the
agent rows only — identical outputs on the rows that are used.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor

from .. import ops
from ..graph import GraphBatch
from .mlp import MLP


class AttentionalAggregation(nn.Module):
    """gate = gate_nn(msg); att = scatter-softmax(gate, dst); out = Σ att·msg.

    Equivalent of PyG ``AttentionalAggregation`` (reference gcbf/nn/gnn.py:17).
    """

    def __init__(self, gate_nn: nn.Module):
        super().__init__()
        self.gate_nn = gate_nn

    def forward(self, msg: Tensor, dst: Tensor, num_nodes: int) -> Tensor:
        gate = self.gate_nn(msg)
        return ops.segment_attn_aggregate(msg, gate, dst, num_nodes)


def _gather_edge_inputs(x: Tensor, edge_attr: Tensor,
                        edge_index: Tensor) -> Tensor:
    """cat[x_i, x_j, edge_attr] per edge, with i=dst (receiver), j=src.

    PyG convention used by the reference (gcbf/nn/gnn.py:30-32): ``x_i`` is the
    target node's features, ``x_j`` the source's.
    """
    src, dst = edge_index[0], edge_index[1]
    return torch.cat([x.index_select(0, dst), x.index_select(0, src),
                      edge_attr], dim=1)


def _glue_rows(x: Tensor, node_mask):
    """(row count, row-index tensor or None) of a static agent-row layout:
    every node (``None``), the first n (``int``) or a LONG index tensor.  A
    boolean mask has no static layout: ``None``."""
    if node_mask is None:
        return x.shape[0], None
    if isinstance(node_mask, int):
        return node_mask, None
    if node_mask.dtype == torch.long and node_mask.dim() == 1:
        return node_mask.shape[0], node_mask
    return None


class _UpdateGlueMixin:
    """Padded-bf16 chain of an attention layer in either grad mode (the
    update's forwards): the GEMMs :meth:`forward` issues, on the same
    operand values, with the movement between them done by the glue kernels
    and their backwards (ops/hip/mlp_glue.hip)."""

    def update_glue_applies(self, x: Tensor, edge_attr: Tensor,
                            edge_index: Tensor, node_mask) -> bool:
        from . import fused
        rows = _glue_rows(x, node_mask)
        if rows is None or not x.is_cuda or not ops.hip_available():
            return False
        n_rows, _ = rows
        E = edge_index.shape[1]
        bucket = MLP.BUCKET
        gate = self.aggr_module.gate_nn
        return (n_rows > 0 and E > 0 and not x.requires_grad
                and x.dtype == torch.float32
                and edge_attr.dtype == torch.float32
                and fused.plan_is_plain(gate._plan, -(-E // bucket) * bucket)
                and all(lin.bias is not None for lin, _ in gate._plan)
                and all(m.fused_mfma and fused.plan_on_library(
                            m._plan, -(-r // bucket) * bucket)
                        for m, r in ((self.phi, E), (self.gamma, n_rows),
                                     (gate, E))))

    def forward_padded_bf16_train(self, x: Tensor, edge_attr: Tensor,
                                  edge_index: Tensor, node_mask,
                                  seg_dst: Optional[Tensor] = None) -> Tensor:
        """γ's output for the rows ``node_mask`` selects, as bf16 rows
        padded to the GEMM bucket.  The caller owes it a gradient that is
        zero on pad rows."""
        from . import fused
        from .mlp import SNLinear
        bucket = MLP.BUCKET
        n_rows, idx = _glue_rows(x, node_mask)
        rows_e = -(-edge_index.shape[1] // bucket) * bucket
        rows_n = -(-n_rows // bucket) * bucket
        msg = fused.run_plan_padded_bf16_train(
            self.phi._plan,
            ops.edge_inputs_bf16_grad(x, edge_index, edge_attr, rows_e))
        gate_plan = self.aggr_module.gate_nn._plan
        gamma_in = ops.gate_attn_gamma_in(
            msg, lambda m: fused.run_plan_padded_bf16_train(gate_plan, m),
            fused.plan_params(gate_plan), x,
            edge_index[1] if seg_dst is None else seg_dst, idx, n_rows,
            x.shape[0], rows_n,
            # φ ending in a spectral-normed layer hands the eager path a
            # bf16 msg, whose two gradients meet in bf16
            round_prod=isinstance(self.phi._plan[-1][0], SNLinear))
        return fused.run_plan_padded_bf16_train(self.gamma._plan, gamma_in)


class CBFGNNLayer(_UpdateGlueMixin, nn.Module):
    """Attention message-passing layer of the CBF GNN.

    Reference: gcbf/nn/gnn.py:14-53.  φ and γ are spectral-normed
    (Lipschitz-limited); the gate MLP is not.
    """

    def __init__(self, node_dim: int, edge_dim: int, output_dim: int,
                 phi_dim: int):
        super().__init__()
        self.phi = MLP(in_channels=2 * node_dim + edge_dim,
                       out_channels=phi_dim, hidden_layers=(2048, 2048),
                       limit_lip=True)
        self.gamma = MLP(in_channels=phi_dim + node_dim,
                         out_channels=output_dim, hidden_layers=(2048, 2048),
                         limit_lip=True)
        self.aggr_module = AttentionalAggregation(
            gate_nn=MLP(in_channels=phi_dim, out_channels=1,
                        hidden_layers=(128, 128), limit_lip=False))

    def forward(self, x: Tensor, edge_attr: Tensor, edge_index: Tensor,
                node_mask: Optional[Tensor] = None,
                seg_dst: Optional[Tensor] = None) -> Tensor:
        num_nodes = x.shape[0]
        msg = self.phi(_gather_edge_inputs(x, edge_attr, edge_index))
        dst = edge_index[1] if seg_dst is None else seg_dst
        aggr = self.aggr_module(msg, dst, num_nodes)
        gamma_in = torch.cat([aggr, x], dim=1)
        if node_mask is not None:
            # int = "first n rows" static slice (capture-safe); tensor =
            # boolean mask (batched graphs)
            gamma_in = (gamma_in[:node_mask] if isinstance(node_mask, int)
                        else gamma_in[node_mask])
        return self.gamma(gamma_in)

    def attention(self, data: GraphBatch) -> Tensor:
        """Per-edge softmax attention weights (for plotting; reference
        gcbf/nn/gnn.py:44-53)."""
        msg = self.phi(_gather_edge_inputs(data.x, data.edge_attr,
                                           data.edge_index))
        gate = self.aggr_module.gate_nn(msg)
        return ops.segment_softmax(gate, data.edge_index[1], data.num_nodes)


class ControllerGNNLayer(_UpdateGlueMixin, nn.Module):
    """Same structure as CBFGNNLayer without spectral norm (reference
    gcbf/nn/gnn.py:56-79)."""

    def __init__(self, node_dim: int, edge_dim: int, output_dim: int,
                 phi_dim: int):
        super().__init__()
        self.phi = MLP(in_channels=2 * node_dim + edge_dim,
                       out_channels=phi_dim, hidden_layers=(2048, 2048))
        self.gamma = MLP(in_channels=phi_dim + node_dim,
                         out_channels=output_dim, hidden_layers=(2048, 2048))
        self.aggr_module = AttentionalAggregation(
            gate_nn=MLP(in_channels=phi_dim, out_channels=1,
                        hidden_layers=(128, 128)))

    def forward(self, x: Tensor, edge_attr: Tensor, edge_index: Tensor,
                node_mask: Optional[Tensor] = None,
                seg_dst: Optional[Tensor] = None) -> Tensor:
        num_nodes = x.shape[0]
        msg = self.phi(_gather_edge_inputs(x, edge_attr, edge_index))
        dst = edge_index[1] if seg_dst is None else seg_dst
        aggr = self.aggr_module(msg, dst, num_nodes)
        gamma_in = torch.cat([aggr, x], dim=1)
        if node_mask is not None:
            gamma_in = (gamma_in[:node_mask] if isinstance(node_mask, int)
                        else gamma_in[node_mask])
        return self.gamma(gamma_in)

    def glue_applies(self, x: Tensor, edge_index: Tensor, n_rows) -> bool:
        """Whether :meth:`forward_padded_bf16` computes this call: no-grad
        GPU inference on the library-GEMM plans with a static row count."""
        from . import fused
        bucket = MLP.BUCKET
        E = edge_index.shape[1]
        return (not torch.is_grad_enabled() and x.is_cuda
                and isinstance(n_rows, int) and n_rows > 0 and E > 0
                and ops.hip_available()
                and all(m.fused_mfma and fused.plan_is_plain(
                            m._plan, -(-rows // bucket) * bucket)
                        for m, rows in ((self.phi, E), (self.gamma, n_rows),
                                        (self.aggr_module.gate_nn, E))))

    def forward_padded_bf16(self, x: Tensor, edge_attr: Tensor,
                            edge_index: Tensor, n_rows: int,
                            seg_dst: Tensor) -> Tensor:
        """No-grad forward that never leaves padded bf16 between the GEMMs:
        returns γ's output for the first ``n_rows`` nodes as bf16 rows
        padded to the GEMM bucket.  Same GEMM calls on the same operand
        values as :meth:`forward`; the gathers, cats, pads, casts, slices
        and the CSR pointer between them are three glue kernels
        (ops/hip/mlp_glue.hip).  φ's pad rows reach the gate MLP unzeroed:
        GEMM rows are independent and the aggregation reads real edges
        only."""
        from . import fused
        bucket = MLP.BUCKET
        rows_e = -(-edge_index.shape[1] // bucket) * bucket
        rows_n = -(-n_rows // bucket) * bucket
        msg = fused.run_plan_padded_bf16(
            self.phi._plan,
            ops.edge_inputs_bf16(x, edge_index, edge_attr, rows_e))
        gate = fused.run_plan_padded_bf16(self.aggr_module.gate_nn._plan, msg)
        gamma_in = ops.attn_aggregate_gamma_in(
            msg, gate, seg_dst, x, n_rows, x.shape[0], rows_n)
        return fused.run_plan_padded_bf16(self.gamma._plan, gamma_in)


class CBFNetLayer(nn.Module):
    """MACBF per-edge CBF: φ output returned per edge, no aggregation
    (reference gcbf/nn/gnn.py:82-111)."""

    def __init__(self, node_dim: int, edge_dim: int, output_dim: int):
        super().__init__()
        self.phi = MLP(in_channels=2 * node_dim + edge_dim,
                       out_channels=output_dim, hidden_layers=(64, 128, 64),
                       limit_lip=False)

    def forward(self, x: Tensor, edge_attr: Tensor,
                edge_index: Tensor) -> Tensor:
        return self.phi(_gather_edge_inputs(x, edge_attr, edge_index))


class MACBFControllerLayer(nn.Module):
    """Max-aggregation message passing (reference gcbf/nn/gnn.py:114-135)."""

    def __init__(self, node_dim: int, edge_dim: int, output_dim: int,
                 phi_dim: int):
        super().__init__()
        self.phi = MLP(in_channels=2 * node_dim + edge_dim,
                       out_channels=phi_dim, hidden_layers=(64,))
        self.gamma = MLP(in_channels=phi_dim, out_channels=output_dim,
                         hidden_layers=(64, 128, 64))

    def forward(self, x: Tensor, edge_attr: Tensor, edge_index: Tensor,
                node_mask=None, seg_dst: Optional[Tensor] = None) -> Tensor:
        num_nodes = x.shape[0]
        msg = self.phi(_gather_edge_inputs(x, edge_attr, edge_index))
        # seg_dst: segment ids of a padded edge list, whose pad entries
        # carry the sentinel id num_nodes and fall outside every segment
        dst = edge_index[1] if seg_dst is None else seg_dst
        aggr = ops.segment_max(msg, dst, num_nodes)
        if node_mask is not None:
            # int = "first n rows" static slice, LONG tensor = static row
            # indices (both capture-safe); boolean mask otherwise
            aggr = (aggr[:node_mask] if isinstance(node_mask, int)
                    else aggr[node_mask])
        return self.gamma(aggr)

    def glue_applies(self, x: Tensor, edge_index: Tensor, node_mask) -> bool:
        """Whether :meth:`forward_padded_bf16` computes this call: no-grad
        GPU inference on the library-GEMM plans with a static row layout."""
        from . import fused
        bucket = MLP.BUCKET
        rows = _glue_rows(x, node_mask)
        E = edge_index.shape[1]
        return (rows is not None and rows[0] > 0 and E > 0
                and not torch.is_grad_enabled() and x.is_cuda
                and ops.hip_available()
                and all(m.fused_mfma and fused.plan_is_plain(
                            m._plan, -(-r // bucket) * bucket)
                        for m, r in ((self.phi, E), (self.gamma, rows[0]))))

    def forward_padded_bf16(self, x: Tensor, edge_attr: Tensor,
                            edge_index: Tensor, node_mask,
                            seg_dst: Tensor) -> Tensor:
        """No-grad forward that never leaves padded bf16 between the GEMMs:
        γ's output for the rows ``node_mask`` selects (every node, the first
        n, or LONG indices) as bf16 rows padded to the GEMM bucket.  Same
        GEMM calls on the same operand values as :meth:`forward`; the
        gathers, cat, pads, casts, CSR pointer, segment max and row select
        between them are two glue kernels (ops/hip/mlp_glue.hip,
        ops/hip/macbf_glue.hip).  φ's pad rows are never read: the segment
        max scans real edges only."""
        from . import fused
        bucket = MLP.BUCKET
        n_rows, idx = _glue_rows(x, node_mask)
        rows_e = -(-edge_index.shape[1] // bucket) * bucket
        rows_n = -(-n_rows // bucket) * bucket
        msg = fused.run_plan_padded_bf16(
            self.phi._plan,
            ops.edge_inputs_bf16(x, edge_index, edge_attr, rows_e))
        gamma_in = ops.segmax_rows_bf16(
            msg, seg_dst, n_rows if idx is None else idx, x.shape[0], rows_n)
        return fused.run_plan_padded_bf16(self.gamma._plan, gamma_in)
