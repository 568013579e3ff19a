"""Graph container for batched multi-agent graphs.

MI355X-native replacement for the reference's ``torch_geometric.data.Data`` /
``Batch`` containers (reference: gcbf/env/base.py uses Data; gcbf/algo/gcbf.py:159
uses Batch.from_data_list).  Design differences:

* Block-diagonal batching is explicit: ``ptr`` holds node offsets per graph and
  ``edge_index`` stores *global* node ids, so a batch of B graphs is one set of
  flat tensors — no Python-level graph lists on the hot path.
* Uniform-topology fast path: every graph produced by one environment instance
  has the same node count N, so batched tensors reshape to (B, N, D) views and
  the O(N^2) mask/graph-construction work runs as single batched kernels
  (the reference loops over ``to_data_list()`` instead,
  e.g. gcbf/env/simple_car.py:313-327).
* Edges are destination-sorted by construction (the dense builders emit them in
  (graph, dst, src) row-major order), so segment reductions over incoming edges
  use a CSR layout with no sort.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
from torch import Tensor

# Tensor fields that are concatenated along the node dimension.
_NODE_FIELDS = ("x", "pos", "states")


class GraphBatch:
    """A (possibly batched) multi-agent graph.

    Fields
    ------
    x          : (N, node_dim)  node features (0 = agent, 1 = obstacle rows)
    pos        : (N, pos_dim)   node positions
    states     : (N, state_dim) node states
    edge_index : (2, E) long    [src; dst] with *global* node ids, dst-sorted
    edge_attr  : (E, edge_dim)  edge features
    agent_mask : (N,) bool or None (None means every node is an agent)
    u_ref      : (num_agents_total, action_dim) or None
    ptr        : (B + 1,) long  node offsets of each graph in the batch
    """

    __slots__ = ("x", "pos", "states", "edge_index", "edge_attr", "agent_mask",
                 "u_ref", "_ptr", "_dst_ptr", "seg_dst", "agents_first_n",
                 "ring_id", "agent_index", "_edge_count", "actor_glue",
                 "update_glue")

    def __init__(
            self,
            x: Tensor,
            pos: Tensor,
            states: Tensor,
            edge_index: Optional[Tensor] = None,
            edge_attr: Optional[Tensor] = None,
            agent_mask: Optional[Tensor] = None,
            u_ref: Optional[Tensor] = None,
            ptr: Optional[Tensor] = None,
    ):
        self.x = x
        self.pos = pos
        self.states = states
        self.edge_index = edge_index
        self.edge_attr = edge_attr
        self.agent_mask = agent_mask
        self.u_ref = u_ref
        # ptr materializes lazily: a host->device copy here would break
        # hipGraph capture (single graphs never need the tensor)
        self._ptr = ptr
        self._dst_ptr = None  # lazy CSR pointer over destinations
        # optional: segment destinations for aggregation when edge buffers
        # are padded to a fixed capacity (pad entries carry a sentinel id
        # past the last node); None means edge_index[1] is used directly
        self.seg_dst = None
        # optional: number of leading agent rows (single graphs lay agents
        # first) — lets models use a static slice instead of boolean-mask
        # indexing, which is data-dependent and not hipGraph-capturable
        self.agents_first_n = None
        # optional: slot id in the update engine's device ring (stamped by
        # Buffer.on_append when the captured update engine is active)
        self.ring_id = None
        self._edge_count = None
        # optional: LONG index tensor of agent rows (uniform batches have a
        # static agent layout) — models prefer it over the boolean
        # agent_mask because integer indexing is hipGraph-capturable
        self.agent_index = None
        # optional: caller's switch for the actor's padded-bf16 glue path
        # (True/False; None lets the controller read GCBF_AMD_ACTOR_GLUE)
        self.actor_glue = None
        # optional: True where the update's eager iteration wants the
        # networks' padded-bf16 chain in either grad mode (GCBF reads
        # GCBF_AMD_UPDATE_GLUE when it is built); None/False: plain forward
        self.update_glue = None

    # ------------------------------------------------------------------ sizes
    @property
    def ptr(self) -> Tensor:
        if self._ptr is None:
            self._ptr = torch.tensor([0, self.states.shape[0]],
                                     dtype=torch.long,
                                     device=self.states.device)
        return self._ptr

    @ptr.setter
    def ptr(self, value):
        self._ptr = value

    @property
    def num_nodes(self) -> int:
        return (self.states if self.states is not None else self.x).shape[0]

    @property
    def num_edges(self) -> int:
        if self.edge_index is None:
            # metadata-only snapshots (ring-backed rollout) carry the count
            return getattr(self, "_edge_count", None) or 0
        return self.edge_index.shape[1]

    @property
    def num_graphs(self) -> int:
        return 1 if self._ptr is None else self._ptr.shape[0] - 1

    @property
    def nodes_per_graph(self) -> int:
        """Node count per graph; valid only for uniform batches."""
        n, b = self.num_nodes, self.num_graphs
        assert n % b == 0, "non-uniform batch"
        return n // b

    @property
    def device(self) -> torch.device:
        return self.states.device

    @property
    def num_agents(self) -> int:
        if self.agent_mask is None:
            return self.num_nodes
        return int(self.agent_mask.sum().item())

    # -------------------------------------------------------------- builders
    def replace(self, **kwargs) -> "GraphBatch":
        """Return a shallow copy with some fields replaced."""
        out = GraphBatch(
            x=kwargs.get("x", self.x),
            pos=kwargs.get("pos", self.pos),
            states=kwargs.get("states", self.states),
            edge_index=kwargs.get("edge_index", self.edge_index),
            edge_attr=kwargs.get("edge_attr", self.edge_attr),
            agent_mask=kwargs.get("agent_mask", self.agent_mask),
            u_ref=kwargs.get("u_ref", self.u_ref),
            ptr=kwargs.get("ptr", self._ptr),
        )
        return out

    def update(self, **kwargs) -> "GraphBatch":
        """In-place field update (mirrors the reference's ``Data.update``)."""
        for k, v in kwargs.items():
            setattr(self, k, v)
            if k == "edge_index":
                self._dst_ptr = None
        return self

    @staticmethod
    def from_list(graphs: Sequence["GraphBatch"]) -> "GraphBatch":
        """Concatenate graphs into one block-diagonal batch.

        Equivalent of ``Batch.from_data_list`` (gcbf/algo/gcbf.py:159).
        """
        assert len(graphs) > 0, "from_list needs at least one graph"
        if len(graphs) == 1:
            # clone edge_attr: callers (GCBF._iter_eager) set
            # requires_grad_ on the batch's edge_attr, which must not leak
            # back into the stored replay-buffer graph
            g = graphs[0]
            out = g.replace(edge_attr=None if g.edge_attr is None
                            else g.edge_attr.clone())
            return out
        device = graphs[0].device
        node_counts = [g.num_nodes for g in graphs]
        offsets = torch.zeros(len(graphs) + 1, dtype=torch.long,
                              device=device)
        offsets[1:] = torch.cumsum(
            torch.tensor(node_counts, dtype=torch.long, device=device), 0)

        x = torch.cat([g.x for g in graphs], dim=0)
        pos = torch.cat([g.pos for g in graphs], dim=0)
        states = torch.cat([g.states for g in graphs], dim=0)
        # edge offsets applied in ONE vectorized add (repeat_interleave of
        # per-graph node offsets over per-graph edge counts) instead of a
        # per-graph loop — the update loop batches ~300 graphs per call
        e_parts = [g.edge_index for g in graphs if g.edge_index is not None]
        if e_parts:
            edge_index = torch.cat(e_parts, dim=1)
            e_counts = torch.tensor(
                [0 if g.edge_index is None else g.edge_index.shape[1]
                 for g in graphs], dtype=torch.long, device=device)
            shift = torch.repeat_interleave(offsets[:-1], e_counts)
            edge_index = edge_index + shift
        else:
            edge_index = torch.zeros(2, 0, dtype=torch.long, device=device)
        ea = [g.edge_attr for g in graphs if g.edge_attr is not None]
        edge_attr = torch.cat(ea, dim=0) if ea else None

        if graphs[0].agent_mask is not None:
            agent_mask = torch.cat([g.agent_mask for g in graphs], dim=0)
        else:
            agent_mask = None
        if graphs[0].u_ref is not None:
            u_ref = torch.cat([g.u_ref for g in graphs], dim=0)
        else:
            u_ref = None
        return GraphBatch(x, pos, states, edge_index, edge_attr, agent_mask,
                          u_ref, offsets)

    def to_list(self) -> List["GraphBatch"]:
        """Split a batch back into per-graph containers (rarely needed; the
        batched mask kernels replace the reference's ``to_data_list`` loops)."""
        out = []
        ei, ea = self.edge_index, self.edge_attr
        if ei is not None:
            dst = ei[1]
            # edges are dst-sorted, hence graph-sorted
            bounds = torch.searchsorted(dst, self.ptr)
        for i in range(self.num_graphs):
            lo, hi = int(self.ptr[i]), int(self.ptr[i + 1])
            g = GraphBatch(
                x=self.x[lo:hi],
                pos=self.pos[lo:hi],
                states=self.states[lo:hi],
                edge_index=None if ei is None else ei[:, bounds[i]:bounds[i + 1]] - lo,
                edge_attr=None if ea is None else ea[bounds[i]:bounds[i + 1]],
                agent_mask=None if self.agent_mask is None else self.agent_mask[lo:hi],
                u_ref=None,
            )
            out.append(g)
        return out

    # ----------------------------------------------------------------- views
    def states_view(self) -> Tensor:
        """(B, N, state_dim) view for uniform batches."""
        return self.states.view(self.num_graphs, self.nodes_per_graph, -1)

    def pos_view(self) -> Tensor:
        return self.pos.view(self.num_graphs, self.nodes_per_graph, -1)

    def agent_mask_view(self) -> Optional[Tensor]:
        if self.agent_mask is None:
            return None
        return self.agent_mask.view(self.num_graphs, self.nodes_per_graph)

    def detach(self) -> "GraphBatch":
        return GraphBatch(
            self.x.detach(), self.pos.detach(), self.states.detach(),
            None if self.edge_index is None else self.edge_index,
            None if self.edge_attr is None else self.edge_attr.detach(),
            self.agent_mask,
            None if self.u_ref is None else self.u_ref.detach(),
            self._ptr)

    def to(self, device) -> "GraphBatch":
        def mv(t):
            return None if t is None else t.to(device)
        return GraphBatch(mv(self.x), mv(self.pos), mv(self.states),
                          mv(self.edge_index), mv(self.edge_attr),
                          mv(self.agent_mask), mv(self.u_ref),
                          mv(self._ptr))
