"""GCBF: jointly learned graph CBF and GNN policy.

Behavioral equivalent of the reference GCBF algorithm (gcbf/algo/gcbf.py):
CBF GNN + actor GNN, Adam optimizers, replay buffers with balanced
safe/unsafe segment sampling, CBF-condition losses with the ḣ re-link
residue trick, and test-time per-agent action refinement.

MI355X redesign points:
* the ḣ re-link step rebuilds communication links for the whole batch in one
  batched kernel (``env.add_communication_links_batched``) instead of the
  reference's Python loop over ~300 graphs (gcbf/algo/gcbf.py:196-200);
* safety masks run batched (no ``to_data_list`` loops);
* scalar logging is deferred and synced once per update, not per item;
* a ``grad_sync`` hook lets the DP layer all-reduce gradients over
  RCCL/xGMI between backward and the optimizer steps.
"""
from __future__ import annotations

import os
import sys
import time
from typing import Callable, Optional, Union

import numpy as np
import torch
import torch.nn as nn
from torch import Tensor
from torch.optim import Adam

from ..controller import GNNController
from ..env import MultiAgentEnv
from ..graph import GraphBatch
from ..nn import MLP, CBFGNNLayer
from ..nn.fused import sync_bf16_mirrors
from ..nn.mlp import sn_weight_reuse
from ..utils.trace import trace_range
from .base import Algorithm
from .buffer import Buffer


def _masked_mean(viol: Tensor, ok: Tensor, mask: Tensor,
                 weight: Optional[Tensor]):
    """Mean of ``viol`` (a loss) and of ``ok`` (an accuracy) over the rows
    ``mask`` selects, as weighted sums: boolean-mask indexing (h[mask])
    calls nonzero and forces a device→host sync per mask per inner
    iteration; the weighted form is mathematically identical (incl. the
    empty-mask fallbacks of loss 0 / acc 1) and stays on device."""
    w = mask.to(viol.dtype)
    if weight is not None:
        w = w * weight
    c = w.sum()
    c1 = c.clamp(min=1)
    any_ = (c > 0).to(viol.dtype)
    loss = any_ * (viol * w).sum() / c1
    acc = any_ * (ok.to(viol.dtype) * w).sum() / c1 + (1 - any_)
    return loss, acc


def _wmean(x: Tensor, w: Optional[Tensor], w_sum: Optional[Tensor]):
    return torch.mean(x) if w is None else (x * w).sum() / w_sum


def cbf_losses(h: Tensor, h_dot: Union[Tensor, Callable[[], Tensor]],
               actions: Tensor, unsafe: Tensor, safe: Tensor, params: dict,
               weight: Optional[Tensor] = None):
    """The CBF-condition loss of every update path (reference
    gcbf/algo/gcbf.py:167-215).  Returns ``(loss, log7)``; ``log7`` is the
    detached stack loss unsafe, safe, h_dot, action; acc unsafe, safe, h_dot.

    ``h`` [R, 1] and the ``unsafe``/``safe`` masks [R] share their rows
    (agents for GCBF, edges for MACBF); ``actions`` is per agent.  ``h_dot``
    is the caller's: GCBF adds the re-link residue, MACBF does not.  It may
    be a zero-argument callable, evaluated after the mask terms: gradient
    contributions accumulate into ``h`` in the reverse of the order their
    consumers were created, and float addition does not associate, so the
    eager paths keep the order they have always built the graph in.

    ``weight=None`` takes plain means.  ``weight`` [R] (pad rows 0, for the
    captured engine's fixed-capacity batch; needs per-row ``actions``)
    multiplies the mask weights and turns the means into
    ``(x * w).sum() / w.sum()``, exactly equal on the real rows.
    """
    eps, alpha = params["eps"], params["alpha"]
    w_sum = None if weight is None else weight.sum()
    hv = h[:, 0]
    # unsafe region: h < 0; safe region: h > 0
    loss_unsafe, acc_unsafe = _masked_mean(
        torch.relu(hv + eps), hv < 0, unsafe, weight)
    loss_safe, acc_safe = _masked_mean(
        torch.relu(-hv + eps), hv >= 0, safe, weight)

    if callable(h_dot):
        h_dot = h_dot()
    if weight is None:
        hd, ha = h_dot, alpha * h
    else:   # flat rows, to multiply by the per-row weight
        hd, ha = h_dot[:, 0], hv * alpha
    loss_h_dot = _wmean(torch.relu(-hd - ha + eps), weight, w_sum)
    acc_h_dot = _wmean((hd + ha >= 0).to(hd.dtype), weight, w_sum)

    loss_action = _wmean(torch.square(actions).sum(dim=1), weight, w_sum)

    loss = (params["loss_unsafe_coef"] * loss_unsafe +
            params["loss_safe_coef"] * loss_safe +
            params["loss_h_dot_coef"] * loss_h_dot +
            params["loss_action_coef"] * loss_action)
    log7 = torch.stack([
        loss_unsafe.detach(), loss_safe.detach(), loss_h_dot.detach(),
        loss_action.detach(), acc_unsafe.detach(), acc_safe.detach(),
        acc_h_dot.detach()])
    return loss, log7


class _UpdateProf:
    """Wall-clock buckets of one ``update()``; every method is a no-op
    unless GCBF_AMD_UPDATE_PROF=1."""

    def __init__(self, device: torch.device):
        self.on = os.environ.get("GCBF_AMD_UPDATE_PROF") == "1"
        self.cuda = device.type == "cuda"
        self.buckets = dict.fromkeys(("sample", "batch", "fwd", "mask",
                                      "hdot", "bwd", "opt", "engine"), 0.0)
        self.t0 = 0.0

    def _now(self) -> float:
        if self.cuda:
            torch.cuda.synchronize()
        return time.perf_counter()

    def start(self):
        if self.on:
            self.t0 = self._now()

    def lap(self, name: str):
        """Charge the time since the last start/lap to bucket ``name``."""
        if self.on:
            t1 = self._now()
            self.buckets[name] += t1 - self.t0
            self.t0 = t1

    def report(self):
        if self.on:
            print("# update prof: " + " ".join(
                f"{k}={v * 1000:.1f}ms" for k, v in self.buckets.items()),
                file=sys.stderr, flush=True)


class _Seq(nn.Module):
    """Name-compat container mirroring PyG ``Sequential``'s ``module_0``."""

    def __init__(self, layer: nn.Module):
        super().__init__()
        self.module_0 = layer


class CBFGNN(nn.Module):
    """CBF value network h(x) per agent (reference gcbf/algo/gcbf.py:21-61)."""

    def __init__(self, num_agents: int, node_dim: int, edge_dim: int,
                 phi_dim: int):
        super().__init__()
        self.num_agents = num_agents
        self.feat_transformer = _Seq(CBFGNNLayer(
            node_dim=node_dim, edge_dim=edge_dim, output_dim=1024,
            phi_dim=phi_dim))
        self.feat_2_CBF = MLP(in_channels=1024, out_channels=1,
                              hidden_layers=(512, 128, 32),
                              output_activation=nn.Tanh())

    def forward(self, data: GraphBatch) -> Tensor:
        nm = data.agent_mask
        if data.agent_index is not None:
            nm = data.agent_index      # static LONG indices (capture-safe)
        elif data.agents_first_n is not None:
            nm = data.agents_first_n
        layer = self.feat_transformer.module_0
        if data.update_glue and self._update_glue_applies(data, nm):
            # the update's padded-bf16 chain: the same GEMMs on the same
            # operand values, glue kernels between them, either grad mode
            # (tests/test_update_glue.py).  γ's pad rows reach feat_2_CBF
            # unzeroed: GEMM rows are independent, and the slice's backward
            # supplies the zero pad-row gradient the chain needs.
            from ..nn import fused
            from ..nn.gnn import _glue_rows
            feat = layer.forward_padded_bf16_train(
                data.x, data.edge_attr, data.edge_index, nm, data.seg_dst)
            out = fused.run_plan_padded_bf16_train(self.feat_2_CBF._plan,
                                                   feat)
            return out[:_glue_rows(data.x, nm)[0]].float()
        x = layer(data.x, data.edge_attr, data.edge_index,
                  node_mask=nm, seg_dst=data.seg_dst)
        return self.feat_2_CBF(x)

    def _update_glue_applies(self, data: GraphBatch, nm) -> bool:
        from ..nn import fused
        from ..nn.gnn import _glue_rows
        rows = _glue_rows(data.x, nm)
        f2c = self.feat_2_CBF
        return (rows is not None
                and self.feat_transformer.module_0.update_glue_applies(
                    data.x, data.edge_attr, data.edge_index, nm)
                and f2c.fused_mfma
                and fused.plan_on_library(
                    f2c._plan, -(-rows[0] // f2c.BUCKET) * f2c.BUCKET))

    def attention(self, data: GraphBatch) -> Tensor:
        return self.feat_transformer.module_0.attention(data)


class GCBF(Algorithm):

    def __init__(self, env: MultiAgentEnv, num_agents: int, node_dim: int,
                 edge_dim: int, action_dim: int, device: torch.device,
                 batch_size: int = 500, params: Optional[dict] = None):
        super().__init__(env=env, num_agents=num_agents, node_dim=node_dim,
                         edge_dim=edge_dim, action_dim=action_dim,
                         device=device)
        self.cbf = CBFGNN(num_agents=num_agents, node_dim=node_dim,
                          edge_dim=edge_dim, phi_dim=256).to(device)
        self.actor = GNNController(num_agents=num_agents, node_dim=node_dim,
                                   edge_dim=edge_dim, phi_dim=256,
                                   action_dim=action_dim).to(device)

        # fused multi-tensor Adam on GPU: one kernel per step instead of a
        # foreach chain (~10 launches/step measured in rocprof r02);
        # numerics identical (fp32 master weights)
        fused = (device.type == "cuda"
                 and os.environ.get("GCBF_AMD_FUSED_ADAM", "1") == "1")
        try:
            self.optim_cbf = Adam(self.cbf.parameters(), lr=3e-4,
                                  fused=fused)
            self.optim_actor = Adam(self.actor.parameters(), lr=1e-3,
                                    fused=fused)
        except (RuntimeError, ValueError):
            self.optim_cbf = Adam(self.cbf.parameters(), lr=3e-4)
            self.optim_actor = Adam(self.actor.parameters(), lr=1e-3)

        self.buffer = Buffer()   # current-episode buffer
        self.memory = Buffer()   # replay memory
        self.batch_size = batch_size

        if params is None:
            params = {  # defaults (reference gcbf/algo/gcbf.py:112-120)
                "alpha": 1.0,
                "eps": 0.02,
                "inner_iter": 10,
                "loss_action_coef": 0.001,
                "loss_unsafe_coef": 1.0,
                "loss_safe_coef": 1.0,
                "loss_h_dot_coef": 0.1,
            }
        self.params = params

        # DP hook: called after backward, before the optimizer steps
        self.grad_sync: Optional[Callable[[], None]] = None

        # eager inner iterations run the networks' padded-bf16 glue chain
        # (ops/hip/mlp_glue.hip); 0 keeps the plain forwards.  Read once
        # here and carried on the batches _iter_eager creates.
        self._update_glue = (
            os.environ.get("GCBF_AMD_UPDATE_GLUE", "1") != "0")
        self._agent_index_cache = {}

        # device ring of replayed states (fast batched re-batching for the
        # eager update path; also backs the captured update engine)
        self._ring = None
        self._ring_tried = False
        # hipGraph-captured update engine (created lazily at first update
        # when supported); None -> eager inner iterations
        self._upd_engine = None
        self._upd_engine_tried = False

    # ---------------------------------------------------------------- acting
    @torch.no_grad()
    def act(self, data: GraphBatch) -> Tensor:
        return self.actor(data)

    @torch.no_grad()
    def step(self, data: GraphBatch, prob: float) -> Tensor:
        action = self.actor(data)
        if np.random.rand() < prob:
            action = torch.zeros_like(action)
        # is_safe stays a device tensor; the buffer classifies lazily in one
        # batched transfer (no per-step host sync)
        is_safe = torch.logical_not(torch.any(self._env.unsafe_mask(data)))
        self.buffer.append(data, is_safe)
        return action

    def is_update(self, step: int) -> bool:
        return step % self.batch_size == 0

    # -------------------------------------------------------------- training
    def _make_ring(self):
        """Device ring + batched exact rebuild for sampled batches (replaces
        per-graph Python concatenation in the update; see gcbf_amd/ring.py).
        """
        self._ring_tried = True
        if os.environ.get("GCBF_AMD_RING", "1") == "0":
            return
        env = self._env
        if (env.data is None
                or getattr(env, "_max_neighbors", None) is not None):
            return
        try:
            from ..ring import RingStore
            ring = RingStore(env, Buffer.MAX_SIZE + 2 * self.batch_size)
            for g in list(self.buffer.data) + list(self.memory.data):
                ring.push(g)
            self.buffer.on_append = ring.push
            self._ring = ring
        except Exception as e:
            import warnings
            warnings.warn(f"ring batcher unavailable ({e})")
            self._ring = None

    def _make_update_engine(self):
        """Try to build the hipGraph-captured update engine (GPU only).

        Opt-in via GCBF_AMD_UPDATE_CAPTURE=1.  r02 status: gradient parity
        vs eager is VALIDATED on hardware (tests/test_gpu_kernels.py
        update-engine tests), but the engine measures SLOWER than the
        improved eager path (0.17-0.18 s vs 0.13-0.14 s per update) —
        its fixed-capacity padding and duplicated actor forward cost more
        GPU time than the launch gaps it saves (docs/ARCHITECTURE.md,
        "Captured update engine: measured decision").  Default stays
        eager on measurement, not correctness."""
        self._upd_engine_tried = True
        if os.environ.get("GCBF_AMD_UPDATE_CAPTURE", "0") != "1":
            return
        if type(self) is not GCBF:
            return
        if self.device.type != "cuda":
            return
        env = self._env
        data = env.data
        # obstacle nodes are supported via the static agent-index layout
        # (agents are the first n rows of every graph); the MACBF
        # neighbor-cap path stays eager
        if (data is None
                or getattr(env, "_max_neighbors", None) is not None):
            return
        try:
            from ..update_engine import UpdateEngine
            self._upd_engine = UpdateEngine(self, env)
        except Exception as e:  # fall back to eager iterations
            import traceback
            import warnings
            if os.environ.get("GCBF_AMD_UPDATE_CAPTURE_DEBUG") == "1":
                traceback.print_exc()
            warnings.warn(f"update capture unavailable ({e}); eager updates")
            self._upd_engine = None

    def _sample_batch(self, seg_len: int = 3) -> list:
        """Segments from the current buffer and the replay memory, balanced
        between safe and unsafe steps once there is a memory."""
        if self.memory.size == 0:
            graph_list = self.buffer.sample(self.batch_size // 5, seg_len)
        else:
            curr = self.buffer.sample(self.batch_size // 10, seg_len, True)
            prev = self.memory.sample(
                self.batch_size // 5 - self.batch_size // 10, seg_len, True)
            graph_list = curr + prev
        if not graph_list:
            # degenerate batch_size (< 10): the reference's balanced
            # quotas (n//2 draws) collapse to zero and it crashes at
            # Batch.from_data_list([]); sample unbalanced instead
            graph_list = self.buffer.sample(
                max(1, self.batch_size // 5), seg_len)
        return graph_list

    def _stamp_glue(self, g: GraphBatch, from_ring: bool = True
                    ) -> GraphBatch:
        """Carry the update-glue switch on a batch ``_iter_eager`` made.  A
        uniform batch with obstacle rows also gets its static agent-row
        index (agents are the first rows of every graph), which the glue
        needs in place of the boolean mask.  Side effect outside the
        networks: with ``agent_index`` set, ``env.forward_graph`` and the
        dynamics take their integer-index branch (``index_select`` /
        ``index_copy``) where they took the boolean-mask one, as they do for
        the captured update engine's batches; same values and gradients.
        Ring batches only: every graph of a ring has ``ring.N`` nodes with
        its ``ring.n`` agents first.  GCBF itself only, subclasses keep the
        plain forwards."""
        if type(self) is not GCBF or not self._update_glue \
                or not g.x.is_cuda \
                or getattr(self._env, "_max_neighbors", None) is not None:
            return g
        g.update_glue = True
        if g.agent_mask is not None and g.agent_index is None \
                and from_ring and self._ring is not None \
                and g.num_nodes % self._ring.N == 0:
            L = g.num_nodes // self._ring.N
            ai = self._agent_index_cache.get(L)
            if ai is None:
                dev = g.x.device
                ai = (torch.arange(L, device=dev).unsqueeze(1) * self._ring.N
                      + torch.arange(self._ring.n, device=dev)).reshape(-1)
                self._agent_index_cache[L] = ai
            g.agent_index = ai
        return g

    def _zero_grad(self):
        self.optim_cbf.zero_grad(set_to_none=True)
        self.optim_actor.zero_grad(set_to_none=True)

    def _optimizer_step(self):
        """Everything between backward and the next forward: DP gradient
        all-reduce, clipping, both Adam steps, bf16 mirror refresh."""
        if self.grad_sync is not None:
            with trace_range("gcbf/grad_allreduce"):
                self.grad_sync()
        with trace_range("gcbf/optim"):
            torch.nn.utils.clip_grad_norm_(self.cbf.parameters(), 1e-3)
            torch.nn.utils.clip_grad_norm_(self.actor.parameters(), 1e-3)
            self.optim_cbf.step()
            self.optim_actor.step()
            # bf16 mirror refresh must follow EVERY step: fused Adam does
            # not bump version counters, so lazy staleness checks miss it,
            # and captured graphs (rollout and the update engine's) read
            # the mirrors by address
            sync_bf16_mirrors(self.cbf)
            sync_bf16_mirrors(self.actor)

    def update(self, step: int, writer=None) -> dict:
        inner_iter = self.params["inner_iter"]
        logs = []  # deferred scalars, synced once at the end
        prof = _UpdateProf(self.device)

        if self._ring is None and not self._ring_tried:
            self._make_ring()
        if self._upd_engine is None and not self._upd_engine_tried:
            self._make_update_engine()

        for i_inner in range(inner_iter):
            prof.start()
            graph_list = self._sample_batch()
            prof.lap("sample")

            log7 = None
            if self._upd_engine is not None:
                log7 = self._upd_engine.try_iter(graph_list)
                if log7 is not None:
                    prof.lap("engine")
            if log7 is None:
                log7 = self._iter_eager(graph_list, prof)
            logs.append(log7)

        prof.report()
        return self._update_tail(step, writer, logs, inner_iter)

    def _iter_eager(self, graph_list, prof=None) -> Tensor:
        """One eager inner iteration (sampled batch -> losses -> backward ->
        optimizer).  Returns the 7-scalar log stack (device tensor)."""
        prof = prof or _UpdateProf(self.device)
        prof.start()

        graphs = None
        if self._ring is not None and self._ring.usable(graph_list):
            try:
                graphs = self._ring.batch(graph_list)
            except Exception:
                # metadata-only snapshots (ring-backed rollout) cannot fall
                # back to from_list — there are no stored tensors to
                # concatenate; fail loudly rather than mix gradients
                if any(g.states is None for g in graph_list):
                    raise
                import warnings
                warnings.warn("ring batch failed; falling back to from_list")
                self._ring = None
        from_ring = graphs is not None
        if graphs is None:
            graphs = GraphBatch.from_list(graph_list)
        graphs.edge_attr.requires_grad_(True)
        self._stamp_glue(graphs, from_ring)
        prof.lap("batch")
        # σ reuse ends before backward: the optimizer step changes the weights
        with sn_weight_reuse():
            with trace_range("gcbf/forward"):
                actions = self.actor(graphs)
                # h and h_next in ONE doubled-batch CBF forward: halves the
                # CBF forward/backward chains vs. the reference's separate
                # calls (gcbf/algo/gcbf.py:161,194) and evaluates both sides
                # of the finite difference under the SAME spectral-norm σ
                graphs_next = self._env.forward_graph(graphs, actions)
                both = self._stamp_glue(
                    GraphBatch.from_list([graphs, graphs_next]), from_ring)
                h_both = self.cbf(both)
                n_ag = h_both.shape[0] // 2
                h, h_next = h_both[:n_ag], h_both[n_ag:]
            prof.lap("fwd")

            unsafe_mask = self._env.unsafe_mask(graphs)
            safe_mask = self._env.safe_mask(graphs)
            prof.lap("mask")

            # ḣ condition with the re-link residue trick
            # (reference gcbf/algo/gcbf.py:191-209): the VALUE reflects the
            # re-linked next graph, the GRADIENT flows through the
            # fixed-topology path.
            with trace_range("gcbf/h_dot"):
                with torch.no_grad():
                    relinked = self._stamp_glue(
                        self._env.add_communication_links_batched(
                            graphs_next.detach()), from_ring)
                    h_next_new_link = self.cbf(relinked)
        prof.lap("hdot")

        def h_dot():
            h_dot = (h_next - h) / self._env.dt
            h_dot_new_link = (h_next_new_link - h) / self._env.dt
            residue = (h_dot_new_link - h_dot).detach()
            return residue + h_dot

        loss, log7 = cbf_losses(h, h_dot, actions, unsafe_mask, safe_mask,
                                self.params)
        self._zero_grad()
        with trace_range("gcbf/backward"):
            loss.backward()
        prof.lap("bwd")
        self._optimizer_step()
        prof.lap("opt")
        return log7

    def _update_tail(self, step, writer, logs, inner_iter) -> dict:
        # one host sync for the whole update's scalars; under DP the stack
        # is mean-reduced across ranks first, so rank-0 TensorBoard curves
        # reflect the GLOBAL batch (one small collective per update, not
        # one per scalar; reference semantics gcbf/algo/gcbf.py:229-237)
        log_stack = torch.stack(logs).detach()
        import torch.distributed as dist
        if dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(log_stack, op=dist.ReduceOp.SUM)
            log_stack /= dist.get_world_size()
        log_vals = log_stack.cpu()
        if writer is not None:
            names = ("loss/unsafe", "loss/safe", "loss/derivative",
                     "loss/action", "acc/unsafe", "acc/safe", "acc/derivative")
            for i_inner in range(inner_iter):
                t = step * inner_iter + i_inner
                for k, name in enumerate(names):
                    writer.add_scalar(name, float(log_vals[i_inner, k]), t)

        # refresh bf16 weight mirrors (captured rollout graphs read them
        # by address; Python is skipped during replay)
        sync_bf16_mirrors(self.actor)
        sync_bf16_mirrors(self.cbf)

        self.memory.merge(self.buffer)
        self.buffer.clear()

        return {
            "acc/safe": float(log_vals[-1, 5]),
            "acc/unsafe": float(log_vals[-1, 4]),
            "acc/derivative": float(log_vals[-1, 6]),
        }

    # ----------------------------------------------------------- checkpoints
    def save(self, save_dir: str):
        os.makedirs(save_dir, exist_ok=True)
        torch.save(self.cbf.state_dict(), os.path.join(save_dir, "cbf.pkl"))
        torch.save(self.actor.state_dict(),
                   os.path.join(save_dir, "actor.pkl"))

    def load(self, load_dir: str):
        assert os.path.exists(load_dir)
        self.cbf.load_state_dict(torch.load(
            os.path.join(load_dir, "cbf.pkl"), map_location=self.device,
            weights_only=True))
        self.actor.load_state_dict(torch.load(
            os.path.join(load_dir, "actor.pkl"), map_location=self.device,
            weights_only=True))

    def extra_state(self) -> dict:
        """Optimizer state for training resume (an addition over the
        reference, stored in a separate file so the checkpoint layout stays
        compatible)."""
        return {
            "optim_cbf": self.optim_cbf.state_dict(),
            "optim_actor": self.optim_actor.state_dict(),
        }

    def load_extra_state(self, state: dict):
        self.optim_cbf.load_state_dict(state["optim_cbf"])
        self.optim_actor.load_state_dict(state["optim_actor"])

    # ------------------------------------------------------------- test time
    def apply(self, data: GraphBatch, rand: Optional[float] = 30) -> Tensor:
        """Test-time refinement (reference gcbf/algo/gcbf.py:260-309):
        agents already satisfying the ḣ condition under the nominal (zero)
        action fall back to it; the rest run up to 30 rounds of per-agent
        Adam descent on the ḣ violation through the frozen CBF, plus
        exploration noise.

        On a scene batch (``data.num_graphs > 1``, inside
        ``SceneBatch.scenes()``) the refinement loss is the sum over graphs
        of the per-graph mean.  Scenes do not interact, so every agent's
        gradient, Adam state and noise scale are the single-scene ones; a
        satisfied or finished scene has an all-false ``val`` row and is left
        alone."""
        lr = 0.1
        n_graphs = data.num_graphs
        # agents of scenes that still run; None: all of them
        live = getattr(self._env, "_live_rows", None) if n_graphs > 1 \
            else None

        def violation(h_dot):
            val_h_dot = torch.relu(-h_dot - self.params["alpha"] * h)
            return val_h_dot if live is None else val_h_dot * live
        h = self.cbf(data).detach()
        action = self.actor(data).detach()
        nominal = torch.zeros_like(action)

        data_next = self._env.forward_graph(data, nominal)
        h_next = self.cbf(data_next)
        h_dot = (h_next - h) / self._env.dt
        max_val_h_dot = violation(h_dot)

        ok = (max_val_h_dot[:, 0] <= 0)
        action = torch.where(ok.unsqueeze(1), nominal, action)

        # Vectorized per-agent Adam (equivalent to the reference's list of
        # per-agent optimizers, gcbf/algo/gcbf.py:275-307: Adam state and
        # step counts advance only for violating agents; gradients keep
        # accumulating for agents that are not stepped).
        action = action.clone().requires_grad_(True)
        exp_avg = torch.zeros_like(action)
        exp_avg_sq = torch.zeros_like(action)
        step_cnt = torch.zeros(action.shape[0], 1, device=action.device)
        grad_buf = torch.zeros_like(action)
        b1, b2, adam_eps = 0.9, 0.999, 1e-8

        i_iter = 0
        max_iter = 30
        while True:
            data_next = self._env.forward_graph(data, action)
            h_next = self.cbf(data_next)
            h_dot = (h_next - h) / self._env.dt
            max_val_h_dot = violation(h_dot)
            if n_graphs == 1:
                loss_h_dot = torch.mean(max_val_h_dot)
            else:
                loss_h_dot = max_val_h_dot.sum() \
                    / (max_val_h_dot.shape[0] // n_graphs)
            if loss_h_dot <= 0 or i_iter > max_iter:
                break
            val = (max_val_h_dot[:, 0] > 0).unsqueeze(1)
            g, = torch.autograd.grad(loss_h_dot, action)
            with torch.no_grad():
                grad_buf = torch.where(val, g, grad_buf + g)
                step_cnt = step_cnt + val
                exp_avg = torch.where(
                    val, b1 * exp_avg + (1 - b1) * grad_buf, exp_avg)
                exp_avg_sq = torch.where(
                    val, b2 * exp_avg_sq + (1 - b2) * grad_buf ** 2,
                    exp_avg_sq)
                bc1 = 1 - b1 ** step_cnt.clamp(min=1)
                bc2 = 1 - b2 ** step_cnt.clamp(min=1)
                upd = (lr / bc1) * exp_avg / (
                    (exp_avg_sq / bc2).sqrt() + adam_eps)
                noise = rand * lr * torch.randn_like(grad_buf) * grad_buf
                action -= torch.where(val, upd + noise,
                                      torch.zeros_like(upd))
            i_iter += 1

        return action.detach()
