"""Vectorized training rollouts: B independent scenes per captured step.

``RolloutEngine`` (rollout.py) advances one scene per hipGraph replay, and
at rollout sizes that replay is launch and latency bound.  This engine holds
B scenes of ONE static layout (same node count, same agent rows) as one
block-diagonal batch and advances all of them per replay:

    actor forward over the whole batch (padded, fixed-capacity edge buffers)
    → ops.rollout_tail_batched (rollout_tail_batched.hip): per scene the
      exploration gate, unsafe mask, env step and edge counts, then the
      globally compacted padded graph rebuild; two launches of B workgroups
    → ONE host readback: flags (B, 3) and the total edge count in one tensor

Node ids of scene b are offset by b·N, ``x`` and ``agent_mask`` are repeated
B times, the edge buffers hold ``E_cap = B·n·(N−1)`` entries (full capacity:
no soft capacity, no overflow fallback).  Pads lie after all real edges
(src = dst = 0, seg = B·N), exactly as ``build_graph_padded(batch=B)`` lays
them out, so the CSR consumers' ``searchsorted`` over ``seg`` holds.

Two bodies share the bookkeeping.  The captured one uses the op above.  The
plain one is the kernel sequence the op equals bit for bit

    fused_masks → env_step_batched(where(explore, 0, action)) →
    build_graph_padded(batch=B, topk)

with the eager implementations on CPU; it runs uncaptured, on CPU, with
``GCBF_AMD_VEC_TAIL=0`` and where the op's bounds do not hold.

Episodes end per scene: a finished scene is reset alone between replays
(``env.reset()`` draws one scene, honouring ``device_reset``), its rows are
copied into the current buffer set and one eager ``build_graph_padded``
rebuilds the current edge buffers.  Snapshots wait in per-scene pending
lists; ``flush()`` appends them to ``algo.buffer`` scene by scene, each
scene's steps in time order, so ``Buffer.sample``'s windows of consecutive
graphs stay within one trajectory stream.  The env object serves as the
scene generator: after a reset it holds the scene drawn last.

GCBF on uncapped scenes by default; ``capped=True`` (``train.py --num-envs B
--capture-capped``) also admits MACBF and neighbour-capped scenes, as
``RolloutEngine`` does: the env's ``max_neighbors`` becomes the ``topk`` of
the tail op and of every builder call, the exploration draw honours
``algo.explore_prob``, and MACBF (whose update batches the stored graphs
themselves) gets full-tensor snapshots, never ring slots.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import ops
from .graph import GraphBatch

# sanity bound on the batch's edge capacity (the same figure RolloutEngine
# uses for one scene)
MAX_EDGE_CAPACITY = 262144


def vec_engine_unsupported_reason(env, algo, B: int, capped: bool = False):
    """None where ``VecRolloutEngine(env, algo, B, capped)`` applies, else
    why not.  ``capped`` (opt-in) also admits MACBF and neighbour-capped
    scenes (``max_neighbors``)."""
    from .algo.gcbf import GCBF
    from .algo.macbf import MACBF
    from .env.point_agent import PointAgentEnv
    if B < 1:
        return "needs at least one scene"
    if not isinstance(algo, GCBF) \
            or (isinstance(algo, MACBF) and not capped):
        return "only GCBF collects vectorized (MACBF is out of scope)"
    if not isinstance(env, PointAgentEnv):
        return "needs a point-agent env"
    if env._mode != "train":
        return f"env mode {env._mode!r} is not 'train'"
    if not capped and env._max_neighbors is not None:
        return "neighbour-capped scenes are not supported"
    if env.device.type == "cuda" and not ops.hip_available():
        return "the HIP extension is not built"
    data = env.data if env.data is not None else env.reset()
    n, N = env.num_agents, data.num_nodes
    if B * n * (N - 1) > MAX_EDGE_CAPACITY:
        return (f"edge capacity {B * n * (N - 1)} above "
                f"{MAX_EDGE_CAPACITY}")
    return None


def vec_engine_supported(env, algo, B: int, capped: bool = False) -> bool:
    return vec_engine_unsupported_reason(env, algo, B, capped) is None


class VecRolloutEngine:

    def __init__(self, env, algo, B: int, capped: bool = False):
        reason = vec_engine_unsupported_reason(env, algo, B, capped)
        if reason is not None:
            raise NotImplementedError(f"VecRolloutEngine: {reason}")
        self.env = env
        self.algo = algo
        self.B = B = int(B)
        self.device = dev = env.device
        self.cuda = dev.type == "cuda"
        self.n = n = env.num_agents
        self.pos_dim = env.pos_dim
        self.edge_dim = env.edge_dim

        data = env.data if env.data is not None else env.reset()
        self.N = N = data.num_nodes
        S, A = env.state_dim, env.action_dim
        # full capacity with or without a cap: ties at the k-th distance
        # are all kept, so a capped row can exceed k
        self.E_cap = B * n * (N - 1)
        # neighbour cap of the scenes' graphs (the env's max_neighbors),
        # read once: -1 is no cap
        self.topk = (-1 if env._max_neighbors is None
                     else int(env._max_neighbors))

        # one scene's static content (snapshots share it)
        self.x1 = data.x.clone()
        self.am1 = (None if data.agent_mask is None
                    else data.agent_mask.clone())
        self.n_rec = n if self.am1 is not None else N
        # the batch's
        self.x = self.x1.repeat(B, 1)
        self.agent_mask = None if self.am1 is None else self.am1.repeat(B)
        self.ptr = torch.arange(B + 1, dtype=torch.long, device=dev) * N
        self.agent_index = None
        if self.am1 is not None and B > 1:
            self.agent_index = (
                torch.arange(B, device=dev).unsqueeze(1) * N
                + torch.arange(n, device=dev)).reshape(-1)

        # ping-pong buffer pairs, as in RolloutEngine
        self.states = [torch.zeros(B, N, S, device=dev) for _ in range(2)]
        self.u_ref = [torch.zeros(B, n, A, device=dev) for _ in range(2)]
        self.goal = torch.zeros((B,) + tuple(env._goal.shape), device=dev)
        E = self.E_cap
        self.ei = [torch.zeros(2, E, dtype=torch.long, device=dev)
                   for _ in range(2)]
        self.seg = [torch.full((E,), B * N, dtype=torch.long, device=dev)
                    for _ in range(2)]
        self.ea = [torch.zeros(E, self.edge_dim, device=dev)
                   for _ in range(2)]
        self.cur = 0
        self.zero_action = torch.zeros(B, n, A, device=dev)
        self.ones = torch.ones(B, dtype=torch.int32, device=dev)
        # exploration gate, host-written before every replay
        self.explore = torch.zeros(B, dtype=torch.int32, device=dev)
        self._explore_host = torch.zeros(B, dtype=torch.int32)
        if self.cuda:
            self._explore_host = self._explore_host.pin_memory()
        # flags (B, 3) and the total edge count share one tensor: one
        # readback per step
        self.fe = torch.zeros(3 * B + 1, dtype=torch.int32, device=dev)
        self.flags = self.fe[:3 * B].view(B, 3)
        self.e_count = self.fe[3 * B:]
        # persistent step outputs
        self.reward_buf = torch.zeros(B, n, device=dev)
        self.reach_buf = torch.zeros(B, n, dtype=torch.bool, device=dev)
        self.coll_buf = torch.zeros(B, n, dtype=torch.bool, device=dev)
        self.reach_all_buf = torch.zeros(B, dtype=torch.bool, device=dev)

        # per-scene bookkeeping (host)
        self.t = np.zeros(B, dtype=np.int64)
        self.counts = np.zeros(B, dtype=np.int64)   # edges per scene
        self.E = 0                                  # their sum
        self.pending = [[] for _ in range(B)]
        self.last_explore = np.zeros(B, dtype=bool)

        # first scene: the one the env holds (B=1 then consumes the same
        # random stream as RolloutEngine); the others are drawn in order
        self._store_scene(0, data)
        for b in range(1, B):
            self._store_scene(b, env.reset())

        K = env._get_K_tensor()
        self.K = None if K is None else K.clone().contiguous()

        self._ext = None
        if self.cuda:
            from gcbf_amd import _C
            self._ext = _C
        self._tail = (self.cuda
                      and os.environ.get("GCBF_AMD_VEC_TAIL", "1") != "0"
                      and ops.rollout_tail_batched_supported(
                          B, self.n_rec, N))
        self._glue = os.environ.get("GCBF_AMD_ACTOR_GLUE", "1") != "0"

        self._rebuild_current()
        self.g = None
        if self._tail:
            self._capture()
        # (no ring for MACBF: its update batches the stored graphs
        # themselves, which a metadata-only snapshot does not carry)
        from .algo.macbf import MACBF
        if getattr(algo, "_ring", None) is None \
                and not isinstance(algo, MACBF) \
                and hasattr(algo, "_make_ring") \
                and not getattr(algo, "_ring_tried", True):
            algo._make_ring()

    # ---------------------------------------------------------- scene plumbing
    def _store_scene(self, b: int, data: GraphBatch):
        """Copy the scene the env just drew into rows b of the current set."""
        c = self.cur
        self.states[c][b].copy_(data.states)
        self.goal[b].copy_(self.env._goal)
        self.u_ref[c][b].copy_(self.env.u_ref(data))
        self.t[b] = 0

    def _flat(self, i: int):
        return self.states[i].view(self.B * self.N, -1)

    def _scene_counts(self, dst: torch.Tensor) -> torch.Tensor:
        """Edges per scene of a dst-sorted list (pads carry B·N)."""
        bounds = torch.searchsorted(dst, self.ptr)
        return bounds[1:] - bounds[:-1]

    def _build_padded(self, i: int):
        """Padded edge buffers of set i from its states, the third call of
        the sequence: ``build_graph_padded(batch=B)``, its eager twin on
        CPU.  Returns the per-scene edge counts (device)."""
        B, N, pd = self.B, self.N, self.pos_dim
        flat = self._flat(i)
        if self.cuda:
            self._ext.build_graph_padded(
                flat[:, :pd].contiguous(), flat, B, self.n_rec,
                self.env.params["comm_radius"], self.topk,
                self.env._attr_kind, self.edge_dim, self.E_cap,
                out=[self.ei[i], self.seg[i], self.ea[i], self.e_count])
            return self._scene_counts(self.seg[i])
        ei, ea = ops.build_graph(
            flat[:, :pd], flat, None if self.am1 is None else self.n,
            self.env.params["comm_radius"],
            None if self.topk < 0 else self.topk, B, self.env._attr_kind,
            self.edge_dim, self.env.edge_attr)
        E = ei.shape[1]
        self.ei[i].zero_()
        self.ei[i][:, :E] = ei
        self.seg[i].fill_(B * N)
        self.seg[i][:E] = ei[1]
        self.ea[i].zero_()
        self.ea[i][:E] = ea
        self.e_count.fill_(E)
        return self._scene_counts(self.seg[i])

    def _rebuild_current(self):
        """One eager rebuild of the current edge buffers (construction and
        after resets)."""
        counts = self._build_padded(self.cur)
        self.counts = counts.cpu().numpy().astype(np.int64)
        self.E = int(self.counts.sum())

    def _graph(self, i: int) -> GraphBatch:
        B, n = self.B, self.n
        flat = self._flat(i)
        if self.cuda:
            ei, ea = self.ei[i], self.ea[i]
        else:       # the eager segment ops take no sentinel entries
            ei, ea = self.ei[i][:, :self.E], self.ea[i][:self.E]
        data = GraphBatch(x=self.x, pos=flat[:, :self.pos_dim], states=flat,
                          edge_index=ei, edge_attr=ea,
                          agent_mask=self.agent_mask,
                          u_ref=self.u_ref[i].view(B * n, -1),
                          ptr=None if B == 1 else self.ptr)
        if self.cuda:
            data.seg_dst = self.seg[i]
        if self.am1 is not None:
            if B == 1:
                data.agents_first_n = n
            else:
                data.agent_index = self.agent_index
        data.actor_glue = self._glue
        return data

    # ------------------------------------------------------------------ bodies
    def _action(self, all_explore: bool, i: int):
        if all_explore:
            # every scene explores: the action is zero everywhere and the
            # actor is skipped, as RolloutEngine's exploration graphs do
            return self.zero_action
        return self.algo.actor(self._graph(i)).view(self.B, self.n, -1)

    def _body(self, all_explore: bool, i: int):
        """Captured body: actor, then the two-launch tail."""
        o = 1 - i
        with torch.no_grad():
            action = self._action(all_explore, i)
            ops.rollout_tail_batched(
                self.env.fused_step_args(
                    self.states[i], self.goal, action.contiguous(), self.K),
                self.explore, self.n_rec, self.env.params["comm_radius"],
                self.env._attr_kind, self.edge_dim, self.E_cap,
                out=[self.states[o], self.u_ref[o], self.reward_buf,
                     self.reach_buf, self.coll_buf, self.ei[o], self.seg[o],
                     self.ea[o], self.flags, self.e_count],
                topk=self.topk)

    def _body_plain(self, all_explore: bool, i: int):
        """The sequence the tail op equals, call by call."""
        o = 1 - i
        B, env = self.B, self.env
        with torch.no_grad():
            data = self._graph(i)
            action = self._action(all_explore, i)
            gated = torch.where(self.explore.view(B, 1, 1) != 0,
                                torch.zeros_like(action), action)
            if self.cuda:
                uns = ops.fused_masks(self._flat(i), B, self.n_rec,
                                      env.agent_radius, env._env_kind,
                                      "unsafe")
            else:
                uns = env.unsafe_mask(data)
            unsafe_any = uns.view(B, self.n_rec).any(dim=1)
            ops.env_step_batched(
                *env.batched_step_args(self.states[i], self.goal,
                                       gated.contiguous(), self.ones,
                                       self.K),
                out=[self.states[o], self.u_ref[o], self.reward_buf,
                     self.reach_buf, self.coll_buf, self.reach_all_buf])
            counts = self._build_padded(o)
            self.flags[:, 0] = counts.to(torch.int32)
            self.flags[:, 1] = self.reach_buf.all(dim=1).to(torch.int32)
            self.flags[:, 2] = unsafe_any.to(torch.int32)

    def _capture(self):
        """Four graphs, {all scenes explore: actor skipped; otherwise: actor
        over the whole batch, gate in the kernel} × phase, on one stream
        with no forked branches."""
        saved = [t.clone() for t in (
            self.states[0], self.u_ref[0], self.ei[0], self.seg[0],
            self.ea[0])]
        self.explore.zero_()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for k in range(4):
                self._body(False, k % 2)
            self._body(True, 0)
            self._body(True, 1)
        torch.cuda.current_stream().wait_stream(s)
        self.g = {}
        pool = None
        for all_explore in (False, True):
            for i in (0, 1):
                g = torch.cuda.CUDAGraph()
                if pool is None:
                    with torch.cuda.graph(g):
                        self._body(all_explore, i)
                    pool = g.pool()
                else:
                    with torch.cuda.graph(g, pool=pool):
                        self._body(all_explore, i)
                self.g[(all_explore, i)] = g
        self.cur = 0
        for dst, src in zip((self.states[0], self.u_ref[0], self.ei[0],
                             self.seg[0], self.ea[0]), saved):
            dst.copy_(src)

    # --------------------------------------------------------------- snapshots
    def _snapshots(self, c: int) -> list:
        """One snapshot per scene of the CURRENT set, before the replay
        overwrites it.  Ring-backed: metadata only, B consecutive ring
        slots in at most two copies per tensor."""
        B, N = self.B, self.N
        ring = getattr(self.algo, "_ring", None)
        snaps = []
        # (bound methods are made per access: compare with ==, not identity)
        if ring is not None and self.algo.buffer.on_append == ring.push:
            ids = ring.push_raw_many(self.states[c], self.u_ref[c])
            for b in range(B):
                snap = GraphBatch(x=self.x1, pos=None, states=None,
                                  agent_mask=self.am1)
                snap.ring_id = ids[b]
                snap._edge_count = int(self.counts[b])
                snaps.append(snap)
            return snaps
        off = 0
        for b in range(B):
            cnt = int(self.counts[b])
            st = self.states[c][b].clone()
            snap = GraphBatch(
                x=self.x1, pos=st[:, :self.pos_dim], states=st,
                edge_index=self.ei[c][:, off:off + cnt] - b * N,
                edge_attr=self.ea[c][off:off + cnt].clone(),
                agent_mask=self.am1, u_ref=self.u_ref[c][b].clone())
            if self.am1 is not None:
                snap.agents_first_n = self.n
            snaps.append(snap)
            off += cnt
        return snaps

    # -------------------------------------------------------------------- step
    def step(self, prob: float) -> np.ndarray:
        """One env step of every scene.  Returns the (B,) bool array of the
        scenes that finished; those are reset before returning."""
        B = self.B
        c = self.cur
        snaps = self._snapshots(c)

        # exploration gate: one draw per scene, against the probability
        # algo.step would use (MACBF floors it)
        explore = np.random.rand(B) < self.algo.explore_prob(prob)
        all_explore = bool(explore.all())
        self.last_explore = explore
        self._explore_host.copy_(torch.from_numpy(explore.astype(np.int32)))
        self.explore.copy_(self._explore_host, non_blocking=True)

        if self.g is not None:
            self.g[(all_explore, c)].replay()
        else:
            self._body_plain(all_explore, c)
        self.cur = c = 1 - c

        fe = self.fe.cpu().numpy()      # ONE host readback per step
        flags = fe[:3 * B].reshape(B, 3)
        self.counts = flags[:, 0].astype(np.int64)
        self.E = int(fe[3 * B])

        self.t += 1
        done = (flags[:, 1] != 0) | (self.t >= self.env.max_episode_steps)
        for b in range(B):
            self.pending[b].append((snaps[b], not bool(flags[b, 2])))
        if done.any():
            for b in np.nonzero(done)[0]:
                self._store_scene(int(b), self.env.reset())
            self._rebuild_current()
        return done

    def flush(self) -> int:
        """Append the pending snapshots to ``algo.buffer`` scene by scene,
        each scene's steps in time order.  Returns how many."""
        count = 0
        for b in range(self.B):
            for snap, is_safe in self.pending[b]:
                self.algo.buffer.append(snap, is_safe)
                count += 1
            self.pending[b] = []
        return count
