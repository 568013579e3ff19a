"""Op dispatch layer: HIP/CDNA4 kernels on GPU, eager PyTorch on CPU.

Every hot-path op has (a) an eager PyTorch implementation in ``eager.py``
(the numerics oracle, used on CPU and in tests) and (b) a HIP kernel for
gfx950 in ``gcbf_amd/ops/hip`` exposed through the in-tree extension
``gcbf_amd._C``.  On a GPU tensor the HIP path is mandatory: a missing
extension raises instead of silently falling back to eager (so GPU runs
always exercise the native kernels).  Set ``GCBF_AMD_ALLOW_EAGER_GPU=1``
to permit the eager path on GPU (bring-up/debug only).
"""
from __future__ import annotations

import os
from typing import Optional

import torch
from torch import Tensor

from . import eager

_EXT = None
_EXT_ERR: Optional[str] = None


def _load_ext():
    global _EXT, _EXT_ERR
    if _EXT is not None or _EXT_ERR is not None:
        return _EXT
    try:
        from gcbf_amd import _C  # built in-tree by setup.py / __graft_entry__.build()
        _EXT = _C
    except ImportError as e:  # remember why, report on first GPU use
        _EXT_ERR = str(e)
    return _EXT


def hip_available() -> bool:
    return _load_ext() is not None


def _require_ext(opname: str):
    ext = _load_ext()
    if ext is None:
        if os.environ.get("GCBF_AMD_ALLOW_EAGER_GPU") == "1":
            return None
        raise RuntimeError(
            f"gcbf_amd HIP extension is required for {opname} on GPU but could "
            f"not be imported ({_EXT_ERR}). Build it with "
            f"`python setup.py build_ext --inplace` "
            f"(or set GCBF_AMD_ALLOW_EAGER_GPU=1 to allow the slow eager path).")
    return ext


def _csr_ptr(dst: Tensor, num_nodes: int) -> Tensor:
    """CSR segment pointer from a dst-sorted edge list (device op, no host
    sync)."""
    bounds = torch.arange(num_nodes + 1, device=dst.device, dtype=dst.dtype)
    return torch.searchsorted(dst, bounds).to(torch.int32)


# --------------------------------------------------------------------------
# segment attention aggregation (softmax over incoming edges + weighted sum)
# --------------------------------------------------------------------------

class _SegmentAttnAggregate(torch.autograd.Function):
    """Fused scatter-softmax + weighted scatter-sum with analytic VJP.

    forward: a_e = softmax over {e: dst[e]=n} of gate_e;  out_n = sum a_e m_e
    backward: dm_e = a_e * g_{n(e)};  s_e = <m_e, g_{n(e)}>;
              dgate_e = a_e * (s_e - sum_{e' in n} a_e' s_e')
    """

    @staticmethod
    def forward(ctx, msg: Tensor, gate: Tensor, dst: Tensor, num_nodes: int):
        ext = _require_ext("segment_attn_aggregate") if msg.is_cuda else None
        ctx.msg_dtype = msg.dtype
        ctx.gate_dtype = gate.dtype
        if ext is not None and msg.is_cuda:
            # kernel computes fp32 (softmax stability; the op is tiny next to
            # the bf16 GEMMs around it) — upcast bf16 inputs at the boundary
            msg = msg.float()
            ptr = _csr_ptr(dst, num_nodes)
            att, out = ext.segment_attn_fwd(
                msg.contiguous(), gate.reshape(-1).float().contiguous(), ptr)
            att = att.unsqueeze(-1)
            ctx.ptr = ptr
        else:
            att = eager.segment_softmax(gate, dst, num_nodes)
            out = eager.segment_sum(att * msg, dst, num_nodes)
            ctx.ptr = None
        ctx.save_for_backward(msg, att, dst)
        ctx.num_nodes = num_nodes
        return out

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        msg, att, dst = ctx.saved_tensors
        n = ctx.num_nodes
        ext = _EXT
        if ext is not None and msg.is_cuda and ctx.ptr is not None:
            dmsg, dgate = ext.segment_attn_bwd(
                grad_out.float().contiguous(), msg.contiguous(),
                att.reshape(-1).contiguous(), ctx.ptr)
            dgate = dgate.unsqueeze(-1)
            dmsg = dmsg.to(ctx.msg_dtype)
            dgate = dgate.to(ctx.gate_dtype)
        else:
            g = grad_out.index_select(0, dst)            # (E, D)
            dmsg = att * g
            s = (msg * g).sum(dim=1, keepdim=True)       # (E, 1)
            seg = torch.zeros(n, 1, dtype=s.dtype, device=s.device)
            seg = seg.index_add(0, dst, att * s)
            dgate = att * (s - seg.index_select(0, dst))
        return dmsg, dgate, None, None


def segment_attn_aggregate(msg: Tensor, gate: Tensor, dst: Tensor,
                           num_nodes: int) -> Tensor:
    if not msg.is_cuda:
        return eager.segment_attn_aggregate(msg, gate, dst, num_nodes)
    return _SegmentAttnAggregate.apply(msg, gate, dst, num_nodes)


def segment_softmax(gate: Tensor, dst: Tensor, num_nodes: int) -> Tensor:
    return eager.segment_softmax(gate, dst, num_nodes)


class _SegmentMaxHip(torch.autograd.Function):
    """CSR segment max on the HIP kernel (dst-sorted edges)."""

    @staticmethod
    def forward(ctx, values: Tensor, dst: Tensor, num_nodes: int):
        ext = _require_ext("segment_max")
        vdtype = values.dtype
        v32 = values if vdtype == torch.float32 else values.float()
        ptr = _csr_ptr(dst, num_nodes)
        out, argmax = ext.segment_max_fwd(v32.contiguous(), ptr)
        ctx.save_for_backward(argmax)
        ctx.E = values.shape[0]
        ctx.vdtype = vdtype
        return out.to(vdtype)

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        (argmax,) = ctx.saved_tensors
        from gcbf_amd import _C
        dval = _C.segment_max_bwd(grad_out.float().contiguous(), argmax,
                                  ctx.E)
        return dval.to(ctx.vdtype), None, None


class _SegmentMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values: Tensor, dst: Tensor, num_nodes: int):
        # one extra row absorbs sentinel destinations (padded edge lists
        # use dst == num_nodes for invalid entries), as in eager.segment_sum
        out = eager.segment_max(values.detach(), dst, num_nodes + 1)
        # argmax for backward: first edge attaining the max in its segment
        sel = out.index_select(0, dst)
        is_max = (values.detach() == sel)
        # keep only the first maximal edge per (segment, feature)
        order = torch.arange(values.shape[0], device=values.device)
        big = values.shape[0] + 1
        cand = torch.where(is_max, order.unsqueeze(1), torch.full_like(
            is_max, big, dtype=torch.long))
        first = torch.full((num_nodes + 1, values.shape[1]), big,
                           dtype=torch.long, device=values.device)
        first = first.scatter_reduce(0, dst.unsqueeze(1).expand_as(cand), cand,
                                     reduce="amin", include_self=True)
        ctx.save_for_backward(dst, first[:num_nodes])
        ctx.E = values.shape[0]
        return out[:num_nodes]

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        dst, first = ctx.saved_tensors
        E = ctx.E
        dval = torch.zeros(E + 1, grad_out.shape[1], dtype=grad_out.dtype,
                           device=grad_out.device)
        idx = torch.clamp(first, max=E)
        dval.scatter_add_(0, idx, grad_out)
        return dval[:E], None, None


def segment_max(values: Tensor, dst: Tensor, num_nodes: int) -> Tensor:
    if values.is_cuda and _load_ext() is not None:
        return _SegmentMaxHip.apply(values, dst, num_nodes)
    return _SegmentMax.apply(values, dst, num_nodes)


# --------------------------------------------------------------------------
# graph construction
# --------------------------------------------------------------------------

def dense_radius_graph(pos: Tensor, agent_mask: Optional[Tensor],
                       comm_radius: float,
                       max_neighbors: Optional[int] = None,
                       batch: int = 1) -> Tensor:
    """Edge list only (eager helper; GPU paths use :func:`build_graph`)."""
    return eager.dense_radius_graph(pos, agent_mask, comm_radius,
                                    max_neighbors, batch)


# edge_attr kinds understood by the fused builder (mirrors graph_build.hip)
ATTR_DIFF = 0    # states[src] - states[dst]
ATTR_DUBINS = 1  # [x, y, theta, v cos, v sin] difference


def build_graph(pos: Tensor, states: Tensor, n_rec: Optional[int],
                comm_radius: float, max_neighbors: Optional[int],
                batch: int, attr_kind: int, attr_dim: int,
                eager_attr_fn) -> tuple:
    """Fused radius-graph + edge_attr construction.

    ``n_rec`` is the number of receiver (agent) nodes per graph — agents are
    the first ``n_rec`` rows of each graph; ``None`` means every node
    receives.  GPU: one count/scan/fill kernel pair writing edge_index and
    edge_attr in a single pass.  CPU: eager builder + the env's edge_attr
    function.  Returns (edge_index (2,E) long, edge_attr (E, attr_dim)).
    """
    N = pos.shape[0] // batch
    if n_rec is None:
        n_rec = N
    if pos.is_cuda:
        ext = _require_ext("build_graph")
        if ext is not None:
            topk = -1 if max_neighbors is None else int(max_neighbors)
            ei, ea = ext.build_graph(
                pos.contiguous(), states.contiguous(), batch, n_rec,
                float(comm_radius), topk, int(attr_kind), int(attr_dim))
            return ei, ea
    am = None
    if n_rec != N:
        am = torch.zeros(batch, N, dtype=torch.bool, device=pos.device)
        am[:, :n_rec] = True
        am = am.view(-1)
    ei = eager.dense_radius_graph(pos, am, comm_radius, max_neighbors, batch)
    return ei, eager_attr_fn(states, ei)


def env_step_fused(kind: str, *args, out=None):
    """Fused single-graph rollout step (env_step.hip); None on CPU/no-ext.

    kind: "dubins" | "car" | "drone"; args are forwarded to the binding.
    Returns (new_states, u_ref_next, reward, reach, collision).  ``out``
    optionally provides those five output buffers (ping-pong capture: the
    kernel writes the next phase's inputs directly).
    """
    states = args[0]
    if not states.is_cuda:
        return None
    ext = _require_ext(f"{kind}_step")
    if ext is None:
        return None
    fn = {"dubins": ext.dubins_step, "car": ext.car_step,
          "drone": ext.drone_step}[kind]
    return fn(*[a.contiguous() if torch.is_tensor(a) else a for a in args],
              out=out)


def env_step_batched(kind: str, states: Tensor, goal: Tensor, action: Tensor,
                     active: Tensor, *rest, out=None):
    """Step ``B`` scenes of identical shape in one launch
    (env_step_batched.hip; semantics in :func:`eager.env_step_batched`).

    kind: "dubins" | "car" | "drone"; ``states`` (B, N, S), ``goal``
    (B, n, G), ``action`` (B, n, A), ``active`` (B,) int32; ``rest`` is
    ``[K,] dt, r, sl, d2g, act_lim`` (one LQR gain ``K`` shared by all
    scenes, "car" and "drone" only).  Returns (new_states, u_ref_next,
    reward, reach, collision, reach_all); ``out`` optionally provides those
    six buffers.  GPU tensors run the HIP kernel, CPU tensors the eager
    oracle.
    """
    if states.is_cuda:
        ext = _require_ext(f"{kind}_step_batched")
        if ext is not None:
            fn = {"dubins": ext.dubins_step_batched,
                  "car": ext.car_step_batched,
                  "drone": ext.drone_step_batched}[kind]
            args = (states, goal, action, active) + rest
            return fn(*[a.contiguous() if torch.is_tensor(a) else a
                        for a in args], out=out)
    res = eager.env_step_batched(kind, states, goal, action, active, *rest)
    if out is not None:
        for buf, val in zip(out, res):
            buf.copy_(val)
        return list(out)
    return list(res)


# env kinds understood by the fused mask kernel (mirrors masks.hip)
ENV_CAR = 0
ENV_DUBINS = 1
ENV_DRONE = 2

_WHICH = {"safe": 0, "unsafe": 1, "collision": 2}


def fused_masks(states: Tensor, batch: int, n_rec: int, radius: float,
                env_kind: int, which: str) -> Optional[Tensor]:
    """One-pass batched agent mask on GPU; returns None on CPU (callers fall
    back to the eager vectorized math)."""
    if not states.is_cuda:
        return None
    ext = _require_ext("fused_masks")
    if ext is None:
        return None
    idx = _WHICH[which]
    res = ext.fused_masks(states.contiguous(), batch, n_rec, float(radius),
                          env_kind, idx == 0, idx == 1, idx == 2)
    return res[idx]


# --------------------------------------------------------------------------
# rollout tail: mask -> env step -> padded graph rebuild -> flags, one launch
# --------------------------------------------------------------------------

_TAIL_KIND = {"car": ENV_CAR, "dubins": ENV_DUBINS, "drone": ENV_DRONE}


def rollout_tail_supported(n_rec: int, num_nodes: int) -> bool:
    """True where the extension is built and the scene fits the single
    workgroup of rollout_tail.hip (bound in docs/KERNELS.md)."""
    ext = _load_ext()
    if ext is None or not hasattr(ext, "rollout_tail"):
        return False
    max_rows, max_nodes = ext.rollout_tail_bounds()
    return 1 <= n_rec <= max_rows and num_nodes <= max_nodes


def rollout_tail(step_args, n_rec: int, comm_radius: float, attr_kind: int,
                 attr_dim: int, E_max: int, out, threads: int = 1024,
                 topk: int = -1) -> None:
    """Everything a captured rollout step does after the actor, in one
    launch (rollout_tail.hip), bit-equal to the kernel sequence

        fused_masks(states, 1, n_rec, r, kind, "unsafe").any()
        env_step_fused(*step_args)
        _C.build_graph_padded(new_states[:, :pos_dim], new_states, 1, n_rec,
                              comm_radius, topk, attr_kind, attr_dim, E_max)
        reach.all()

    ``topk`` caps every receiver at its k nearest senders, ties at the k-th
    distance kept (the env's ``max_neighbors``); -1 is no cap.

    ``step_args`` is ``env.fused_step_args(...)``.  ``out`` is [new_states,
    u_ref_next, reward, reach, collision, edge_index (2, E_max), seg
    (E_max,), edge_attr (E_max, attr_dim), flags int32 (3,)]; flags receives
    [edge_count, all(reach), unsafe_any].  GPU only: there is no eager twin,
    callers keep the kernel sequence where this op does not apply.
    """
    ext = _require_ext("rollout_tail")
    if ext is None:
        raise RuntimeError("rollout_tail needs the HIP extension")
    kind, states, goal, action, *rest = step_args
    K = rest[0] if torch.is_tensor(rest[0]) else None
    dt, r, sl, d2g, act_lim = rest[-5:]
    ext.rollout_tail(_TAIL_KIND[kind], states.contiguous(), goal.contiguous(),
                     action.contiguous(),
                     None if K is None else K.contiguous(), dt, r, sl,
                     d2g, act_lim, n_rec, float(comm_radius), int(attr_kind),
                     int(attr_dim), int(E_max), list(out), threads,
                     topk=int(topk))


def rollout_tail_batched_supported(B: int, n_rec: int,
                                   num_nodes: int) -> bool:
    """True where the extension is built and ``B`` scenes of ``n_rec``
    receivers and ``num_nodes`` nodes each fit rollout_tail_batched.hip (one
    workgroup per scene; bounds in docs/KERNELS.md)."""
    ext = _load_ext()
    if ext is None or not hasattr(ext, "rollout_tail_batched"):
        return False
    max_b, max_rows, max_nodes = ext.rollout_tail_batched_bounds()
    return (1 <= B <= max_b and 1 <= n_rec <= max_rows
            and num_nodes <= max_nodes)


def rollout_tail_batched(step_args, explore: Tensor, n_rec: int,
                         comm_radius: float, attr_kind: int, attr_dim: int,
                         E_cap: int, out, threads: int = 1024,
                         topk: int = -1) -> None:
    """:func:`rollout_tail` for ``B`` scenes of one static layout, in two
    launches of ``B`` workgroups (rollout_tail_batched.hip).  On ``states``
    (B, N, S), ``goal`` (B, n, G), ``action`` (B, n, A) and ``explore``
    (B,) int32 it is bit-equal to the kernel sequence

        fused_masks(states.view(B*N, S), B, n_rec, r, kind,
                    "unsafe").view(B, n_rec).any(1)
        env_step_batched(kind, states, goal, where(explore, 0, action),
                         active=ones(B), ...)
        _C.build_graph_padded(new_states[..., :pos_dim], new_states, B,
                              n_rec, comm_radius, topk, attr_kind, attr_dim,
                              E_cap)

    ``topk`` caps every receiver at its k nearest senders of its own scene,
    ties at the k-th distance kept (the env's ``max_neighbors``); -1 is no
    cap.  Each row's cap threshold is searched for once, in the first launch,
    and handed to the second.

    ``step_args`` is ``env.fused_step_args(...)`` on the batched tensors.
    ``out`` is [new_states, u_ref_next, reward (B, n), reach, collision,
    edge_index (2, E_cap), seg (E_cap,), edge_attr (E_cap, attr_dim), flags
    int32 (B, 3), e_count int32 (1,)].  The edge list is the one globally
    compacted list of ``build_graph_padded(batch=B)``: global node ids, all
    pads (src = dst = 0, seg = B*N, attr = 0) after all real edges.
    ``flags[b]`` is [scene b's edge count, all(reach[b]), unsafe_any[b]],
    ``e_count`` the total.  GPU only: there is no eager twin, callers keep
    the kernel sequence where this op does not apply.
    """
    ext = _require_ext("rollout_tail_batched")
    if ext is None:
        raise RuntimeError("rollout_tail_batched needs the HIP extension")
    kind, states, goal, action, *rest = step_args
    K = rest[0] if torch.is_tensor(rest[0]) else None
    dt, r, sl, d2g, act_lim = rest[-5:]
    ext.rollout_tail_batched(
        _TAIL_KIND[kind], states, goal, action, explore, K, dt, r, sl, d2g,
        act_lim, n_rec, float(comm_radius), int(attr_kind), int(attr_dim),
        int(E_cap), list(out), threads, topk=int(topk))


# --------------------------------------------------------------------------
# MLP glue: padded bf16 GEMM inputs written directly (mlp_glue.hip)
# --------------------------------------------------------------------------

def _pad_rows(t: Tensor, rows: int) -> Tensor:
    return t if t.shape[0] == rows else torch.cat(
        [t, t.new_zeros(rows - t.shape[0], t.shape[1])])


def edge_inputs_bf16(x: Tensor, edge_index: Tensor, edge_attr: Tensor,
                     rows_padded: int) -> Tensor:
    """bf16 (rows_padded, 2*node_dim+edge_dim): row e is ``[x[dst_e],
    x[src_e], edge_attr[e]]`` rounded to nearest even, rows past the edge
    capacity are zero.  One launch instead of two gathers, two cats, a
    zero-fill and a cast."""
    if x.is_cuda:
        ext = _require_ext("edge_inputs_bf16")
        if ext is not None:
            return ext.edge_inputs_bf16(
                x.contiguous(), edge_index.contiguous(),
                edge_attr.contiguous(), rows_padded)
    src, dst = edge_index[0], edge_index[1]
    rows = torch.cat([x.index_select(0, dst), x.index_select(0, src),
                      edge_attr], dim=1)
    return _pad_rows(rows, rows_padded).bfloat16()


def attn_aggregate_gamma_in(msg: Tensor, gate: Tensor, seg: Tensor,
                            x: Tensor, n_rows: int, num_nodes: int,
                            rows_padded: int) -> Tensor:
    """bf16 (rows_padded, D+node_dim): row r < n_rows is the
    softmax-weighted sum of the messages whose ``seg == r`` followed by
    ``x[r]``; the other rows are zero.  ``msg`` is bf16 with at least
    ``len(seg)`` rows, ``seg`` is dst-sorted with sentinel entries ==
    ``num_nodes`` at the end.  Same fp32 arithmetic as
    :func:`segment_attn_aggregate` (one shared device function)."""
    if msg.is_cuda:
        ext = _require_ext("attn_aggregate_gamma_in")
        if ext is not None:
            return ext.attn_aggregate_gamma_in(
                msg.contiguous(), gate.reshape(-1).contiguous(),
                seg.contiguous(), x.contiguous(), n_rows, num_nodes,
                rows_padded)
    E = seg.shape[0]
    real = seg < num_nodes          # drop the sentinel entries
    aggr = segment_attn_aggregate(
        msg[:E][real].float(),
        gate.reshape(-1)[:E][real].float().unsqueeze(-1), seg[real],
        num_nodes)
    rows = torch.cat([aggr, x], dim=1)[:n_rows]
    return _pad_rows(rows, rows_padded).bfloat16()


def rows_cat_pad_bf16(a: Tensor, b: Tensor, n_rows: int,
                      rows_padded: int) -> Tensor:
    """bf16 (rows_padded, Da+Db): ``[a[r], bf16(b[r])]`` for r < n_rows,
    zero rows after.  ``a`` is bf16, ``b`` fp32."""
    if a.is_cuda:
        ext = _require_ext("rows_cat_pad_bf16")
        if ext is not None:
            return ext.rows_cat_pad_bf16(a.contiguous(), b.contiguous(),
                                         n_rows, rows_padded)
    rows = torch.cat([a[:n_rows], b[:n_rows].bfloat16()], dim=1)
    return _pad_rows(rows, rows_padded)


def segmax_rows_bf16(msg: Tensor, seg: Tensor, row_index_or_n,
                     num_nodes: int, rows_padded: int) -> Tensor:
    """bf16 (rows_padded, D): row r is the element-wise max over the
    messages whose ``seg`` equals row r's node id, 0 for an empty segment;
    rows past the row count are zero.  Row r's node is r for an int
    ``row_index_or_n`` (the first n nodes) or ``row_index_or_n[r]`` for a
    LONG index tensor.  ``msg`` is bf16 with at least ``len(seg)`` rows
    (rows past the real edges may hold anything), ``seg`` is dst-sorted with
    sentinel entries == ``num_nodes`` at the end.  Forward only.  One launch
    (macbf_glue.hip) for the CSR pointer, :func:`segment_max`, its casts,
    the row select and the pad; same comparison as ``seg_max_fwd``."""
    if torch.is_tensor(row_index_or_n):
        idx, n_rows = row_index_or_n, row_index_or_n.shape[0]
    else:
        idx, n_rows = None, int(row_index_or_n)
    if msg.is_cuda:
        ext = _require_ext("segmax_rows_bf16")
        if ext is not None:
            return ext.segmax_rows_bf16(
                msg.contiguous(), seg.contiguous(),
                None if idx is None else idx.contiguous(), n_rows,
                num_nodes, rows_padded)
    E = seg.shape[0]
    real = seg < num_nodes          # drop the sentinel entries
    aggr = segment_max(msg[:E][real].float(), seg[real], num_nodes)
    rows = aggr[:n_rows] if idx is None else aggr.index_select(0, idx)
    return _pad_rows(rows, rows_padded).bfloat16()


# --------------------------------------------------------------------------
# update glue: the same kernels in grad mode, with their backwards.  GPU and
# extension only (callers check ``hip_available``); every backward hands its
# padded bf16 input a gradient that is exactly zero on pad rows.
# --------------------------------------------------------------------------

class _EdgeInputsBf16(torch.autograd.Function):
    """:func:`edge_inputs_bf16` with the gradient of ``edge_attr``:
    ``d_edge_attr[e] = float(dIn[e, 2*node_dim:])``, what the cast, the row
    slice and the cat of the eager composition hand back.  ``x`` takes no
    gradient."""

    @staticmethod
    def forward(ctx, x: Tensor, edge_index: Tensor, edge_attr: Tensor,
                rows_padded: int):
        ctx.dims = (edge_attr.shape[0], x.shape[1], edge_attr.shape[1])
        return _require_ext("edge_inputs_bf16").edge_inputs_bf16(
            x.contiguous(), edge_index.contiguous(), edge_attr.contiguous(),
            rows_padded)

    @staticmethod
    def backward(ctx, d_in: Tensor):
        E, nd, ed = ctx.dims
        return None, None, _EXT.edge_inputs_bwd(d_in.contiguous(), E, nd,
                                                ed), None


def edge_inputs_bf16_grad(x: Tensor, edge_index: Tensor, edge_attr: Tensor,
                          rows_padded: int) -> Tensor:
    return _EdgeInputsBf16.apply(x, edge_index, edge_attr, rows_padded)


class _GateAttnGammaIn(torch.autograd.Function):
    """Gate MLP + segment attention + γ input as ONE autograd node.

    ``msg`` (padded bf16, φ's output) feeds both the gate MLP and the
    weighted sum.  Eagerly the two gradients meet in fp32 at φ's fp32
    output and are rounded to bf16 once; as two nodes on a bf16 tensor
    they would be rounded twice.  So the gate MLP runs here on a detached
    copy with a graph of its own, and backward is: gate gradient (kernel)
    -> that graph's backward (the same GEMMs autograd would run) -> message
    gradient ``bf16(att * g + float(dmsg_gate))`` (kernel).  ``round_prod``
    is for a φ whose eager output was bf16 already (spectral-normed last
    layer): there ``att * g`` was rounded to bf16 before the sum.
    ``params`` are the leaves ``gate_fn`` reads; their gradients are
    returned through this node.  The inner graph is used up by the first
    backward: one backward per forward, no double backward."""

    @staticmethod
    def forward(ctx, msg: Tensor, gate_fn, x: Tensor, seg: Tensor, idx,
                n_rows: int, num_nodes: int, rows_padded: int,
                round_prod: bool, *params):
        ext = _require_ext("attn_gamma_in")
        with torch.enable_grad():
            msg_in = msg.detach().requires_grad_(True)
            gate = gate_fn(msg_in)
        out, att = ext.attn_gamma_in_fwd(
            msg, gate.detach().reshape(-1), seg.contiguous(), x.contiguous(),
            idx, n_rows, num_nodes, rows_padded)
        ctx.save_for_backward(msg, att, seg, *params)
        ctx.idx = idx
        ctx.inner = (msg_in, gate)
        ctx.dims = (n_rows, num_nodes, round_prod)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out: Tensor):
        msg, att, seg, *params = ctx.saved_tensors
        if ctx.inner is None:
            raise RuntimeError(
                "gate_attn_gamma_in supports one backward per forward: the "
                "gate MLP's graph was freed by the first one")
        msg_in, gate = ctx.inner
        ctx.inner = None
        n_rows, num_nodes, round_prod = ctx.dims
        d_out = d_out.contiguous()
        seg = seg.contiguous()
        dgate = _EXT.attn_gamma_in_bwd_gate(d_out, msg, att, seg, ctx.idx,
                                            n_rows, num_nodes)
        wanted = [p for p, need in zip(params, ctx.needs_input_grad[9:])
                  if need]
        grads = torch.autograd.grad(gate, [msg_in] + wanted, dgate)
        dmsg = _EXT.attn_gamma_in_bwd_msg(d_out, att, seg, ctx.idx,
                                          grads[0].contiguous(), n_rows,
                                          num_nodes, round_prod)
        it = iter(grads[1:])
        dparams = [next(it) if need else None
                   for need in ctx.needs_input_grad[9:]]
        return (dmsg, None, None, None, None, None, None, None, None,
                *dparams)


def gate_attn_gamma_in(msg: Tensor, gate_fn, params, x: Tensor, seg: Tensor,
                       idx: Optional[Tensor], n_rows: int, num_nodes: int,
                       rows_padded: int, round_prod: bool = False) -> Tensor:
    """bf16 (rows_padded, D+node_dim) γ input from φ's padded bf16 output:
    ``gate = gate_fn(msg)`` (padded bf16 in and out), softmax over the edges
    of each node, weighted message sum, ``x`` appended.  Row r is node
    ``idx[r]`` (strictly increasing int64), or node r without ``idx``.  In
    grad mode one autograd node (see :class:`_GateAttnGammaIn`)."""
    if torch.is_grad_enabled() and (msg.requires_grad or any(
            p.requires_grad for p in params)):
        return _GateAttnGammaIn.apply(msg, gate_fn, x, seg, idx, n_rows,
                                      num_nodes, rows_padded, round_prod,
                                      *params)
    gate = gate_fn(msg)
    return _require_ext("attn_gamma_in").attn_gamma_in_fwd(
        msg.contiguous(), gate.reshape(-1).contiguous(), seg.contiguous(),
        x.contiguous(), idx, n_rows, num_nodes, rows_padded)[0]


class _RowsCatPadBf16(torch.autograd.Function):
    """:func:`rows_cat_pad_bf16` with the gradient of ``a`` (itself
    ``rows_padded`` rows): the first ``Da`` columns of the real rows, zero
    pad rows.  ``b`` takes none."""

    @staticmethod
    def forward(ctx, a: Tensor, b: Tensor, n_rows: int, rows_padded: int):
        assert a.shape[0] == rows_padded, "a must already be row-padded"
        ctx.dims = (a.shape[1], n_rows)
        return _require_ext("rows_cat_pad_bf16").rows_cat_pad_bf16(
            a.contiguous(), b.contiguous(), n_rows, rows_padded)

    @staticmethod
    def backward(ctx, d_in: Tensor):
        Da, n_rows = ctx.dims
        return _EXT.rows_cat_bwd(d_in.contiguous(), Da, n_rows), None, None, \
            None


def rows_cat_pad_bf16_grad(a: Tensor, b: Tensor, n_rows: int,
                           rows_padded: int) -> Tensor:
    return _RowsCatPadBf16.apply(a, b, n_rows, rows_padded)


# --------------------------------------------------------------------------
# episode reset
# --------------------------------------------------------------------------

def reset_sample(cand: Tensor, min_sep: Tensor, avoid: Optional[Tensor],
                 avoid_dist: float, pts: Tensor, count: Tensor) -> Tensor:
    """Greedy rejection sampling over a pre-drawn candidate stream, ``B``
    independent problems per call (reset_sample.hip; semantics in
    :func:`eager.reset_sample`).

    ``cand`` (B, C, dim) fp32, ``min_sep`` (B,) fp32, ``avoid`` (B, A, dim)
    or (A, dim) shared by all problems or None, ``pts`` (B, n, dim) and
    ``count`` (B,) int32 updated in place (resumable).  Returns ``used``
    (B,) int32, the number of candidates consumed from this pool.  GPU
    tensors run the HIP kernel (one wavefront per problem), CPU tensors the
    eager oracle.
    """
    B, _, dim = cand.shape
    if avoid is None:
        avoid = cand.new_zeros(B, 0, dim)
    elif avoid.dim() == 2:
        avoid = avoid.unsqueeze(0).expand(B, -1, -1)
    if cand.is_cuda:
        ext = _require_ext("reset_sample")
        if ext is not None:
            return ext.reset_sample(
                cand.contiguous(), min_sep.contiguous(), avoid.contiguous(),
                float(avoid_dist), pts, count)
    used, _ = eager.reset_sample(cand, min_sep, avoid, avoid_dist, pts, count)
    return used
