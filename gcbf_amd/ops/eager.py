"""Eager (pure PyTorch) reference implementations of every hot-path op.

These are the golden oracles for the HIP/CDNA4 kernels in ``gcbf_amd/ops/hip``
and the CPU execution path.  Semantics mirror the reference implementation:

* segment softmax / weighted sum  ~ PyG ``AttentionalAggregation``
  (reference: gcbf/nn/gnn.py:17-19 via torch_scatter)
* dense radius graph with optional k-nearest cap
  (reference: gcbf/env/dubins_car.py:730-746, simple_drone.py:316-333)
* batched pairwise masks (reference: gcbf/env/simple_car.py:306-387 et al.,
  which loop over graphs in Python — here they are single batched ops)
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor


# --------------------------------------------------------------------------
# segment (per-destination) reductions over dst-sorted edge lists
# --------------------------------------------------------------------------

def segment_softmax(gate: Tensor, dst: Tensor, num_nodes: int) -> Tensor:
    """Softmax of ``gate`` (E, 1) over edges grouped by destination node.

    Matches ``torch_geometric.utils.softmax`` semantics (numerically stabilized
    by the per-segment max; empty segments produce no outputs).
    """
    gate = gate.squeeze(-1)
    # one extra row absorbs sentinel destinations (padded edge lists use
    # dst == num_nodes for invalid entries)
    seg_max = torch.full((num_nodes + 1,), float("-inf"),
                         dtype=gate.dtype, device=gate.device)
    seg_max = seg_max.scatter_reduce(0, dst, gate.detach(), reduce="amax",
                                     include_self=True)
    shifted = gate - seg_max.index_select(0, dst)
    ex = shifted.exp()
    denom = torch.zeros(num_nodes + 1, dtype=gate.dtype, device=gate.device)
    denom = denom.index_add(0, dst, ex)
    att = ex / (denom.index_select(0, dst) + 1e-16)
    return att.unsqueeze(-1)


def segment_sum(values: Tensor, dst: Tensor, num_nodes: int) -> Tensor:
    """Sum of (E, D) edge values into (num_nodes, D) per destination.
    A sentinel row absorbs dst == num_nodes (padded edge lists)."""
    out = torch.zeros(num_nodes + 1, values.shape[1],
                      dtype=values.dtype, device=values.device)
    return out.index_add(0, dst, values)[:num_nodes]


def segment_attn_aggregate(msg: Tensor, gate: Tensor, dst: Tensor,
                           num_nodes: int) -> Tensor:
    """out[n] = sum_{e: dst[e]=n} softmax_seg(gate)[e] * msg[e].

    The fused attention aggregation (gate softmax + weighted scatter-sum) of
    PyG ``AttentionalAggregation`` (reference gcbf/nn/gnn.py:17-19).
    """
    att = segment_softmax(gate, dst, num_nodes)
    return segment_sum(att * msg, dst, num_nodes)


def segment_max(values: Tensor, dst: Tensor, num_nodes: int) -> Tensor:
    """Per-destination max with 0 for empty segments (torch_scatter
    ``scatter_max`` as used by PyG ``aggr='max'``, reference gcbf/nn/gnn.py:117
    — PyG fills empty segments with 0)."""
    out = torch.full((num_nodes, values.shape[1]), float("-inf"),
                     dtype=values.dtype, device=values.device)
    idx = dst.unsqueeze(-1).expand_as(values)
    out = out.scatter_reduce(0, idx, values, reduce="amax", include_self=True)
    return out.masked_fill(out == float("-inf"), 0.0)


# --------------------------------------------------------------------------
# graph construction
# --------------------------------------------------------------------------

def dense_radius_graph(
        pos: Tensor,
        agent_mask: Optional[Tensor],
        comm_radius: float,
        max_neighbors: Optional[int] = None,
        batch: int = 1,
) -> Tensor:
    """Batched dense radius-graph construction.

    pos: (B*N, pos_dim); agent_mask: (B*N,) bool or None.  Only agent nodes
    receive edges.  Returns global ``edge_index`` (2, E) = [src; dst] sorted by
    (graph, dst, src), matching the reference builder's ``nonzero`` ordering
    (gcbf/env/dubins_car.py:730-746: receivers are the first ``n_agents`` rows
    of each graph, self-edges excluded, optional cap to the ``max_neighbors``
    nearest senders).
    """
    B = batch
    N = pos.shape[0] // B
    p = pos.view(B, N, -1)
    # (B, N, N) pairwise distances dist[b, i, j] = |p_i - p_j| via explicit
    # differences (same rounding as the reference's torch.norm and the HIP
    # kernel; cdist's matmul trick rounds differently at the radius boundary)
    dist = (p.unsqueeze(2) - p.unsqueeze(1)).norm(dim=-1)
    big = comm_radius + 1.0
    eye = torch.eye(N, device=pos.device, dtype=dist.dtype)
    if agent_mask is None:
        n_rec = N
        dist = dist + eye * big
    else:
        am = agent_mask.view(B, N)
        n_rec = int(am[0].sum().item())
        # reference convention: agents are the first n_rec rows of each graph
        dist = dist[:, :n_rec, :]
        # reference adds eye(n_rec) to the first n_rec columns (self-exclusion)
        dist = dist + eye[:n_rec] * big

    if max_neighbors is not None and max_neighbors < dist.shape[-1]:
        # keep only each receiver's k nearest senders (reference uses topk then
        # masks the rest, gcbf/env/dubins_car.py:736-740, but with a Python
        # loop per row — this is the batched equivalent).  Tie semantics
        # differ from torch.topk: EVERY sender tied at the k-th smallest
        # distance is kept (can exceed k on exact float ties — measure-zero
        # in practice); the HIP kth_smallest kernel matches this rule.
        kth = dist.topk(max_neighbors, dim=-1, largest=False).values[..., -1:]
        dist = torch.where(dist <= kth, dist, dist + big)

    mask = dist < comm_radius  # (B, n_rec, N)
    nz = mask.nonzero(as_tuple=False)  # rows (b, i, j) in row-major order
    b, i, j = nz[:, 0], nz[:, 1], nz[:, 2]
    src = b * N + j
    dst = b * N + i
    return torch.stack([src, dst], dim=0)


# --------------------------------------------------------------------------
# episode-reset rejection sampling over a pre-drawn candidate stream
# --------------------------------------------------------------------------

def _sq_dist(points: Tensor, p: Tensor) -> Tensor:
    """fp32 squared distances, accumulated x, y(, z) in order, no sqrt."""
    diff = points - p
    d2 = diff[:, 0] * diff[:, 0]
    for k in range(1, diff.shape[1]):
        d2 = d2 + diff[:, k] * diff[:, k]
    return d2


def reset_sample(cand: Tensor, min_sep: Tensor, avoid: Tensor,
                 avoid_dist: float, pts: Tensor, count: Tensor):
    """Greedy sequential rejection sampling, the oracle of reset_sample.hip.

    For each of the ``B`` problems walk ``cand[b]`` (C, dim) in order while
    ``count[b] < n`` and accept a candidate iff its squared fp32 distance to
    the origin (reference quirk: the host loop tests against a zero-
    initialised buffer) and to every accepted point exceeds ``min_sep[b]²``
    and its squared distance to every ``avoid[b]`` point exceeds
    ``avoid_dist²``.  ``pts`` (B, n, dim) and ``count`` (B,) int32 are
    updated in place, so a short problem can be resumed with a fresh pool.

    Returns ``(used, min_gap)``: ``used`` (B,) int32 is the number of
    candidates consumed from this pool (``C`` when it ran out), ``min_gap``
    the smallest relative gap ``|d2 - thr²| / thr²`` over every comparison
    made — how far the closest decision was from flipping under a different
    fp32 rounding of ``d2``.
    """
    dev = cand.device
    B, C, dim = cand.shape
    n = pts.shape[1]
    cand_c = cand.detach().float().cpu()
    avoid_c = avoid.detach().float().cpu()
    sep_c = min_sep.detach().float().cpu()
    pts_c = pts.detach().cpu().clone()
    count_c = count.detach().cpu().clone()
    used = torch.zeros(B, dtype=torch.int32)
    av = torch.tensor(float(avoid_dist), dtype=torch.float32)
    av2 = av * av
    min_gap = float("inf")
    for b in range(B):
        sep2 = sep_c[b] * sep_c[b]
        # occupied = origin + accepted points
        occ = torch.zeros(n + 1, dim)
        cnt = min(max(int(count_c[b]), 0), n)
        occ[1:cnt + 1] = pts_c[b, :cnt]
        c = 0
        while cnt < n and c < C:
            p = cand_c[b, c]
            c += 1
            d2 = _sq_dist(occ[:cnt + 1], p)
            ok = bool((d2 > sep2).all())
            if float(sep2) > 0:
                min_gap = min(min_gap, float(((d2 - sep2).abs() / sep2).min()))
            if avoid_c.shape[1]:
                d2a = _sq_dist(avoid_c[b], p)
                ok = ok and bool((d2a > av2).all())
                if float(av2) > 0:
                    min_gap = min(min_gap,
                                  float(((d2a - av2).abs() / av2).min()))
            if ok:
                cnt += 1
                occ[cnt] = p
        pts_c[b, :cnt] = occ[1:cnt + 1]
        count_c[b] = cnt
        used[b] = c
    pts.copy_(pts_c.to(dev))
    count.copy_(count_c.to(dev))
    return used.to(dev), min_gap


# --------------------------------------------------------------------------
# batched environment step (oracle of env_step_batched.hip)
# --------------------------------------------------------------------------

def _dubins_u_ref(s: Tensor, g: Tensor, sl: float) -> Tensor:
    """PID reference controller on (..., 4) states and goals."""
    two_pi = 2 * torch.pi
    # op for op the envs' own u_ref (env/dubins_car.py), so that the CPU
    # paths agree to the bit: the heading controller flips sign on a
    # rounding difference and an episode would amplify it
    diff = s - g
    dist = torch.norm(diff[..., :2], dim=-1)
    theta_t = (torch.acos(torch.clamp(-diff[..., 0] / (dist + 1e-4), -1, 1))
               * torch.sign(-diff[..., 1])) % two_pi
    theta = s[..., 2] % two_pi
    td = theta_t - theta
    agent_dir = torch.stack([torch.cos(theta), torch.sin(theta)], dim=-1)
    inner = (-diff[..., :2] * agent_dir).sum(dim=-1)
    between = torch.acos(torch.clamp(inner / (dist + 1e-4), -1, 1))
    anti = (td < torch.pi) & (td >= 0)
    clock = (td > -torch.pi) & (td <= 0)
    one = torch.ones_like(theta)
    sign = torch.where(theta <= torch.pi, torch.where(anti, one, -one),
                       torch.where(clock, -one, one))
    omega = torch.clamp(sign * 0.2 * between, -5.0, 5.0)
    v = s[..., 3]
    a = -0.6 * v + 0.3 * dist
    a = torch.where(v > sl, torch.clamp(a, max=0.0), a)
    a = torch.where(v < -sl, torch.clamp(a, min=0.0), a)
    return torch.stack([omega, a], dim=-1)


def _lqr_u_ref(s: Tensor, goal_full: Tensor, K: Tensor, sl: float,
               vel: slice, gain: float) -> Tensor:
    """-K (x - goal) minus the over-speed penalty, on (..., S) states."""
    u = -torch.einsum("us,...s->...u", K, s - goal_full)
    v = s[..., vel]
    speed = v.norm(dim=-1, keepdim=True)
    penalty = torch.relu(speed - sl) * gain
    return u - penalty * (v / speed.clamp(min=1e-12))


# per kind: position dims, reach / collision / step reward, action cost and
# whether that cost is one sum over the scene's agents
_STEP_CONST = {
    "dubins": (2, 10.0, 0.1, -1e-4, 0.01, True),
    "car": (2, 4.0, 2.0, -0.01, 1e-4, False),
    "drone": (3, 10.0, 1.0, -0.01, 1e-3, False),
}


def env_step_batched(kind: str, states: Tensor, goal: Tensor, action: Tensor,
                     active: Tensor, *rest):
    """Step ``B`` scenes of identical shape at once, fp32, vectorised.

    ``states`` (B, N, S), ``goal`` (B, n, G), ``action`` (B, n, A),
    ``active`` (B,) int32; ``rest`` is ``[K,] dt, r, sl, d2g, act_lim`` with
    the LQR gain ``K`` for "car" and "drone" only.  Returns
    ``(new_states, u_ref_next, reward (B, n), reach (B, n), collision
    (B, n), reach_all (B,))``.  An active scene is stepped as the env's own
    ``step`` does it (agents freeze on reach in "dubins" and "drone",
    obstacles drift or stay, the Dubins action cost sums the scene's own
    agents).  An inactive scene keeps its states bit for bit, reports the
    u_ref and the reach test of that unchanged state, reward 0 and no
    collision.
    """
    if kind == "dubins":
        K = None
        dt, r, sl, d2g, act_lim = rest
    else:
        K, dt, r, sl, d2g, act_lim = rest
    p, reach_rew, coll_rew, step_rew, act_cost, summed = _STEP_CONST[kind]
    B, N, S = states.shape
    n = action.shape[1]
    on = (active != 0).view(B, 1)
    s = states[:, :n]

    def u_ref(x):
        if kind == "dubins":
            return _dubins_u_ref(x, goal, sl)
        if kind == "car":
            return _lqr_u_ref(x, torch.cat(
                [goal, torch.zeros_like(goal)], dim=-1), K, sl,
                slice(2, 4), 50.0)
        return _lqr_u_ref(x, goal, K, sl, slice(3, 6), 10.0)

    def reached(x):
        return (x[..., :p] - goal[..., :p]).norm(dim=-1) < d2g

    u = torch.clamp(action + u_ref(s), -act_lim, act_lim)
    prev = reached(s)
    xdot = torch.zeros_like(states)
    if kind == "dubins":
        vc = torch.clamp(states[..., 3], max=sl)
        xdot[..., 0] = vc * torch.cos(states[..., 2])
        xdot[..., 1] = vc * torch.sin(states[..., 2])
        xdot[:, :n, 2] = u[..., 0] * 10
        xdot[:, :n, 3] = u[..., 1]
    elif kind == "car":
        xdot[..., :2] = states[..., 2:]
        xdot[..., 2:] = u
    else:
        damp = states.new_tensor([1.1, 1.1, 6.0])
        xdot[:, :n, :3] = s[..., 3:]
        xdot[:, :n, 3:] = -damp * s[..., 3:] + damp * u
    if kind != "car":  # agents freeze on reach
        xdot[:, :n] = xdot[:, :n] * (~prev).to(states.dtype).unsqueeze(-1)
    stepped = states + xdot * dt
    new_states = torch.where(on.unsqueeze(-1), stepped, states)

    ns = new_states[:, :n]
    reach = reached(ns)
    dist = (ns[:, :, None, :p] - new_states[:, None, :, :p]).norm(dim=-1)
    eye = torch.eye(N, device=states.device, dtype=dist.dtype)[:n]
    collision = ((dist + eye * (2 * r + 1)) < 2 * r).any(dim=2) & on
    cost = action.norm(dim=-1)
    if summed:
        cost = cost.sum(dim=1, keepdim=True)
    reward = (reach.int() - prev.int()) * reach_rew \
        - collision.int() * coll_rew + step_rew - cost * act_cost
    reward = torch.where(on, reward, torch.zeros_like(reward))
    return new_states, u_ref(ns), reward, reach, collision, reach.all(dim=1)
