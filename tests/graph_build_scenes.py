"""Hand-built scenes and the fp64 reference for
tests/test_graph_build_branches.py.

Everything here is plain torch / Python on CPU.  A scene is a dict

    name, B, N, n_rec, P, S, r, k (neighbour cap or None), attr (ATTR_*),
    states (B*N, S) fp32 (positions are its first P columns),
    exact  {(b, i, j)}: pairs declared to sit at d == r exactly,
    ties   {(b, i)}: capped rows declared to hold an exact tie at the k-th
                     distance.

The reference is a loop over graph, receiver and sender in fp64 that does not
touch gcbf_amd/ops/eager.py.  It returns the edge list and the adjusted
distance rows, so a test can require that no decision sits within fp32 noise
of its threshold.  Exact cases (d == r, ties) use coordinates that are
multiples of 1/8 only: d^2 is then exact in fp32 with or without FMA
contraction.
"""
import copy
import functools
import math

import torch

ATTR_DIFF = 0
ATTR_DUBINS = 1

MARGIN = 1e-4        # relative to r
FAR = 3.0            # grid pitch of mutually isolated nodes, in units of r


# ------------------------------------------------------------ fp64 reference
def ref_rows(sc, k="scene"):
    """Adjusted fp64 distance rows, thresholds and kept senders.

    Returns (edges, rows): ``edges`` the list of global (src, dst) ordered
    by (graph, dst, src); ``rows[(b, i)]`` = dict(d=[...N], kth=float or
    None, keep=[j...]).
    """
    B, N, n_rec, P, r = sc["B"], sc["N"], sc["n_rec"], sc["P"], sc["r"]
    k = sc["k"] if k == "scene" else k
    p = sc["states"][:, :P].double().tolist()
    edges, rows = [], {}
    for b in range(B):
        for i in range(n_rec):
            pi = p[b * N + i]
            d = []
            for j in range(N):
                pj = p[b * N + j]
                dij = math.sqrt(sum((pi[c] - pj[c]) ** 2 for c in range(P)))
                if i == j:
                    dij += r + 1.0
                d.append(dij)
            kth = None
            if k is not None and 0 < k < N:
                kth = sorted(d)[k - 1]
            keep = [j for j in range(N)
                    if d[j] < r and (kth is None or d[j] <= kth)]
            rows[(b, i)] = dict(d=d, kth=kth, keep=keep)
            edges += [(b * N + j, b * N + i) for j in keep]
    return edges, rows


def ref_edge_index(sc, k="scene"):
    edges, _ = ref_rows(sc, k)
    if not edges:
        return torch.zeros(2, 0, dtype=torch.long)
    return torch.tensor(edges, dtype=torch.long).t().contiguous()


def ref_attr64(sc, ei):
    """fp64 edge attributes of the edge list ``ei``."""
    s = sc["states"].double()
    if sc["attr"] == ATTR_DIFF:
        info = s
    else:
        info = torch.cat([s[:, :3],
                          (s[:, 3] * torch.cos(s[:, 2]))[:, None],
                          (s[:, 3] * torch.sin(s[:, 2]))[:, None]], dim=1)
    return info[ei[0]] - info[ei[1]]


def agent_mask(sc):
    if sc["n_rec"] == sc["N"]:
        return None
    am = torch.zeros(sc["B"], sc["N"], dtype=torch.bool)
    am[:, :sc["n_rec"]] = True
    return am.view(-1)


# ------------------------------------------------------------------ builders
def _grid(m, P, r, origin=10.0):
    """m-th node of a lattice with pitch FAR*r: mutually out of range."""
    pt = [origin + (m % 12) * FAR * r, origin + (m // 12) * FAR * r]
    return pt + [0.0] * (P - 2)


def _cluster(N, P, r, centre=0.0):
    """N distinct points inside a ball of diameter < r/2."""
    pts = []
    for i in range(N):
        rad = 0.24 * r * math.sqrt((i + 1) / N)
        pt = [centre + rad * math.cos(2.4 * i), centre + rad * math.sin(2.4 * i)]
        if P == 3:
            pt.append(0.05 * r * math.cos(1.3 * i))
        pts.append(pt)
    return pts


def _scene(name, B, N, n_rec, pos, r=1.0, k=None, attr=ATTR_DIFF, S=None,
           rest=None, seed=0, exact=(), ties=()):
    """``pos`` is a list of B*N points; the remaining state columns come
    from ``rest`` (B*N, S-P) or a seeded generator."""
    pos = torch.tensor(pos, dtype=torch.float64).float()
    P = pos.shape[1]
    assert pos.shape[0] == B * N
    S = S or (4 if P == 2 else 6)
    if rest is None:
        g = torch.Generator().manual_seed(1000 + seed)
        rest = torch.randn(B * N, S - P, generator=g)
    states = torch.cat([pos, rest.float()], dim=1).contiguous()
    return dict(name=name, B=B, N=N, n_rec=n_rec, P=P, S=S, r=r, k=k,
                attr=attr, states=states, exact=set(exact), ties=set(ties))


def lane_trip_scene(N, P):
    """Graph 0: a cluster inside r/2, every receiver has all N-1 senders
    (full 64-lane ballots).  Graph 1: everything out of range except nodes 1
    and N-1, so receiver 0 has no sender and receiver 1's only sender sits
    in the last lane trip (j = N-1: >= 64 for N = 65, >= 128 for N = 130)."""
    r = 1.0
    g0 = _cluster(N, P, r)
    g1 = [_grid(m, P, r) for m in range(N)]
    g1[N - 1] = [g1[1][0] + 0.3 * r, g1[1][1] + 0.2 * r] + \
        ([0.1 * r] if P == 3 else [])
    return _scene(f"lanes_N{N}_P{P}", 2, N, N, g0 + g1, r=r, seed=N + P)


def partial_wg_scene():
    """B = 3, N = 7, n_rec = 5: 15 receiver rows, the last workgroup of four
    is partial.  Nodes 5 and 6 of every graph are obstacles: they send to
    agents 2 and 4 and would receive from them if rows >= n_rec received."""
    pos = []
    for b in range(3):
        s, y = 1.0 + 0.1 * b, 20.0 * b
        pos += [[0.0, y], [0.5 * s, y], [5.0, y], [10.0, y], [15.0, y],
                [5.0, y + 0.6 * s], [15.0 + 0.3 * s, y + 0.3 * s]]
    return _scene("partial_wg", 3, 7, 5, pos, seed=1)


def isolation_scene():
    """B = 2; graph 1's nodes sit on top of graph 0's, except node 5, which
    is out of everyone's range in graph 1 only."""
    g0 = [[0.0, 0.0], [0.4, 0.1], [0.2, 0.7], [3.0, 0.0], [3.5, 0.3],
          [0.6, -0.5]]
    g1 = copy.deepcopy(g0)
    g1[5] = [8.0, 8.0]
    return _scene("isolation", 2, 6, 6, g0 + g1, seed=2)


def strict_radius_scene():
    """r = 1.25: the pair (0,0)-(0.75,1.0) is at d == r exactly (no edge);
    the pair 2-3 is at r(1 - 1e-3) (an edge)."""
    r = 1.25
    pos = [[0.0, 0.0], [0.75, 1.0], [10.0, 0.0],
           [10.0 + r * (1 - 1e-3), 0.0]]
    return _scene("strict_radius", 1, 4, 4, pos, r=r, seed=3,
                  exact=[(0, 0, 1), (0, 1, 0)])


CAP_LINE_X = [0.0, 0.3, 0.7, 1.2, 1.8, 4.0]


def cap_line_scene(k):
    """Six nodes on a line with growing gaps, all in-row distances distinct.
    k = 1: row 0 binds (kth 0.3 < r, one of two in range kept), row 5 does
    not (kth 2.2 > r).  k = 2: row 1 binds, row 4 does not.  k = N-1 keeps
    everything in range; k >= N is no cap."""
    pos = [[x, 0.25] for x in CAP_LINE_X]
    return _scene(f"cap_line_k{k}", 1, 6, 6, pos, k=k, seed=4)


def cap_tie70_scene():
    """N = 70, one receiver, k = 5: three nearer senders, then an exact tie
    group of four mirror images (+-0.5, +-0.25) at j = 62..65, straddling
    the two lane trips, then one farther sender in range.  All four tied
    senders are kept: 7 edges for k = 5."""
    N = 70
    pos = [_grid(m, 2, 1.0) for m in range(N)]
    pos[0] = [0.0, 0.0]
    pos[1], pos[2], pos[3] = [0.125, 0.0], [-0.25, 0.125], [0.125, -0.375]
    pos[62], pos[63] = [0.5, 0.25], [-0.5, 0.25]
    pos[64], pos[65] = [0.5, -0.25], [-0.5, -0.25]
    pos[66] = [0.75, 0.125]
    return _scene("cap_tie70", 1, N, 1, pos, k=5, seed=5, ties=[(0, 0)])


def cap_colocated_scene(k):
    """Nodes 0, 1, 2 share one point: d = 0 twice in rows 0..2 and an exact
    three-way tie in rows 3 and 4."""
    pos = [[1.0, 1.0], [1.0, 1.0], [1.0, 1.0], [1.5, 1.0], [1.0, 1.75]]
    return _scene(f"cap_colocated_k{k}", 1, 5, 5, pos, k=k, seed=6,
                  ties=[(0, i) for i in range(5)])


def cap_nrec_scene():
    """B = 2, N = 8, n_rec = 5, k = 2: obstacles among the nearest senders."""
    g = torch.Generator().manual_seed(77)
    pos = (torch.rand(16, 2, generator=g) * 1.6).tolist()
    return _scene("cap_nrec_b2", 2, 8, 5, pos, k=2, seed=7)


DUBINS_N = 14
DUBINS_THETA = [-8.0, -5.6, -3.1, -1.7, -0.4, 0.9, 2.6, 4.3, 6.1, 8.0,
                100.0, -50.0, 0.0, math.pi]
DUBINS_V = [0.0, 1.5, -1.5, 0.7, -0.3, 1.5, 0.0, -1.5, 1.1, -0.9,
            1.5, -1.5, 1.5, -1.5]


def dubins_scene(dense):
    """ATTR_DUBINS, B = 2, N = 14, n_rec = 10.  Headings in [-8, 8] plus
    100, -50, 0 and fp32 pi; speeds 0, +-1.5 and a few others; graph 1 has
    the speed list rotated by three.  ``dense``: both graphs are clusters
    (every pair an edge); sparse: graph 0 keeps three close nodes, graph 1
    none."""
    N, r = DUBINS_N, 1.0
    if dense:
        pos = _cluster(N, 2, r) + _cluster(N, 2, r, centre=5.0)
    else:
        g0 = [_grid(m, 2, r) for m in range(N)]
        g0[1] = [g0[0][0] + 0.3, g0[0][1] + 0.1]
        g0[12] = [g0[0][0] - 0.2, g0[0][1] + 0.4]
        pos = g0 + [_grid(m, 2, r, origin=100.0) for m in range(N)]
    th = torch.tensor(DUBINS_THETA + DUBINS_THETA[::-1])
    v = torch.tensor(DUBINS_V + DUBINS_V[3:] + DUBINS_V[:3])
    return _scene("dubins_dense" if dense else "dubins_sparse", 2, N, 10,
                  pos, attr=ATTR_DUBINS, S=4,
                  rest=torch.stack([th, v], dim=1))


@functools.lru_cache(maxsize=None)
def scenes():
    out = [lane_trip_scene(N, P) for N in (63, 64, 65, 130) for P in (2, 3)]
    out += [partial_wg_scene(), isolation_scene(), strict_radius_scene()]
    out += [cap_line_scene(k) for k in (1, 2, 5, 6, 9)]
    out += [cap_tie70_scene(), cap_colocated_scene(1), cap_colocated_scene(2),
            cap_nrec_scene(), dubins_scene(True), dubins_scene(False)]
    return {sc["name"]: sc for sc in out}
