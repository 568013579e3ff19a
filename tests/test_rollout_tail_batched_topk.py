"""rollout_tail_batched.hip with a neighbour cap (``topk``).

The reference is the kernel sequence of tests/test_rollout_tail_batched.py
with the cap handed to the stand-alone builder,

    ops.fused_masks(states.view(B*N, S), B, n_rec, r, kind, "unsafe")
        .view(B, n_rec).any(1)
    ops.env_step_batched(kind, states, goal, where(explore, 0, action),
                         active=ones(B), ...)
    _C.build_graph_padded(new_states[..., :P], new_states, B, n_rec, r_comm,
                          topk, attr_kind, attr_dim, E_cap)

and the comparison is torch.equal on all ten outputs.  Float outputs land in
NaN-prefilled buffers, bool outputs in buffers prefilled with the inverse of
the expected value, integer outputs in -7 / -1, and the edge buffers carry a
64-entry guard region past E_cap that must come back untouched.  The
reference's edge list is itself checked against the eager CPU builder under
the same cap, and in every batch (but the one whose point is k >= N) at
least one scene has strictly fewer edges with the cap than without, so the
cap under test is known to be live.

Scenes are those of tests/test_rollout_tail_topk.py, packed into batches of
equal node count: agents stand still (zero velocity), so the stepped
positions are the given ones exactly; coordinates are multiples of 2^-4
(times a comm radius that is a power of two), so distances that should tie
do tie in fp32.  The action is not zero, so a gated scene's new velocities
differ from an ungated one's.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_branch_scenes as ks  # noqa: E402

from gcbf_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
OUT_KEYS = ("states", "u_ref", "reward", "reach", "collision", "ei", "seg",
            "ea", "flags", "e_count")
ENVS = ["SimpleCar", "DubinsCar", "SimpleDrone"]
R_COMM = {"SimpleCar": 1.0, "DubinsCar": 1.0, "SimpleDrone": 0.5}

# planar positions in units of the comm radius, all multiples of 2^-4
CLUSTER = [(0.0, 0.0), (0.25, 0.0), (0.5, 0.0625), (0.0625, 0.3125),
           (0.375, 0.4375)]
SPARSE = [(0.0, 0.0), (0.25, 0.0), (0.5, 0.0625), (1.4375, 0.0625),
          (5.0, 5.0)]
COLLINEAR = [(0.0, 0.0), (0.25, 0.0), (0.5, 0.0)]
FOUR = CLUSTER[:4]
# per-row edge counts the scenes are built for: {k: capped}, None: no cap
ROWS = {
    "cluster": {None: [4] * 5, 2: [2] * 5, 3: [3, 3, 4, 3, 3]},
    "sparse": {None: [2, 2, 3, 1, 0], 2: [2, 2, 2, 1, 0],
               3: [2, 2, 3, 1, 0]},
    "collinear": {None: [2, 2, 2], 1: [1, 2, 1]},
    "four": {None: [3] * 4, 12: [3] * 4},
    "obstacles": {None: [6] * 4, 2: [2] * 4},
}
UNITS = {"cluster": CLUSTER, "sparse": SPARSE, "collinear": COLLINEAR,
         "four": FOUR, "obstacles": FOUR}
# three obstacle rows among the agents: [x, y, heading, speed]
DUBINS_OBS = [[0.125, 0.1875, 0.4, 0.0], [0.3125, -0.25, 1.1, 0.05],
              [0.5625, 0.375, 2.0, 0.0]]


# ------------------------------------------------------------------ scenes
def _agent(env, x, y, k):
    """Agent at rest at (x, y) [z = 1 for the drone], goal well away."""
    goal = (x + 0.75, y + 0.5)
    if env == "SimpleCar":
        return ks._car(x, y, 0.0, 0.0, goal)
    if env == "DubinsCar":
        return ks._dub(x, y, 0.3 * k, 0.0, goal)
    return ks._drone((x, y, 1.0), (0.0, 0.0, 0.0), goal + (1.0,))


def _scene(env, name):
    R = R_COMM[env]
    agents = {f"a{k}": _agent(env, R * x, R * y, k)
              for k, (x, y) in enumerate(UNITS[name])}
    obs = DUBINS_OBS if name == "obstacles" else None
    return ks._step_scene(env, name, agents, obs=obs)


class _Case:
    """B stacked scenes on the GPU with the env that knows their constants."""

    def __init__(self, env_name, names):
        from gcbf_amd.env import make_env
        scenes = [_scene(env_name, name) for name in names]
        sc0 = scenes[0]
        dev = torch.device("cuda")
        n = len(sc0["names"])
        env = make_env(env_name, n, dev)
        env.train()
        assert env.params["comm_radius"] == R_COMM[env_name]
        env._goal = sc0["goal"].to(dev)
        env._obs = None if env_name == "SimpleCar" else sc0["obs"].to(dev)
        env._data = env.add_communication_links(
            env._build_data(sc0["states"].to(dev)))
        self.env, self.names = env, list(names)
        self.states = torch.stack([
            torch.cat([s["states"], s["obs"]], dim=0) for s in scenes]
        ).cuda().contiguous()
        self.goal = torch.stack([s["goal"] for s in scenes]) \
            .cuda().contiguous()
        self.action = torch.stack([s["action"] for s in scenes]) \
            .cuda().contiguous()
        self.B, self.N, self.S = self.states.shape
        self.n = n
        self.n_rec = env._mask_rows(env._data)
        K = env._get_K_tensor()
        self.K = None if K is None else K.contiguous()
        self.full = self.B * self.n_rec * (self.N - 1)

    def explore(self, pattern=None):
        pattern = [0] * self.B if pattern is None else pattern
        return torch.tensor(pattern, dtype=torch.int32, device="cuda")


def _reference(case, explore, E_cap, topk):
    """The three-call sequence with the cap."""
    from gcbf_amd import _C
    env, B, N, S = case.env, case.B, case.N, case.S
    uns = ops.fused_masks(case.states.view(B * N, S), B, case.n_rec,
                          env.agent_radius, env._env_kind, "unsafe") \
        .view(B, case.n_rec).any(dim=1)
    gated = torch.where(explore.view(B, 1, 1) != 0,
                        torch.zeros_like(case.action), case.action)
    ones = torch.ones(B, dtype=torch.int32, device="cuda")
    ns, ur, rew, reach, coll, _ = ops.env_step_batched(
        *env.batched_step_args(case.states, case.goal, gated, ones, case.K))
    flat = ns.view(B * N, S)
    pos = flat[:, :env.pos_dim].contiguous()
    build = (pos, flat, B, case.n_rec, env.params["comm_radius"], topk,
             env._attr_kind, env.edge_dim)
    ei, seg, ea, ecount = _C.build_graph_padded(*build, E_cap)
    # per-scene counts from an untruncated build
    seg_full = _C.build_graph_padded(*build, case.full)[1]
    ptr = torch.arange(B + 1, device="cuda") * N
    bounds = torch.searchsorted(seg_full, ptr)
    counts = (bounds[1:] - bounds[:-1]).to(torch.int32)
    flags = torch.stack([counts, reach.all(dim=1).to(torch.int32),
                         uns.to(torch.int32)], dim=1).contiguous()
    return dict(states=ns, u_ref=ur, reward=rew, reach=reach, collision=coll,
                ei=ei, seg=seg, ea=ea, flags=flags, e_count=ecount)


def _tail(case, explore, E_cap, ref, threads=1024, **kw):
    """The op into prefilled buffers with guard regions past E_cap."""
    env, dev = case.env, case.states.device
    nan = float("nan")
    ei_raw = torch.full((2 * E_cap + GUARD,), -7, dtype=torch.long,
                        device=dev)
    seg_raw = torch.full((E_cap + GUARD,), -7, dtype=torch.long, device=dev)
    ea_raw = torch.full(((E_cap + GUARD) * env.edge_dim,), nan, device=dev)
    out = dict(
        states=torch.full_like(case.states, nan),
        u_ref=torch.full_like(ref["u_ref"], nan),
        reward=torch.full_like(ref["reward"], nan),
        reach=~ref["reach"], collision=~ref["collision"],
        ei=ei_raw[:2 * E_cap].view(2, E_cap), seg=seg_raw[:E_cap],
        ea=ea_raw[:E_cap * env.edge_dim].view(E_cap, env.edge_dim),
        flags=torch.full((case.B, 3), -1, dtype=torch.int32, device=dev),
        e_count=torch.full((1,), -1, dtype=torch.int32, device=dev))
    ops.rollout_tail_batched(
        env.fused_step_args(case.states, case.goal, case.action, case.K),
        explore, case.n_rec, env.params["comm_radius"], env._attr_kind,
        env.edge_dim, E_cap, out=[out[k] for k in OUT_KEYS],
        threads=threads, **kw)
    torch.cuda.synchronize()
    gi, gs, ga = (ei_raw[2 * E_cap:], seg_raw[E_cap:],
                  ea_raw[E_cap * env.edge_dim:])
    assert bool((gi == -7).all()), "edge_index guard region written"
    assert bool((gs == -7).all()), "seg guard region written"
    assert bool(torch.isnan(ga).all()), "edge_attr guard region written"
    return out


def _assert_equal(out, ref):
    for k in OUT_KEYS:
        assert torch.equal(out[k], ref[k]), k


def _cpu_edges(case, ref, topk):
    """Edge list of the eager CPU builder on the reference's new states."""
    env, B, N = case.env, case.B, case.N
    pos = ref["states"].view(B * N, -1)[:, :env.pos_dim].cpu()
    am = None
    if case.n_rec != N:
        am = torch.zeros(B, N, dtype=torch.bool)
        am[:, :case.n_rec] = True
        am = am.view(-1)
    return ops.dense_radius_graph(pos, am, env.params["comm_radius"],
                                  None if topk < 0 else topk, B)


def _row_counts(case, ei):
    """(B, n_rec) edges per receiver row of a global-id edge list."""
    per_node = torch.bincount(ei[1], minlength=case.B * case.N)
    return per_node.view(case.B, case.N)[:, :case.n_rec].tolist()


def _check(case, topk, explore=None, threads=1024, E_cap=None, live=True):
    """Op vs kernel sequence at ``topk``.  The reference's edge list equals
    the CPU builder's under the same cap, the per-row counts with and
    without the cap are the ones the scenes are built for, and (``live``)
    at least one scene loses edges to the cap."""
    explore = case.explore() if explore is None else explore
    E_cap = case.full if E_cap is None else E_cap
    ref = _reference(case, explore, E_cap, topk)
    # agents at rest: their stepped positions are the given ones (an
    # obstacle row may drift; the row counts below are of the new states)
    P, n_rec = case.env.pos_dim, case.n_rec
    assert torch.equal(ref["states"][:, :n_rec, :P],
                       case.states[:, :n_rec, :P])
    E = int(ref["e_count"])
    assert E <= E_cap
    cpu_capped = _cpu_edges(case, ref, topk)
    cpu_free = _cpu_edges(case, ref, -1)
    assert torch.equal(ref["ei"][:, :E].cpu(), cpu_capped)
    key = topk if topk >= 0 else None
    assert _row_counts(case, cpu_capped) == [ROWS[s][key]
                                             for s in case.names]
    assert _row_counts(case, cpu_free) == [ROWS[s][None] for s in case.names]
    capped_per_scene = ref["flags"][:, 0].cpu().tolist()
    free_per_scene = [sum(ROWS[s][None]) for s in case.names]
    assert capped_per_scene == [sum(ROWS[s][key]) for s in case.names]
    if live:
        assert any(c < f for c, f in zip(capped_per_scene, free_per_scene))
    out = _tail(case, explore, E_cap, ref, threads, topk=topk)
    _assert_equal(out, ref)
    assert int(out["e_count"]) == sum(capped_per_scene)
    assert bool((out["seg"][E:] == case.B * case.N).all())
    assert not bool(torch.isnan(out["ea"]).any())
    return ref, out


# ------------------------------------------------------------------- tests
@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("env_name", ENVS)
def test_rows_above_below_and_empty(env_name, threads):
    """B = 3 at n = 5, k = 2.  The clusters have every row above the cap
    (four senders in radius); the sparse set between them has a row above
    it (a2: 3), rows at it, a row below it (a3: 1) and an isolated agent
    (a4: 0), so scene 2's base is a sum over a capped and a sparse scene."""
    case = _Case(env_name, ["cluster", "sparse", "cluster"])
    _check(case, 2, threads=threads)


@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("env_name", ENVS)
def test_tie_at_the_kth_distance_keeps_both_b1(env_name, threads):
    """B = 1, three collinear agents at spacing d, k = 1: the middle
    agent's two neighbours are equidistant and both edges appear (the row
    keeps 2 > k edges)."""
    case = _Case(env_name, ["collinear"])
    P = case.env.pos_dim
    p = case.states[0, :, :P]
    d10, d12 = (p[1] - p[0]).norm(), (p[1] - p[2]).norm()
    assert bool(d10 == d12), "the tie must be exact in fp32"
    assert float(d10) == 0.25 * R_COMM[env_name]
    ref, out = _check(case, 1, threads=threads)
    assert int(out["e_count"]) == 4
    assert out["ei"][:, :4].tolist() == [[1, 0, 2, 1], [0, 1, 1, 2]]
    assert out["seg"].tolist()[:4] == [0, 1, 1, 2]
    assert bool((out["seg"][4:] == 3).all())


@pytest.mark.parametrize("env_name", ENVS)
def test_more_scenes_than_pad_entries(env_name):
    """B = 8 collinear triples, k = 1, mixed gate.  At full capacity the 16
    pad entries split into chunks of 2, fewer than the 8 workgroups that
    share them out; at a capacity three above the edge count the chunk is
    one entry and five workgroups have none.  Global ids of scene b start at
    3 b."""
    case = _Case(env_name, ["collinear"] * 8)
    explore = case.explore([0, 1, 0, 0, 1, 1, 0, 1])
    ref, out = _check(case, 1, explore=explore)
    assert int(out["e_count"]) == 32 and case.full == 48
    assert out["ei"][:, 28:32].tolist() == [[22, 21, 23, 22],
                                            [21, 22, 22, 23]]
    ref, out = _check(case, 1, explore=explore, E_cap=35, threads=256)
    assert int(out["e_count"]) == 32


@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("env_name", ENVS)
def test_cap_at_least_n_is_no_cap(env_name, threads):
    """B = 2 at n = 4, k = 12 >= N: equal to topk = -1 (no workspace is
    used), and omitting topk is topk = -1."""
    case = _Case(env_name, ["four", "four"])
    explore = case.explore([0, 1])
    ref, out = _check(case, 12, explore=explore, threads=threads, live=False)
    free = _reference(case, explore, case.full, -1)
    _assert_equal(out, free)
    explicit = _tail(case, explore, case.full, free, threads, topk=-1)
    default = _tail(case, explore, case.full, free, threads)
    _assert_equal(explicit, free)
    _assert_equal(default, explicit)


@pytest.mark.parametrize("threads", [256, 1024])
def test_receivers_fewer_than_nodes(threads):
    """DubinsCar n = 4 plus 3 obstacle rows, B = 2, k = 2: n_rec < N, the
    obstacle rows send and never receive, the threshold workspace is
    indexed by receiver row (b * n_rec + row), not by node."""
    case = _Case("DubinsCar", ["obstacles", "obstacles"])
    assert case.n_rec == 4 and case.N == 7
    ref, out = _check(case, 2, explore=case.explore([1, 0]), threads=threads)
    E = int(out["e_count"])
    src, dst = out["ei"][0, :E] % 7, out["ei"][1, :E] % 7
    assert bool((src >= 4).any()), "an obstacle must send"
    assert bool((dst < 4).all())


@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("env_name", ENVS)
def test_live_and_inactive_scenes_mixed_gate(env_name, threads):
    """B = 3 at k = 3: the clusters lose an edge per row but a2's, whose
    third and fourth senders tie (0.5 to the left, 0.5 diagonally); the
    sparse scene between them has no row above 3 and keeps its uncapped
    edges.  The gate is [1, 0, 1]: the gated scenes step under a zero
    action."""
    case = _Case(env_name, ["cluster", "sparse", "cluster"])
    explore = case.explore([1, 0, 1])
    ref, out = _check(case, 3, explore=explore, threads=threads)
    assert out["flags"][:, 0].tolist() == [16, 8, 16]
    plain = _reference(case, case.explore(), case.full, 3)
    assert not torch.equal(plain["states"][0], out["states"][0])
    assert torch.equal(plain["states"][1], out["states"][1])


def test_capped_output_differs_from_uncapped():
    """The cap reaches the op: at k = 2 the cluster's list is shorter than
    what topk = -1 writes for the same inputs."""
    case = _Case("SimpleCar", ["cluster", "sparse", "cluster"])
    ref, out = _check(case, 2)
    free = _reference(case, case.explore(), case.full, -1)
    assert int(out["e_count"]) == 27 < int(free["e_count"]) == 48


def test_binding_refuses_a_cap_of_zero():
    case = _Case("SimpleCar", ["four", "four"])
    explore = case.explore()
    ref = _reference(case, explore, case.full, -1)
    for bad in (0, -2):
        with pytest.raises(RuntimeError, match="topk"):
            _tail(case, explore, case.full, ref, 1024, topk=bad)
