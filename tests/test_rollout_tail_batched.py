"""rollout_tail_batched.hip: the rollout tail for B scenes in two launches.

The reference in every test is the kernel sequence the op documents, on the
same inputs:

    ops.fused_masks(states.view(B*N, S), B, n_rec, r, kind, "unsafe")
        .view(B, n_rec).any(1)
    ops.env_step_batched(kind, states, goal, where(explore, 0, action),
                         active=ones(B), ...)
    _C.build_graph_padded(new_states[..., :P], new_states, B, n_rec, r_comm,
                          -1, attr_kind, attr_dim, E_cap)

and the comparison is torch.equal on every output (both sides run the same
per-wave device functions).  Float outputs land in NaN-prefilled buffers,
bool outputs in buffers prefilled with the inverse of the expected value,
edge buffers carry a 64-entry guard region past E_cap that must come back
untouched.  The per-scene edge counts in ``flags`` are checked against an
untruncated build of the same states.

Shapes are the smallest that reach each branch: n = 4 agents with three
obstacle rows (N > n_rec), a zero-edge scene between two scenes with edges
(bases), n = 70 (two trips of the in-LDS scan), B = 64 at n = 2 (the base
sum over a full wave), capacities that cut inside a scene and before one.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_branch_scenes as ks  # noqa: E402

from gcbf_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
KINDS = ["DubinsCar", "SimpleCar", "SimpleDrone"]
OUT_KEYS = ("states", "u_ref", "reward", "reach", "collision", "ei", "seg",
            "ea", "flags", "e_count")


# ------------------------------------------------------------------- scenes
def _agent(kind, x, y, k, goal=None, act=None):
    """Agent k of a scene at (x, y) (drones fly at z = 1), moving; ``goal``
    None puts the goal on the agent (at rest: it has reached and stays)."""
    act2 = (0.3 * math.sin(k + 1), 0.2 * math.cos(2 * k)) \
        if act is None else act
    if kind == "DubinsCar":
        if goal is None:
            return ks._dub(x, y, 0.4 * k, 0.0, (x, y), act2)
        return ks._dub(x, y, 0.4 + 0.9 * k, 0.3 + 0.05 * k, goal, act2)
    if kind == "SimpleCar":
        if goal is None:
            return ks._car(x, y, 0.0, 0.0, (x, y), act2)
        return ks._car(x, y, 0.2 * math.sin(k), 0.2 * math.cos(k), goal,
                       act2)
    act3 = tuple(act2) + (0.07,)
    if goal is None:
        return ks._drone((x, y, 1.0), (0.0, 0.0, 0.0), (x, y, 1.0), act3)
    return ks._drone((x, y, 1.0), (0.1 * math.sin(k), 0.1 * math.cos(k),
                                   0.05), goal + (1.2,), act3)


def _obstacles(kind, at):
    """Three obstacle rows around ``at`` (none for SimpleCar)."""
    if kind == "SimpleCar":
        return None
    rows = []
    for k in range(3):
        x, y = at[0] + 0.25 * k, at[1] + 0.5
        if kind == "DubinsCar":
            rows.append([x, y, 0.3 + k, 0.05 * (k + 1)])
        else:
            rows.append([x, y, 1.1, 0.0, 0.0, 0.0])
    return rows


def _scene(kind, name, xy, goals, obs_at):
    agents = {f"a{k}": _agent(kind, x, y, k, g)
              for k, ((x, y), g) in enumerate(zip(xy, goals))}
    return ks._step_scene(kind, name, agents, obs=_obstacles(kind, obs_at))


def _mixed(kind):
    """B = 3, n = 4.  Scene 0: a cluster with two agents 0.09 apart
    (closer than 2r: unsafe) and obstacles in range.  Scene 1: agents 5
    apart, each at rest on its goal, obstacles far away: zero edges, all
    reach.  Scene 2: a 0.3-spaced cluster with obstacles in range."""
    far = [(x + 0.7, y + 0.4) for x, y in
           [(0, 0), (0.09, 0), (0, 0.3), (0.3, 0.3)]]
    s0 = _scene(kind, "unsafe_cluster",
                [(0, 0), (0.09, 0), (0, 0.3), (0.3, 0.3)], far, (0, 0))
    s1 = _scene(kind, "spread_reached",
                [(5.0 * k, 0.0) for k in range(4)], [None] * 4, (50, 50))
    s2 = _scene(kind, "cluster",
                [(0, 0), (0.3, 0), (0, 0.3), (0.3, 0.3)],
                [(0.8, 0.5), (1.0, -0.4), (-0.6, 0.9), (0.9, 0.9)], (0, 0))
    return [s0, s1, s2]


def _n70_pair():
    """B = 2 at n = 70 (DubinsCar): the in-LDS scan takes two wave trips."""
    base = {(s["env"], s["name"]): s for s in ks.dubins_scenes()}[
        ("DubinsCar", "summed_action_cost")]
    other = dict(base)
    other["states"] = base["states"].flip(0).contiguous()
    other["action"] = (base["action"] * -0.5).contiguous()
    return [base, other]


def _pairs64():
    """B = 64 at n = 2 (SimpleCar): every third scene has its two agents
    out of range, the others 0.2 apart."""
    scenes = []
    for b in range(64):
        d = 5.0 if b % 3 == 0 else 0.2
        agents = {
            "a": ks._car(0.1 * b, 0.0, 0.1, 0.05, (0.1 * b + 0.5, 0.4),
                         (0.02 * b, -0.1)),
            "b": ks._car(0.1 * b + d, 0.0, -0.1, 0.02, (0.1 * b, -0.6),
                         (0.1, 0.01 * b))}
        scenes.append(ks._step_scene("SimpleCar", f"pair{b}", agents))
    return scenes


# ----------------------------------------------------------------- plumbing
class _Case:
    """B stacked scenes on the GPU with the env that knows their constants."""

    def __init__(self, scenes):
        from gcbf_amd.env import make_env
        sc0 = scenes[0]
        dev = torch.device("cuda")
        n = len(sc0["names"])
        env = make_env(sc0["env"], n, dev)
        env.train()
        env._goal = sc0["goal"].to(dev)
        env._obs = None if sc0["env"] == "SimpleCar" else sc0["obs"].to(dev)
        env._data = env.add_communication_links(
            env._build_data(sc0["states"].to(dev)))
        self.env = env
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


def _reference(case, explore, E_cap, action=None):
    """The three-call sequence."""
    from gcbf_amd import _C
    env, B, N, S = case.env, case.B, case.N, case.S
    action = case.action if action is None else action
    P = env.pos_dim
    uns = ops.fused_masks(case.states.view(B * N, S), B, case.n_rec,
                          env.agent_radius, env._env_kind, "unsafe") \
        .view(B, case.n_rec).any(dim=1)
    gated = torch.where(explore.view(B, 1, 1) != 0,
                        torch.zeros_like(action), action)
    ones = torch.ones(B, dtype=torch.int32, device="cuda")
    ns, ur, rew, reach, coll, _ = ops.env_step_batched(
        *env.batched_step_args(case.states, case.goal, gated, ones, case.K))
    flat = ns.view(B * N, S)
    pos = flat[:, :P].contiguous()
    build = (pos, flat, B, case.n_rec, env.params["comm_radius"], -1,
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


def _buffers(case, E_cap, ref):
    dev = case.states.device
    env = case.env
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
    guards = (ei_raw[2 * E_cap:], seg_raw[E_cap:],
              ea_raw[E_cap * env.edge_dim:])
    return out, guards


def _tail(case, explore, E_cap, ref, threads=1024, action=None):
    env = case.env
    action = case.action if action is None else action
    out, guards = _buffers(case, E_cap, ref)
    ops.rollout_tail_batched(
        env.fused_step_args(case.states, case.goal, action, case.K),
        explore, case.n_rec, env.params["comm_radius"], env._attr_kind,
        env.edge_dim, E_cap, out=[out[k] for k in OUT_KEYS],
        threads=threads)
    torch.cuda.synchronize()
    return out, guards


def _assert_all(out, ref, guards):
    for k in OUT_KEYS:
        assert torch.equal(out[k], ref[k]), k
    gi, gs, ga = guards
    assert bool((gi == -7).all()), "edge_index guard region written"
    assert bool((gs == -7).all()), "seg guard region written"
    assert bool(torch.isnan(ga).all()), "edge_attr guard region written"


@pytest.fixture(scope="module")
def mixed():
    return {kind: _Case(_mixed(kind)) for kind in KINDS}


@pytest.fixture(scope="module")
def n70():
    return _Case(_n70_pair())


# -------------------------------------------------------------------- tests
@pytest.mark.parametrize("kind", KINDS)
def test_single_scene(kind):
    """B = 1: the branch scenes of the single-scene tail."""
    key = {"DubinsCar": "obstacles", "SimpleDrone": "obstacles",
           "SimpleCar": "reach_leave_stay_collide_t1"}[kind]
    sc = {(s["env"], s["name"]): s for s in ks.step_scenes()}[(kind, key)]
    case = _Case([sc])
    explore = case.explore()
    ref = _reference(case, explore, case.full)
    out, guards = _tail(case, explore, case.full, ref)
    _assert_all(out, ref, guards)
    assert int(out["e_count"]) == int(out["flags"][0, 0])


@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("kind", KINDS)
def test_mixed_scene_set(mixed, kind, threads):
    """B = 3, n = 4: obstacle rows (N > n_rec, not SimpleCar), a zero-edge
    scene between two scenes with edges, an all-reach scene, an unsafe
    one."""
    case = mixed[kind]
    assert case.B == 3 and case.n == 4
    assert (case.N > case.n_rec) == (kind != "SimpleCar")
    explore = case.explore()
    ref = _reference(case, explore, case.full)
    flags = ref["flags"].cpu()
    assert flags[0, 0] > 0 and flags[1, 0] == 0 and flags[2, 0] > 0
    assert flags[:, 1].tolist() == [0, 1, 0]        # reach_all
    assert flags[0, 2] == 1 and flags[1, 2] == 0    # unsafe_any
    assert int(ref["e_count"]) == int(flags[:, 0].sum())
    out, guards = _tail(case, explore, case.full, ref, threads)
    _assert_all(out, ref, guards)
    E = int(out["e_count"])
    assert bool((out["seg"][E:] == case.B * case.N).all())
    assert not bool(torch.isnan(out["ea"]).any())


@pytest.mark.parametrize("kind", KINDS)
def test_explore_gate_selects_zero(mixed, kind):
    """explore = [1, 0, 1]: the gated scenes step under a zero action.  The
    gate is a select, so a NaN action of a gated scene leaves no trace."""
    case = mixed[kind]
    explore = case.explore([1, 0, 1])
    plain = _reference(case, case.explore(), case.full)
    ref = _reference(case, explore, case.full)
    assert not torch.equal(plain["states"][0], ref["states"][0])
    assert torch.equal(plain["states"][1], ref["states"][1])
    poisoned = case.action.clone()
    poisoned[0] = float("nan")
    out, guards = _tail(case, explore, case.full, ref, action=poisoned)
    _assert_all(out, ref, guards)
    assert not bool(torch.isnan(out["states"]).any())
    assert not bool(torch.isnan(out["reward"]).any())


@pytest.mark.parametrize("threads", [256, 1024])
def test_two_trip_scan(n70, threads):
    """n_rec = 70: the scan of the row counts takes two wave trips; with
    256 threads every wave loops over several rows."""
    case = n70
    assert case.n_rec == 70
    explore = case.explore([0, 1])
    ref = _reference(case, explore, case.full)
    assert int(ref["flags"][0, 0]) >= 128 and int(ref["flags"][1, 0]) >= 128
    out, guards = _tail(case, explore, case.full, ref, threads)
    _assert_all(out, ref, guards)


@pytest.mark.parametrize("kind", KINDS)
def test_capacity_below_total_mixed(mixed, kind):
    """E_cap cuts inside the last scene: the total is reported, the guarded
    writes equal the reference's truncated buffers."""
    case = mixed[kind]
    explore = case.explore([0, 0, 1])
    full = _reference(case, explore, case.full)
    E = int(full["e_count"])
    c0 = int(full["flags"][0, 0])
    E_cap = c0 + (E - c0) // 2 + 1
    assert c0 < E_cap < E
    ref = _reference(case, explore, E_cap)
    assert int(ref["e_count"]) == E
    out, guards = _tail(case, explore, E_cap, ref)
    _assert_all(out, ref, guards)
    assert torch.equal(out["ei"], full["ei"][:, :E_cap])
    assert torch.equal(out["flags"], full["flags"])


def test_capacity_before_last_scene(n70):
    """E_cap cuts inside scene 0: scene 1 starts past the capacity and
    writes nothing."""
    case = n70
    explore = case.explore()
    full = _reference(case, explore, case.full)
    E_cap = int(full["flags"][0, 0]) // 2 + 1
    ref = _reference(case, explore, E_cap)
    assert int(ref["e_count"]) == int(full["e_count"]) > E_cap
    out, guards = _tail(case, explore, E_cap, ref)
    _assert_all(out, ref, guards)
    assert torch.equal(out["ei"], full["ei"][:, :E_cap])


def test_base_sum_over_a_full_wave():
    """B = 64 at n = 2: bases are sums over up to 63 scenes, a third of them
    empty."""
    case = _Case(_pairs64())
    assert case.B == 64 and case.n == 2
    pattern = [int(b % 5 == 1) for b in range(64)]
    explore = case.explore(pattern)
    ref = _reference(case, explore, case.full)
    counts = ref["flags"][:, 0].cpu().tolist()
    assert counts == [0 if b % 3 == 0 else 2 for b in range(64)]
    out, guards = _tail(case, explore, case.full, ref)
    _assert_all(out, ref, guards)


def test_deterministic(mixed):
    case = mixed["DubinsCar"]
    explore = case.explore([1, 0, 0])
    ref = _reference(case, explore, case.full)
    a, _ = _tail(case, explore, case.full, ref)
    b, _ = _tail(case, explore, case.full, ref)
    for k in OUT_KEYS:
        assert torch.equal(a[k], b[k]), k


def test_binding_errors(mixed):
    case = mixed["SimpleCar"]
    env = case.env
    explore = case.explore()
    ref = _reference(case, explore, case.full)
    out, _ = _buffers(case, case.full, ref)
    outs = [out[k] for k in OUT_KEYS]
    tail = (case.n_rec, env.params["comm_radius"], env._attr_kind,
            env.edge_dim, case.full)
    # a non-contiguous input
    wide = torch.zeros(case.B, case.N, 2 * case.S, device="cuda")
    strided = wide[..., :case.S]
    assert not strided.is_contiguous()
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.rollout_tail_batched(
            env.fused_step_args(strided, case.goal, case.action, case.K),
            explore, *tail, out=outs)
    with pytest.raises(RuntimeError, match="threads"):
        ops.rollout_tail_batched(
            env.fused_step_args(case.states, case.goal, case.action, case.K),
            explore, *tail, out=outs, threads=128)
    with pytest.raises(RuntimeError, match="explore"):
        ops.rollout_tail_batched(
            env.fused_step_args(case.states, case.goal, case.action, case.K),
            explore.long(), *tail, out=outs)
    # B = 65
    big = _Case(_pairs64() + _pairs64()[:1])
    ex = big.explore()
    with pytest.raises(RuntimeError, match="B must be in"):
        ops.rollout_tail_batched(
            big.env.fused_step_args(big.states, big.goal, big.action, big.K),
            ex, big.n_rec, big.env.params["comm_radius"],
            big.env._attr_kind, big.env.edge_dim, big.full, out=[])
    assert ops.rollout_tail_batched_supported(64, 128, 256)
    assert not ops.rollout_tail_batched_supported(65, 2, 2)
    assert not ops.rollout_tail_batched_supported(2, 129, 129)
    assert not ops.rollout_tail_batched_supported(2, 4, 257)
