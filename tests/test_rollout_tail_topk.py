"""rollout_tail.hip with a neighbour cap (``topk``).

The reference is the kernel sequence of tests/test_rollout_tail.py with the
cap handed to the stand-alone builder,

    ops.fused_masks(states, 1, n_rec, r, kind, "unsafe").any()
    ops.env_step_fused(*env.fused_step_args(...))
    _C.build_graph_padded(new_states[:, :P], new_states, 1, n_rec, r_comm,
                          topk, ...)
    reach.all()

and the comparison is torch.equal on all nine outputs: the tail hands
``topk`` to the per-wave bodies the builder calls.  The reference's edge
list is itself checked against the eager CPU builder on the stepped
positions, so the cap each scene is built for is known to be live.

Scenes are the smallest that reach every branch of the cap: every row above
k, a row below k and an empty row, an exact tie at the k-th distance, k >= N
(no cap), receivers fewer than nodes, and a capacity one short of the count.
Agents stand still (zero velocity), so the stepped positions are the given
ones exactly; coordinates are multiples of 2^-4 (times a comm radius that is
a power of two), so distances that should tie do tie in fp32.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_branch_scenes as ks  # noqa: E402

from gcbf_amd import ops  # noqa: E402

GUARD = 64
OUT_KEYS = ("states", "u_ref", "reward", "reach", "collision", "ei", "seg",
            "ea", "flags")
ENVS = ["SimpleCar", "DubinsCar", "SimpleDrone"]
R_COMM = {"SimpleCar": 1.0, "DubinsCar": 1.0, "SimpleDrone": 0.5}

# planar positions in units of the comm radius, all multiples of 2^-4
CLUSTER = [(0.0, 0.0), (0.25, 0.0), (0.5, 0.0625), (0.0625, 0.3125),
           (0.375, 0.4375)]
SPARSE = [(0.0, 0.0), (0.25, 0.0), (0.5, 0.0625), (1.4375, 0.0625),
          (5.0, 5.0)]
COLLINEAR = [(0.0, 0.0), (0.25, 0.0), (0.5, 0.0)]
FOUR = CLUSTER[:4]


# ------------------------------------------------------------------ scenes
def _agent(env, x, y, k):
    """Agent at rest at (x, y) [z = 1 for the drone], goal well away."""
    goal = (x + 0.75, y + 0.5)
    if env == "SimpleCar":
        return ks._car(x, y, 0.0, 0.0, goal)
    if env == "DubinsCar":
        return ks._dub(x, y, 0.3 * k, 0.0, goal)
    return ks._drone((x, y, 1.0), (0.0, 0.0, 0.0), goal + (1.0,))


def _scene(env, name, units, obs=None):
    R = R_COMM[env]
    agents = {f"a{k}": _agent(env, R * x, R * y, k)
              for k, (x, y) in enumerate(units)}
    return ks._step_scene(env, name, agents, obs=obs)


def _inject(sc, dev):
    from gcbf_amd.env import make_env
    env = make_env(sc["env"], len(sc["names"]), torch.device(dev))
    env.train()
    env._goal = sc["goal"].to(dev)
    env._obs = None if sc["env"] == "SimpleCar" else sc["obs"].to(dev)
    env._data = env.add_communication_links(
        env._build_data(sc["states"].to(dev)))
    return env


def _inputs(sc):
    env = _inject(sc, "cuda")
    assert env.params["comm_radius"] == R_COMM[sc["env"]]
    states = torch.cat([sc["states"], sc["obs"]], dim=0).cuda().contiguous()
    K = env._get_K_tensor()
    args = env.fused_step_args(states, env._goal.contiguous(),
                               sc["action"].cuda().contiguous(),
                               None if K is None else K.contiguous())
    n_rec = env._mask_rows(env._data)
    return env, states, args, n_rec


def _reference(env, states, args, n_rec, E_max, topk):
    from gcbf_amd import _C
    uns = ops.fused_masks(states, 1, n_rec, env.agent_radius, env._env_kind,
                          "unsafe")
    ns, ur, rew, reach, coll = ops.env_step_fused(*args)
    ei, seg, ea, ecount = _C.build_graph_padded(
        ns[:, :env.pos_dim].contiguous(), ns, 1, n_rec,
        env.params["comm_radius"], topk, env._attr_kind, env.edge_dim, E_max)
    flags = torch.stack([ecount[0], reach.all().to(torch.int32),
                         uns.any().to(torch.int32)]).to(torch.int32)
    return dict(states=ns, u_ref=ur, reward=rew, reach=reach, collision=coll,
                ei=ei, seg=seg, ea=ea, flags=flags)


def _tail(env, states, args, n_rec, E_max, ref, threads, **kw):
    """The tail into prefilled buffers with guard regions past E_max."""
    dev = states.device
    n, A = ref["u_ref"].shape
    nan = float("nan")
    ei_raw = torch.full((2 * E_max + GUARD,), -7, dtype=torch.long,
                        device=dev)
    seg_raw = torch.full((E_max + GUARD,), -7, dtype=torch.long, device=dev)
    ea_raw = torch.full(((E_max + GUARD) * env.edge_dim,), nan, device=dev)
    out = dict(
        states=torch.full_like(states, nan),
        u_ref=torch.full((n, A), nan, device=dev),
        reward=torch.full((n,), nan, device=dev),
        reach=~ref["reach"], collision=~ref["collision"],
        ei=ei_raw[:2 * E_max].view(2, E_max), seg=seg_raw[:E_max],
        ea=ea_raw[:E_max * env.edge_dim].view(E_max, env.edge_dim),
        flags=torch.full((3,), -1, dtype=torch.int32, device=dev))
    ops.rollout_tail(args, n_rec, env.params["comm_radius"], env._attr_kind,
                     env.edge_dim, E_max, out=[out[k] for k in OUT_KEYS],
                     threads=threads, **kw)
    torch.cuda.synchronize()
    gi, gs, ga = (ei_raw[2 * E_max:], seg_raw[E_max:],
                  ea_raw[E_max * env.edge_dim:])
    assert bool((gi == -7).all()), "edge_index guard region written"
    assert bool((gs == -7).all()), "seg guard region written"
    assert bool(torch.isnan(ga).all()), "edge_attr guard region written"
    return out


def _assert_equal(out, ref, upto=None):
    for k in OUT_KEYS:
        if upto is not None and k in ("ei", "seg", "ea"):
            a = out[k][..., :upto] if k == "ei" else out[k][:upto]
            b = ref[k][..., :upto] if k == "ei" else ref[k][:upto]
        else:
            a, b = out[k], ref[k]
        assert torch.equal(a, b), k


def _cpu_edges(env, ref, n_rec, topk):
    """Edge list of the eager CPU builder on the reference's new states."""
    pos = ref["states"][:, :env.pos_dim].cpu()
    N = pos.shape[0]
    am = None
    if n_rec != N:
        am = torch.zeros(N, dtype=torch.bool)
        am[:n_rec] = True
    return ops.dense_radius_graph(pos, am, env.params["comm_radius"],
                                  None if topk < 0 else topk)


def _row_counts(ei, n_rec):
    return torch.bincount(ei[1], minlength=n_rec)[:n_rec].tolist()


def _check(sc, topk, threads, counts_capped, counts_free):
    """Tail vs kernel sequence at ``topk``; the reference's per-row edge
    counts, with and without the cap, are the ones the scene is built for
    and agree with the CPU builder."""
    env, states, args, n_rec = _inputs(sc)
    N = states.shape[0]
    # agents at rest: the stepped positions are the given ones
    E_max = n_rec * (N - 1)
    ref = _reference(env, states, args, n_rec, E_max, topk)
    assert torch.equal(ref["states"][:n_rec, :env.pos_dim],
                       states[:n_rec, :env.pos_dim])
    E = int(ref["flags"][0])
    cpu_capped = _cpu_edges(env, ref, n_rec, topk)
    cpu_free = _cpu_edges(env, ref, n_rec, -1)
    assert torch.equal(ref["ei"][:, :E].cpu(), cpu_capped)
    assert _row_counts(cpu_capped, n_rec) == counts_capped
    assert _row_counts(cpu_free, n_rec) == counts_free
    out = _tail(env, states, args, n_rec, E_max, ref, threads, topk=topk)
    _assert_equal(out, ref)
    assert not bool(torch.isnan(out["ea"]).any())
    return env, states, args, n_rec, ref, out


# ------------------------------------------------------------------- tests
@pytest.mark.gpu
@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("env_name", ENVS)
def test_cap_live_on_every_row(env_name, threads):
    """n = 5 clustered, k = 2: every row has four senders in radius."""
    _check(_scene(env_name, "cluster", CLUSTER), 2, threads,
           [2] * 5, [4] * 5)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("env_name", ENVS)
def test_rows_below_the_cap_and_empty(env_name, threads):
    """k = 2 with a row above the cap (a2: 3 in radius), rows at it, a row
    below it (a3: 1) and an isolated agent (a4: 0)."""
    _check(_scene(env_name, "sparse", SPARSE), 2, threads,
           [2, 2, 2, 1, 0], [2, 2, 3, 1, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("env_name", ENVS)
def test_tie_at_the_kth_distance_keeps_both(env_name, threads):
    """Three collinear agents at spacing d, k = 1: the middle agent's two
    neighbours are equidistant and both edges appear."""
    sc = _scene(env_name, "collinear", COLLINEAR)
    P = ks.CONST[env_name]["P"]
    p = sc["states"][:, :P]
    d10 = (p[1] - p[0]).norm()
    d12 = (p[1] - p[2]).norm()
    assert bool(d10 == d12), "the tie must be exact in fp32"
    assert float(d10) == 0.25 * R_COMM[env_name]
    env, states, args, n_rec, ref, out = _check(
        sc, 1, threads, [1, 2, 1], [2, 2, 2])
    assert int(out["flags"][0]) == 4
    assert out["ei"][:, :4].tolist() == [[1, 0, 2, 1], [0, 1, 1, 2]]
    assert out["seg"].tolist()[:4] == [0, 1, 1, 2]
    assert bool((out["seg"][4:] == 3).all())


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("env_name", ENVS)
def test_cap_at_least_n_is_no_cap(env_name, threads):
    """n = 4, k = 12: equal to topk = -1, and the default is topk = -1."""
    sc = _scene(env_name, "four", FOUR)
    env, states, args, n_rec, ref, out = _check(
        sc, 12, threads, [3] * 4, [3] * 4)
    E_max = n_rec * (states.shape[0] - 1)
    free = _reference(env, states, args, n_rec, E_max, -1)
    _assert_equal(out, free)
    explicit = _tail(env, states, args, n_rec, E_max, free, threads, topk=-1)
    default = _tail(env, states, args, n_rec, E_max, free, threads)
    _assert_equal(explicit, free)
    _assert_equal(default, explicit)


def _dubins_obstacle_scene():
    # three obstacle rows among the agents: [x, y, heading, speed]
    obs = [[0.125, 0.1875, 0.4, 0.0], [0.3125, -0.25, 1.1, 0.05],
           [0.5625, 0.375, 2.0, 0.0]]
    return _scene("DubinsCar", "obstacles", FOUR, obs=obs)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [256, 1024])
def test_receivers_fewer_than_nodes(threads):
    """DubinsCar n = 4 plus 3 obstacles, k = 2: n_rec < N, obstacle rows
    send and never receive."""
    sc = _dubins_obstacle_scene()
    env, states, args, n_rec, ref, out = _check(
        sc, 2, threads, [2] * 4, [6] * 4)
    assert n_rec == 4 and states.shape[0] == 7
    E = int(out["flags"][0])
    assert bool((out["ei"][0, :E] >= 4).any()), "an obstacle must send"
    assert bool((out["ei"][1, :E] < 4).all())


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [256, 1024])
def test_capacity_one_short_with_cap(threads):
    """E_max one below the capped edge count: the true count is reported,
    the first E_max entries match, nothing past E_max is written."""
    sc = _scene("SimpleCar", "cluster", CLUSTER)
    env, states, args, n_rec = _inputs(sc)
    full = _reference(env, states, args, n_rec,
                      n_rec * (states.shape[0] - 1), 2)
    E = int(full["flags"][0])
    assert E == 10
    E_max = E - 1
    ref = _reference(env, states, args, n_rec, E_max, 2)
    assert int(ref["flags"][0]) == E
    out = _tail(env, states, args, n_rec, E_max, ref, threads, topk=2)
    assert int(out["flags"][0]) == E
    _assert_equal(out, ref, upto=E_max)
    assert torch.equal(out["ei"], full["ei"][:, :E_max])


@pytest.mark.gpu
def test_binding_refuses_a_cap_of_zero():
    sc = _scene("SimpleCar", "four", FOUR)
    env, states, args, n_rec = _inputs(sc)
    E_max = n_rec * (states.shape[0] - 1)
    ref = _reference(env, states, args, n_rec, E_max, -1)
    for bad in (0, -2):
        with pytest.raises(RuntimeError, match="topk"):
            _tail(env, states, args, n_rec, E_max, ref, 1024, topk=bad)
