"""rollout_tail.hip: one launch for mask -> step -> graph rebuild -> flags.

The reference in every kernel-level test is the kernel sequence the
captured rollout step ran before, on the same inputs:

    ops.fused_masks(states, 1, n_rec, r, kind, "unsafe").any()
    ops.env_step_fused(*env.fused_step_args(...))
    _C.build_graph_padded(new_states[:, :P], new_states, 1, n_rec, ...)
    reach.all()

and the comparison is torch.equal on every output (the tail calls the same
per-wave device functions, so nothing may differ by even one bit).  Float
outputs land in NaN-prefilled buffers, bool outputs in buffers prefilled
with the inverse of the expected value, edge buffers carry a 64-entry guard
region past E_max that must come back untouched.

Scenes come from tests/kernel_branch_scenes.py: the smallest shapes at which
the shared bodies take every branch (n % 4 = 1, 66 obstacle rows, n = 70 for
the second trip of the pair scan).
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_branch_scenes as ks  # noqa: E402

from gcbf_amd import ops  # noqa: E402

GUARD = 64
STEP_SCENES = {(s["env"], s["name"]): s for s in ks.step_scenes()}
TAIL_KEYS = [
    ("DubinsCar", "obstacles"),
    ("DubinsCar", "summed_action_cost"),
    ("DubinsCar", "u_ref_edges"),
    ("SimpleCar", "reach_leave_stay_collide_t1"),
    ("SimpleCar", "far_neighbour"),
    ("SimpleDrone", "obstacles"),
    ("SimpleDrone", "collide_t_only_frozen_nbr"),
]
TAIL_IDS = [f"{e}-{n}" for e, n in TAIL_KEYS]


# ------------------------------------------------------------------ plumbing
def _inject(sc, dev):
    """Env holding the scene: goal, obstacle rows and the linked graph."""
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
    states = torch.cat([sc["states"], sc["obs"]], dim=0).cuda().contiguous()
    K = env._get_K_tensor()
    args = env.fused_step_args(states, env._goal.contiguous(),
                               sc["action"].cuda().contiguous(),
                               None if K is None else K.contiguous())
    n_rec = env._mask_rows(env._data)
    return env, states, args, n_rec


def _reference(env, states, args, n_rec, E_max):
    """The kernel sequence of the multi-launch rollout body."""
    from gcbf_amd import _C
    uns = ops.fused_masks(states, 1, n_rec, env.agent_radius, env._env_kind,
                          "unsafe")
    ns, ur, rew, reach, coll = ops.env_step_fused(*args)
    ei, seg, ea, ecount = _C.build_graph_padded(
        ns[:, :env.pos_dim].contiguous(), ns, 1, n_rec,
        env.params["comm_radius"], -1, env._attr_kind, env.edge_dim, E_max)
    flags = torch.stack([ecount[0], reach.all().to(torch.int32),
                         uns.any().to(torch.int32)]).to(torch.int32)
    return dict(states=ns, u_ref=ur, reward=rew, reach=reach, collision=coll,
                ei=ei, seg=seg, ea=ea, flags=flags, unsafe_rows=uns)


def _tail(env, states, args, n_rec, E_max, ref, threads=1024):
    """Run the tail into prefilled buffers with guard regions; returns the
    outputs and the guards."""
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
                     env.edge_dim, E_max,
                     out=[out[k] for k in ("states", "u_ref", "reward",
                                           "reach", "collision", "ei", "seg",
                                           "ea", "flags")],
                     threads=threads)
    torch.cuda.synchronize()
    guards = (ei_raw[2 * E_max:], seg_raw[E_max:],
              ea_raw[E_max * env.edge_dim:])
    return out, guards


def _assert_guards(guards):
    gi, gs, ga = guards
    assert bool((gi == -7).all()), "edge_index guard region written"
    assert bool((gs == -7).all()), "seg guard region written"
    assert bool(torch.isnan(ga).all()), "edge_attr guard region written"


def _assert_equal(out, ref, upto=None):
    for k in ("states", "u_ref", "reward", "reach", "collision", "flags"):
        assert torch.equal(out[k], ref[k]), k
    if upto is None:
        for k in ("ei", "seg", "ea"):
            assert torch.equal(out[k], ref[k]), k
    else:
        assert torch.equal(out["ei"][:, :upto], ref["ei"][:, :upto])
        assert torch.equal(out["seg"][:upto], ref["seg"][:upto])
        assert torch.equal(out["ea"][:upto], ref["ea"][:upto])


def _full_capacity(n_rec, N):
    return n_rec * (N - 1)


# -------------------------------------------------- branch scenes, all kinds
@pytest.mark.gpu
@pytest.mark.parametrize("key", TAIL_KEYS, ids=TAIL_IDS)
def test_tail_equals_kernel_sequence(key):
    """E_max = n_rec (N - 1), the engine's capacity at small scenes."""
    env, states, args, n_rec = _inputs(STEP_SCENES[key])
    E_max = _full_capacity(n_rec, states.shape[0])
    ref = _reference(env, states, args, n_rec, E_max)
    out, guards = _tail(env, states, args, n_rec, E_max, ref)
    _assert_equal(out, ref)
    _assert_guards(guards)
    assert not bool(torch.isnan(out["ea"]).any())


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [256, 512])
def test_tail_block_sizes(threads):
    """Fewer waves than rows: every wave loops over several rows (n = 70
    rows over 4 and 8 waves, a ragged last trip)."""
    env, states, args, n_rec = _inputs(
        STEP_SCENES[("DubinsCar", "summed_action_cost")])
    E_max = _full_capacity(n_rec, states.shape[0])
    ref = _reference(env, states, args, n_rec, E_max)
    out, guards = _tail(env, states, args, n_rec, E_max, ref, threads)
    _assert_equal(out, ref)
    _assert_guards(guards)


# ------------------------------------------------------------- edge capacity
@pytest.mark.gpu
def test_tail_edge_capacity_overflow():
    """E_max below the scene's edge count: the true count is reported, the
    first E_max entries match, nothing past E_max is written."""
    env, states, args, n_rec = _inputs(
        STEP_SCENES[("DubinsCar", "summed_action_cost")])
    full = _reference(env, states, args, n_rec,
                      _full_capacity(n_rec, states.shape[0]))
    E = int(full["flags"][0])
    assert E >= 128, "scene must have enough edges to overflow"
    E_max = E // 2 + 1          # odd split inside a receiver row
    ref = _reference(env, states, args, n_rec, E_max)
    assert int(ref["flags"][0]) == E
    out, guards = _tail(env, states, args, n_rec, E_max, ref)
    assert int(out["flags"][0]) == E
    _assert_equal(out, ref, upto=E_max)
    assert torch.equal(out["ei"][:, :E_max], full["ei"][:, :E_max])
    _assert_guards(guards)


def _spread_scene(spacing, n=5):
    agents = {f"a{k}": ks._dub(spacing * k, 0.0, 0.3 * k, 0.3,
                               (spacing * k + 0.5, 0.4))
              for k in range(n)}
    return ks._step_scene("DubinsCar", "spread", agents)


@pytest.mark.gpu
def test_tail_zero_edges():
    """Agents farther apart than comm_radius: every entry is a pad."""
    sc = _spread_scene(5.0)
    cpu_env = _inject(sc, "cpu")
    assert cpu_env.params["comm_radius"] < 4.9
    nxt = ks.ref_step_dubins(sc["states"], sc["goal"], sc["action"])[0]
    linked = cpu_env.add_communication_links(
        cpu_env._build_data(nxt["states"].float()))
    assert linked.num_edges == 0, "CPU reference must give 0 edges"

    env, states, args, n_rec = _inputs(sc)
    N = states.shape[0]
    E_max = _full_capacity(n_rec, N)
    ref = _reference(env, states, args, n_rec, E_max)
    out, guards = _tail(env, states, args, n_rec, E_max, ref)
    _assert_equal(out, ref)
    _assert_guards(guards)
    assert int(out["flags"][0]) == 0
    assert bool((out["ei"] == 0).all()) and bool((out["seg"] == N).all())
    assert bool((out["ea"] == 0).all())
    ptr = ops._csr_ptr(out["seg"], N)
    assert bool((ptr == 0).all())


# --------------------------------------------------------------------- flags
def _reach_scene(all_reach):
    """Agents 3 apart, each 0.06 short of its goal and driving at it with
    v = 0.6: the step covers 0.018, so every agent lands 0.042 from its goal
    (d2g = 0.05, margin 0.008).  ``all_reach=False`` moves one goal away."""
    agents = {}
    for k in range(5):
        th = 0.4 + 0.9 * k
        gx, gy = ks._ang(th, 0.06)
        agents[f"a{k}"] = ks._dub(3.0 * k, 0.0, th, 0.6,
                                  (3.0 * k + gx, gy))
    if not all_reach:
        agents["a3"] = ks._dub(9.0, 0.0, 0.4, 0.6, (9.8, 0.5))
    return ks._step_scene("DubinsCar", "reach", agents)


@pytest.mark.gpu
@pytest.mark.parametrize("all_reach", [True, False])
def test_tail_reach_flag(all_reach):
    sc = _reach_scene(all_reach)
    ref64 = ks.ref_step_dubins(sc["states"], sc["goal"], sc["action"])[0]
    assert bool(ref64["reach"].all()) == all_reach
    assert not bool(ref64["prev_reach"].any())
    env, states, args, n_rec = _inputs(sc)
    E_max = _full_capacity(n_rec, states.shape[0])
    ref = _reference(env, states, args, n_rec, E_max)
    assert int(ref["flags"][1]) == int(all_reach)
    out, guards = _tail(env, states, args, n_rec, E_max, ref)
    _assert_equal(out, ref)
    _assert_guards(guards)


def _unsafe_scene(now):
    """Two head-to-head Dubins cars (r = 0.05) plus three far fillers.
    now=True:  0.09 apart (< 2r) and driving apart at 0.6 each: unsafe at t,
               0.126 apart and heading away at t+1 (no cone): safe.
    now=False: 0.16 apart (outside the 3r warn zone) and closing: safe at t,
               0.124 apart and head-on at t+1: inside the cone, unsafe."""
    if now:
        a = ks._dub(0.0, 0.0, math.pi, 0.6, (-1.0, 0.7))
        b = ks._dub(0.09, 0.0, 0.0, 0.6, (1.0, 1.2))
    else:
        a = ks._dub(0.0, 0.0, 0.0, 0.6, (1.0, 0.7))
        b = ks._dub(0.16, 0.0, math.pi, 0.6, (-1.0, 1.2))
    agents = {"a": a, "b": b}
    for k in range(3):
        agents[f"f{k}"] = ks._dub(4.0 + 2 * k, 0.0, 2.0, 0.3,
                                  (4.5 + 2 * k, 0.8))
    return ks._step_scene("DubinsCar", "unsafe", agents)


@pytest.mark.gpu
@pytest.mark.parametrize("now", [True, False], ids=["at_t", "at_t1"])
def test_tail_unsafe_flag_reads_current_states(now):
    sc = _unsafe_scene(now)
    env, states, args, n_rec = _inputs(sc)
    E_max = _full_capacity(n_rec, states.shape[0])
    ref = _reference(env, states, args, n_rec, E_max)
    # fp64 decisions at t and at t+1 differ, so a mask on the wrong states
    # would flip the flag
    m_t = ks.ref_masks("DubinsCar", sc["states"], 1, 5)[0]["unsafe"]
    m_t1 = ks.ref_masks("DubinsCar", ref["states"].cpu(), 1, 5)[0]["unsafe"]
    assert bool(m_t.any()) == now and bool(m_t1.any()) == (not now)
    assert int(ref["flags"][2]) == int(now)
    out, guards = _tail(env, states, args, n_rec, E_max, ref)
    _assert_equal(out, ref)
    _assert_guards(guards)


# -------------------------------------------------------------- applicability
@pytest.mark.gpu
def test_tail_refuses_scenes_above_its_bound():
    from gcbf_amd import _C
    max_rows, max_nodes = _C.rollout_tail_bounds()
    assert max_rows >= 16 and max_nodes >= 16       # flagship fits
    assert ops.rollout_tail_supported(16, 16)
    assert not ops.rollout_tail_supported(max_rows + 1, max_rows + 1)
    assert not ops.rollout_tail_supported(4, max_nodes + 1)
    n = 4
    N = max_nodes + 1
    dev = "cuda"
    states = torch.zeros(N, 4, device=dev)
    args = ["dubins", states, torch.zeros(n, 4, device=dev),
            torch.zeros(n, 2, device=dev), 0.03, 0.05, 0.8, 0.05, 2.0]
    out = [torch.zeros(N, 4, device=dev), torch.zeros(n, 2, device=dev),
           torch.zeros(n, device=dev),
           torch.zeros(n, dtype=torch.bool, device=dev),
           torch.zeros(n, dtype=torch.bool, device=dev),
           torch.zeros(2, 8, dtype=torch.long, device=dev),
           torch.zeros(8, dtype=torch.long, device=dev),
           torch.zeros(8, 5, device=dev),
           torch.zeros(3, dtype=torch.int32, device=dev)]
    with pytest.raises(RuntimeError, match="bound"):
        ops.rollout_tail(args, n, 1.0, ops.ATTR_DUBINS, 5, 8, out)


# --------------------------------------------------------------- engine level
def _run_engine(tail, monkeypatch, steps=40):
    """40 pinned steps (policy/explore pattern fixed, one reload) of a
    DubinsCar n=16 engine; returns what every step left behind."""
    import numpy as np
    from gcbf_amd.algo import make_algo
    from gcbf_amd.env import make_env
    from gcbf_amd.rollout import RolloutEngine, engine_supported
    from gcbf_amd.trainer.utils import set_seed
    dev = torch.device("cuda")
    set_seed(3)
    env = make_env("DubinsCar", 16, dev)
    env.train()
    algo = make_algo("gcbf", env, 16, env.node_dim, env.edge_dim,
                     env.action_dim, dev, batch_size=512)
    env.reset()
    assert engine_supported(env, algo)
    monkeypatch.setenv("GCBF_AMD_ROLLOUT_TAIL", "1" if tail else "0")
    eng = RolloutEngine(env, algo)
    assert eng._tail == tail
    set_seed(11)
    np.random.seed(7)
    trace = []
    for t in range(steps):
        if t == 20:
            eng.reload()
        # pinned branch: rand() < 0 never, rand() < 1 always
        if eng.step(prob=1.0 if t % 3 == 1 else 0.0):
            eng.reload()
        c, E = eng.cur, eng.E
        trace.append([x.clone() for x in (
            eng.states[c], eng.u_ref[c], eng.reward_buf, eng.reach_buf,
            eng.coll_buf, eng.flags, eng.ei[c][:, :E], eng.ea[c][:E],
            eng.seg[c])])
    ring = getattr(algo, "_ring", None)
    ring_state = None if ring is None else (
        ring.next_id, ring.states[:steps].clone(), ring.uref[:steps].clone())
    return trace, ring_state


@pytest.mark.gpu
def test_engine_tail_equals_multi_kernel_body(monkeypatch):
    names = ("states", "u_ref", "reward", "reach", "coll", "flags", "ei",
             "ea", "seg")
    ref, ring_ref = _run_engine(False, monkeypatch)
    got, ring_got = _run_engine(True, monkeypatch)
    for t, (a, b) in enumerate(zip(ref, got)):
        for name, x, y in zip(names, a, b):
            assert torch.equal(x, y), f"step {t}: {name} differs"
    assert (ring_ref is None) == (ring_got is None)
    if ring_ref is not None:
        assert ring_ref[0] == ring_got[0]
        assert torch.equal(ring_ref[1], ring_got[1])
        assert torch.equal(ring_ref[2], ring_got[2])


# ------------------------------------------------------------------ CPU path
def test_cpu_path_unchanged():
    """On CPU tensors nothing routes through the tail: the env steps through
    its eager path, and without a GPU the captured engine stays
    unsupported."""
    from gcbf_amd.algo import make_algo
    from gcbf_amd.env import make_env
    from gcbf_amd.rollout import engine_supported
    dev = torch.device("cpu")
    env = make_env("DubinsCar", 4, dev)
    env.train()
    algo = make_algo("gcbf", env, 4, env.node_dim, env.edge_dim,
                     env.action_dim, dev, batch_size=8)
    data = env.reset()
    if not torch.cuda.is_available():
        assert not engine_supported(env, algo)
    if not ops.hip_available():
        assert not ops.rollout_tail_supported(4, 4)
    assert ops.env_step_fused(*env.fused_step_args(
        data.states, env._goal, torch.zeros(4, env.action_dim))) is None
    data.update(u_ref=env.u_ref(data))
    nxt, reward, done, info = env.step(algo.step(data, prob=0.5))
    assert nxt.states.shape == data.states.shape
    assert bool(torch.isfinite(nxt.states).all())
