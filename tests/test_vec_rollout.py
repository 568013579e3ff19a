"""VecRolloutEngine: B scenes per rollout step (gcbf_amd/vec_rollout.py).

CPU part: the plain body (the three-call sequence on the eager ops) and all
of the bookkeeping: independent resets, scene-major flush order, safe /
unsafe indices, the trainer's update cadence, the ring's batched push.
GPU part: the captured body against RolloutEngine at B = 1 and against the
plain body at B = 3, and one short vectorized training run.
"""
import numpy as np
import pytest
import torch

from gcbf_amd.algo import make_algo
from gcbf_amd.env import make_env
from gcbf_amd.graph import GraphBatch
from gcbf_amd.trainer.utils import set_seed


# ----------------------------------------------------------------- plumbing
def _setup(env_name, n, dev, batch_size, seed=3, params=None):
    set_seed(seed)
    dev = torch.device(dev)
    if params is not None:
        base = make_env(env_name, n, dev).default_params
        base.update(params)
        params = base
    env = make_env(env_name, n, dev, params=params)
    env.train()
    algo = make_algo("gcbf", env, n, env.node_dim, env.edge_dim,
                     env.action_dim, dev, batch_size=batch_size)
    env.reset()
    return env, algo


def _short_episodes(monkeypatch, env, steps):
    monkeypatch.setattr(type(env), "max_episode_steps",
                        property(lambda self: steps))


def _snap_states(algo, snap):
    """States of a buffered snapshot: its own, or its ring slot."""
    if snap.states is not None:
        return snap.states
    ring = algo._ring
    assert ring.resident(snap.ring_id)
    return ring.states[snap.ring_id % ring.CAP]


def _engine(env, algo, B):
    from gcbf_amd.vec_rollout import VecRolloutEngine
    return VecRolloutEngine(env, algo, B)


# ------------------------------------------------------------ CPU: engine
def test_scenes_reset_independently(monkeypatch):
    """Scene 1 starts with a head start of three steps: it alone is reset
    after step 2, scenes 0 and 2 go on from where they were."""
    runs = []
    for head_start in (3, 0):
        env, algo = _setup("SimpleCar", 3, "cpu", 6)
        _short_episodes(monkeypatch, env, 5)
        eng = _engine(env, algo, 3)
        assert eng.g is None, "CPU runs the plain body"
        eng.t[1] = head_start
        set_seed(11)
        before = eng.states[eng.cur].clone()
        dones = [eng.step(0.5) for _ in range(2)]
        runs.append((eng, before, dones))
    (eng, before, dones), (twin, _, twin_dones) = runs
    assert dones[0].tolist() == [False] * 3
    assert dones[1].tolist() == [False, True, False]
    assert all(not d.any() for d in twin_dones)
    assert eng.t.tolist() == [2, 0, 2] and twin.t.tolist() == [2, 2, 2]
    now, ref = eng.states[eng.cur], twin.states[twin.cur]
    assert torch.equal(now[0], ref[0]) and torch.equal(now[2], ref[2])
    assert not torch.equal(now[1], ref[1]), "scene 1 was not redrawn"
    # the redrawn scene is at rest at fresh positions, its goal and u_ref
    # are the new layout's, the edge buffers were rebuilt around it
    assert bool((now[1][:, 2:] == 0).all())
    assert torch.equal(eng.goal[1], eng.env._goal)
    assert not torch.equal(eng.goal[1], twin.goal[1])
    from gcbf_amd import ops
    flat = now.view(9, -1)
    ei, ea = ops.build_graph(flat[:, :2], flat, None,
                             env.params["comm_radius"], None, 3,
                             env._attr_kind, env.edge_dim, env.edge_attr)
    E = ei.shape[1]
    assert eng.E == E == int(eng.counts.sum())
    assert torch.equal(eng.ei[eng.cur][:, :E], ei)
    assert torch.equal(eng.ea[eng.cur][:E], ea)
    assert bool((eng.seg[eng.cur][E:] == 9).all())


def test_flush_is_scene_major_and_classifies(monkeypatch):
    env, algo = _setup("SimpleCar", 3, "cpu", 6)
    _short_episodes(monkeypatch, env, 5)
    eng = _engine(env, algo, 3)
    eng.t[1] = 3
    set_seed(11)
    T = 7
    seen = []
    for t in range(T):
        if t == 3:
            # two agents of scene 2 closer than 2r: this step is unsafe
            c = eng.cur
            eng.states[c][2, 1, :2] = eng.states[c][2, 0, :2] + 0.03
            eng._rebuild_current()
        seen.append(eng.states[eng.cur].clone())
        eng.step(0.5)
    assert algo.buffer.size == 0, "nothing reaches the buffer before flush"
    assert eng.flush() == 3 * T
    assert eng.flush() == 0
    assert algo.buffer.size == 3 * T
    expect_safe, expect_unsafe = [], []
    for b in range(3):
        for t in range(T):
            idx = b * T + t
            snap = algo.buffer.data[idx]
            assert torch.equal(_snap_states(algo, snap), seen[t][b]), (b, t)
            st = seen[t][b]
            g = GraphBatch(x=torch.zeros_like(st), pos=st[:, :2], states=st)
            unsafe = bool(env.unsafe_mask(g).any())
            (expect_unsafe if unsafe else expect_safe).append(idx)
    assert 2 * T + 3 in expect_unsafe
    algo.buffer._resolve()
    assert sorted(algo.buffer.safe_data) == expect_safe
    assert sorted(algo.buffer.unsafe_data) == expect_unsafe


def test_b1_trajectory_equals_single_scene_loop(monkeypatch):
    """B = 1, fixed seeds: 40 steps, resets included, against the trainer's
    plain single-scene loop."""
    steps = 40
    env, algo = _setup("SimpleCar", 3, "cpu", 64, seed=5)
    _short_episodes(monkeypatch, env, 15)
    set_seed(7)
    data = env.reset()
    ref = []
    n_reset = 0
    for step in range(1, steps + 1):
        if data.u_ref is None:
            data.update(u_ref=env.u_ref(data))
        action = algo.step(data, prob=1 - (step - 1) / steps)
        next_data, reward, done, info = env.step(action)
        next_data.update(u_ref=env.u_ref(next_data))
        algo.post_step(data, action, reward, done, next_data)
        n_reset += int(done)
        data = env.reset() if done else next_data
        ref.append(data.states.clone())
    assert n_reset >= 2

    env, algo = _setup("SimpleCar", 3, "cpu", 64, seed=5)
    set_seed(7)
    env.reset()
    eng = _engine(env, algo, 1)
    for step in range(1, steps + 1):
        eng.step(prob=1 - (step - 1) / steps)
        assert torch.equal(eng.states[eng.cur][0], ref[step - 1]), step


def test_engine_applicability():
    from gcbf_amd.vec_rollout import (vec_engine_supported,
                                      vec_engine_unsupported_reason)
    env, algo = _setup("SimpleCar", 3, "cpu", 6)
    assert vec_engine_supported(env, algo, 3)
    assert not vec_engine_supported(env, algo, 0)
    env.test()
    assert "train" in vec_engine_unsupported_reason(env, algo, 3)
    env.train()
    env._max_neighbors = 2
    assert "neighbour" in vec_engine_unsupported_reason(env, algo, 3)
    env._max_neighbors = None
    # 100 * 52 * 51 > 262144
    big = make_env("SimpleCar", 52, torch.device("cpu"))
    big.train()
    big.reset()
    assert "capacity" in vec_engine_unsupported_reason(big, algo, 100)
    macbf = make_algo("macbf", env, 3, env.node_dim, env.edge_dim,
                      env.action_dim, torch.device("cpu"), batch_size=6)
    assert "MACBF" in vec_engine_unsupported_reason(env, macbf, 3)


# ----------------------------------------------------------- CPU: trainer
def test_trainer_cadence(monkeypatch, tmp_path):
    from gcbf_amd.trainer import Trainer
    from gcbf_amd.vec_rollout import VecRolloutEngine
    env, algo = _setup("SimpleCar", 3, "cpu", 6)
    env_test = make_env("SimpleCar", 3, torch.device("cpu"))
    updates, saves, probs = [], [], []

    def update(step, writer=None):
        updates.append((step, algo.buffer.size))
        algo.memory.merge(algo.buffer)
        algo.buffer.clear()
        return {"acc/safe": 1.0}

    real_step = VecRolloutEngine.step

    def step(self, prob):
        probs.append(prob)
        return real_step(self, prob)

    monkeypatch.setattr(algo, "update", update)
    monkeypatch.setattr(algo, "save", lambda path: saves.append(path))
    monkeypatch.setattr(VecRolloutEngine, "step", step)
    trainer = Trainer(env, env_test, algo, str(tmp_path), num_envs=3)
    trainer.train(15, eval_interval=6, eval_epi=0)
    # step advances 3, 6, 9, 12, 15
    assert probs == [1 - s / 15 for s in (0, 3, 6, 9, 12)]
    assert updates == [(6, 6), (12, 6)]
    assert [p.rsplit("_", 1)[1] for p in saves] == ["6", "12"]
    assert algo.memory.size == 12


def test_trainer_refuses_bad_combinations(tmp_path):
    from gcbf_amd.trainer import Trainer
    env, algo = _setup("SimpleCar", 3, "cpu", 6)
    with pytest.raises(ValueError, match="multiple of"):
        Trainer(env, env, algo, str(tmp_path), num_envs=4)
    with pytest.raises(ValueError, match="untested"):
        Trainer(env, env, algo, str(tmp_path), rank=1, world_size=2,
                num_envs=2)
    Trainer(env, env, algo, str(tmp_path), num_envs=1)


def test_trainer_falls_back_where_unsupported(monkeypatch, tmp_path, capsys):
    from gcbf_amd.trainer import Trainer
    env, algo = _setup("SimpleCar", 3, "cpu", 6)
    env._max_neighbors = 2
    calls = []
    monkeypatch.setattr(algo, "update", lambda step, writer=None: (
        calls.append(step), algo.buffer.clear())[0])
    monkeypatch.setattr(algo, "save", lambda path: None)
    trainer = Trainer(env, env, algo, str(tmp_path), num_envs=3)
    trainer.train(6, eval_interval=6, eval_epi=0, capture=False)
    assert calls == [6]
    assert "vectorized rollout unavailable" in capsys.readouterr().out


# -------------------------------------------------------------- CPU: ring
def test_push_raw_many_wraps_like_push_raw():
    from gcbf_amd.ring import RingStore
    env, _ = _setup("SimpleCar", 3, "cpu", 6)
    a, b = RingStore(env, 5), RingStore(env, 5)
    g = torch.Generator().manual_seed(0)
    states = torch.randn(7, 3, 4, generator=g)
    uref = torch.randn(7, 3, 2, generator=g)
    for k in range(3):
        assert a.push_raw(states[k], uref[k]) == b.push_raw(states[k],
                                                            uref[k])
    # slots 3, 4, 0, 1: wraps at CAP
    ids = a.push_raw_many(states[3:7], uref[3:7])
    one_by_one = [b.push_raw(states[k], uref[k]) for k in range(3, 7)]
    assert ids == one_by_one == [3, 4, 5, 6]
    assert a.next_id == b.next_id == 7
    assert torch.equal(a.states, b.states)
    assert torch.equal(a.uref, b.uref)
    assert torch.equal(a.states[0], states[5])
    # no wrap: one copy
    ids = a.push_raw_many(states[:2], uref[:2])
    assert ids == [7, 8] and torch.equal(a.states[2:4], states[:2])


# ----------------------------------------------------------------- GPU part
@pytest.mark.gpu
@pytest.mark.parametrize("prob", [1.0, 0.5])
def test_b1_equals_rollout_engine(monkeypatch, prob):
    """B = 1 against RolloutEngine from the same seeds over 40 steps across
    one reset."""
    from gcbf_amd.rollout import RolloutEngine, engine_supported
    steps = 40

    def run(vec):
        env, algo = _setup("DubinsCar", 16, "cuda", 512)
        _short_episodes(monkeypatch, env, 25)
        if vec:
            eng = _engine(env, algo, 1)
            assert eng.g is not None, "the captured body must run"
        else:
            assert engine_supported(env, algo)
            eng = RolloutEngine(env, algo)
        set_seed(11)
        trace, n_done = [], 0
        for _ in range(steps):
            done = eng.step(prob)
            if vec:
                done = bool(done[0])
                flags = eng.flags[0]
            else:
                flags = eng.flags
                if done:
                    eng.reload()
            n_done += int(done)
            c = eng.cur
            trace.append((eng.states[c].reshape(16, -1).clone(),
                          eng.u_ref[c].reshape(16, -1).clone(),
                          flags.clone()))
        return trace, n_done

    ref, ref_done = run(False)
    got, got_done = run(True)
    assert ref_done == got_done >= 1
    for t, (a, b) in enumerate(zip(ref, got)):
        for name, x, y in zip(("states", "u_ref", "flags"), a, b):
            assert torch.equal(x, y), f"step {t}: {name} differs"


@pytest.mark.gpu
def test_captured_body_equals_plain_body(monkeypatch):
    """B = 3 with obstacle rows, frozen weights, a mixed gate: 12 steps of
    the captured body against the plain three-call body."""
    def run(tail):
        monkeypatch.setenv("GCBF_AMD_VEC_TAIL", "1" if tail else "0")
        env, algo = _setup("DubinsCar", 8, "cuda", 512,
                           params={"num_obs": 3})
        _short_episodes(monkeypatch, env, 8)
        eng = _engine(env, algo, 3)
        assert (eng.g is not None) == tail
        assert eng.N == 11 and eng.agent_index is not None
        set_seed(11)
        trace, gates = [], []
        for _ in range(12):
            eng.step(0.5)
            gates.append(eng.last_explore.copy())
            c, E = eng.cur, eng.E
            trace.append([x.clone() for x in (
                eng.states[c], eng.u_ref[c], eng.fe, eng.reward_buf,
                eng.reach_buf, eng.coll_buf, eng.ei[c], eng.seg[c],
                eng.ea[c])])
        return trace, np.stack(gates)

    ref, ref_gates = run(False)
    got, got_gates = run(True)
    assert (ref_gates == got_gates).all()
    mixed = (ref_gates.any(axis=1) & ~ref_gates.all(axis=1)).sum()
    assert mixed >= 3, "the gate must be mixed on several steps"
    names = ("states", "u_ref", "flags+count", "reward", "reach", "coll",
             "ei", "seg", "ea")
    for t, (a, b) in enumerate(zip(ref, got)):
        for name, x, y in zip(names, a, b):
            assert torch.equal(x, y), f"step {t}: {name} differs"


@pytest.mark.gpu
def test_vectorized_training_run(monkeypatch, tmp_path):
    """Trainer.train with num_envs = 4 through two updates."""
    from gcbf_amd.trainer import Trainer
    env, algo = _setup("DubinsCar", 8, "cuda", 16)
    env_test = make_env("DubinsCar", 8, torch.device("cuda"))
    logs, usable, sizes = [], [], []
    iter_eager, sample, update = (algo._iter_eager, algo._sample_batch,
                                  algo.update)

    def _iter(graph_list, prof=None):
        logs.append(iter_eager(graph_list, prof))
        return logs[-1]

    def _sample(*a, **k):
        graphs = sample(*a, **k)
        usable.append(algo._ring is not None and algo._ring.usable(graphs)
                      and all(g.states is None for g in graphs))
        return graphs

    def _update(step, writer=None):
        sizes.append((step, algo.buffer.size))
        return update(step, writer)

    monkeypatch.setattr(algo, "_iter_eager", _iter)
    monkeypatch.setattr(algo, "_sample_batch", _sample)
    monkeypatch.setattr(algo, "update", _update)
    monkeypatch.setattr(algo, "save", lambda path: None)
    trainer = Trainer(env, env_test, algo, str(tmp_path), num_envs=4)
    trainer.train(32, eval_interval=32, eval_epi=0)
    assert sizes == [(16, 16), (32, 16)]
    assert algo.memory.size == 32 and algo.buffer.size == 0
    assert len(logs) == 2 * algo.params["inner_iter"]
    assert bool(torch.isfinite(torch.stack(logs)).all())
    assert usable and all(usable)
