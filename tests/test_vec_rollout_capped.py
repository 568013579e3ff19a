"""VecRolloutEngine with a neighbour cap and with MACBF (``capped=True``).

CPU part: applicability, the plain body at B = 1 against the eager MACBF
loop, MACBF's exploration floor, full-tensor snapshots under the cap, flush
order, one real MACBF update over a flushed buffer, and the trainer's
opt-in.  GPU part: the captured body against the plain body, and the actor
glue switch, bit for bit.
"""
import numpy as np
import pytest
import torch

from gcbf_amd.algo import make_algo
from gcbf_amd.env import make_env
from gcbf_amd.graph import GraphBatch
from gcbf_amd.trainer.utils import set_seed

# smaller areas than the default, so that agents are in each other's comm
# radius.  SimpleCar n = 3 under k = 2 takes the capped code path (k < N)
# but has at most two senders per row, so only the scenes with obstacle
# rows (N = 6) can lose edges to the cap; where they can, the tests require
# that they do
CAR = dict(env_name="SimpleCar", n=3, k=2, params={"area_size": 1.0})
DUBINS = dict(env_name="DubinsCar", n=3, k=2,
              params={"num_obs": 3, "area_size": 1.5})


# ----------------------------------------------------------------- plumbing
def _setup(env_name, n, k, dev, batch_size, algo_name="macbf", seed=3,
           params=None):
    set_seed(seed)
    dev = torch.device(dev)
    base = make_env(env_name, n, dev).default_params
    base.update(params or {})
    env = make_env(env_name, n, dev, params=base, max_neighbors=k)
    env.train()
    algo = make_algo(algo_name, env, n, env.node_dim, env.edge_dim,
                     env.action_dim, dev, batch_size=batch_size)
    env.reset()
    return env, algo


def _short_episodes(monkeypatch, env, steps):
    monkeypatch.setattr(type(env), "max_episode_steps",
                        property(lambda self: steps))


def _engine(env, algo, B, capped=True):
    from gcbf_amd.vec_rollout import VecRolloutEngine
    return VecRolloutEngine(env, algo, B, capped=capped)


def _links(env, eng, states):
    """The env's own builder (under its cap) on one scene's states."""
    data = GraphBatch(x=eng.x1, pos=states[:, :eng.pos_dim], states=states,
                      agent_mask=eng.am1)
    if eng.am1 is not None:
        data.agents_first_n = eng.n
    return env.add_communication_links(data)


def _uncapped_edges(env, eng, states):
    from gcbf_amd import ops
    return ops.dense_radius_graph(states[:, :eng.pos_dim].cpu(),
                                  None if eng.am1 is None else eng.am1.cpu(),
                                  env.params["comm_radius"], None).shape[1]


# ------------------------------------------------------- CPU: applicability
def test_applicability_defaults_unchanged_and_opt_in():
    from gcbf_amd.vec_rollout import (VecRolloutEngine, vec_engine_supported,
                                      vec_engine_unsupported_reason)
    env, macbf = _setup(dev="cpu", batch_size=6, **CAR)
    gcbf = make_algo("gcbf", env, 3, env.node_dim, env.edge_dim,
                     env.action_dim, torch.device("cpu"), batch_size=6)
    # defaults: the reasons and their wording stay
    assert vec_engine_unsupported_reason(env, macbf, 3) == \
        "only GCBF collects vectorized (MACBF is out of scope)"
    assert vec_engine_unsupported_reason(env, gcbf, 3) == \
        "neighbour-capped scenes are not supported"
    assert not vec_engine_supported(env, macbf, 3)
    assert not vec_engine_supported(env, gcbf, 3, capped=False)
    with pytest.raises(NotImplementedError, match="MACBF"):
        VecRolloutEngine(env, macbf, 3)
    # opt-in: MACBF + cap and GCBF + cap
    assert vec_engine_unsupported_reason(env, macbf, 3, capped=True) is None
    assert vec_engine_supported(env, gcbf, 3, capped=True)
    # MACBF without a cap, too
    env._max_neighbors = None
    assert vec_engine_supported(env, macbf, 3, capped=True)
    assert "MACBF" in vec_engine_unsupported_reason(env, macbf, 3)
    env._max_neighbors = 2
    # the other checks still apply
    assert "at least one" in vec_engine_unsupported_reason(
        env, macbf, 0, capped=True)
    env.test()
    assert "train" in vec_engine_unsupported_reason(env, macbf, 3,
                                                    capped=True)
    env.train()
    # 100 * 52 * 51 > 262144
    big = make_env("SimpleCar", 52, torch.device("cpu"), max_neighbors=12)
    big.train()
    big.reset()
    assert "capacity" in vec_engine_unsupported_reason(big, macbf, 100,
                                                       capped=True)


def test_engine_reads_the_cap_once():
    env, algo = _setup(dev="cpu", batch_size=6, **CAR)
    eng = _engine(env, algo, 2)
    assert eng.topk == 2 and eng.g is None
    assert getattr(algo, "_ring", None) is None, "no ring for MACBF"
    env._max_neighbors = None
    free = _engine(env, algo, 2)
    assert free.topk == -1


# ------------------------------------------- CPU: B = 1 against eager loop
@pytest.mark.parametrize("cfg", [CAR, DUBINS],
                         ids=["SimpleCar", "DubinsCar-obstacles"])
def test_b1_macbf_equals_eager_loop(monkeypatch, cfg):
    """B = 1, fixed seeds: 40 steps, resets included, against the trainer's
    plain single-scene loop of MACBF.step + env.step, state for state."""
    steps = 40
    env, algo = _setup(dev="cpu", batch_size=64, seed=5, **cfg)
    _short_episodes(monkeypatch, env, 15)
    set_seed(7)
    data = env.reset()
    ref, n_reset, capped_steps = [], 0, 0
    for step in range(1, steps + 1):
        if data.u_ref is None:
            data.update(u_ref=env.u_ref(data))
        action = algo.step(data, prob=1 - (step - 1) / steps)
        next_data, reward, done, info = env.step(action)
        next_data.update(u_ref=env.u_ref(next_data))
        algo.post_step(data, action, reward, done, next_data)
        n_reset += int(done)
        data = env.reset() if done else next_data
        ref.append((data.states.clone(), data.edge_index.clone()))
    assert n_reset >= 2
    eager_edges = [g.num_edges for g in algo.buffer.data]

    env, algo = _setup(dev="cpu", batch_size=64, seed=5, **cfg)
    set_seed(7)
    env.reset()
    eng = _engine(env, algo, 1)
    for step in range(1, steps + 1):
        eng.step(prob=1 - (step - 1) / steps)
        c = eng.cur
        assert torch.equal(eng.states[c][0], ref[step - 1][0]), step
        assert torch.equal(eng.ei[c][:, :eng.E], ref[step - 1][1]), step
        capped_steps += eng.E < _uncapped_edges(env, eng, eng.states[c][0])
    if eng.N - 1 > cfg["k"]:
        assert capped_steps >= 5, "the cap must decide some edge lists"
    assert eng.flush() == steps
    assert [g.num_edges for g in algo.buffer.data] == eager_edges


# ------------------------------------------------ CPU: exploration floor
def test_macbf_floor_reaches_the_gate(monkeypatch):
    """prob = 0.0 and every draw 0.4: below MACBF's floor of 0.5, so every
    MACBF scene explores; a GCBF engine given the same draw does not."""
    engines = {}
    for name in ("macbf", "gcbf"):
        env, algo = _setup(dev="cpu", batch_size=6, algo_name=name, **CAR)
        engines[name] = _engine(env, algo, 3)
    calls = []

    def rand(*shape):
        calls.append(shape)
        return np.full(shape, 0.4) if shape else 0.4

    monkeypatch.setattr(np.random, "rand", rand)
    for eng in engines.values():
        eng.step(0.0)
    assert calls == [(3,), (3,)], "one draw per scene and step"
    assert engines["macbf"].last_explore.tolist() == [True] * 3
    assert engines["gcbf"].last_explore.tolist() == [False] * 3
    assert engines["macbf"].explore.tolist() == [1, 1, 1]
    assert engines["gcbf"].explore.tolist() == [0, 0, 0]


# ------------------------------------------- CPU: snapshots and flush order
@pytest.mark.parametrize("cfg", [CAR, DUBINS],
                         ids=["SimpleCar", "DubinsCar-obstacles"])
def test_snapshots_are_full_scene_local_and_capped(monkeypatch, cfg):
    env, algo = _setup(dev="cpu", batch_size=6, **cfg)
    _short_episodes(monkeypatch, env, 5)
    B, T = 3, 7
    eng = _engine(env, algo, B)
    eng.t[1] = 3                      # scene 1 resets early
    set_seed(11)
    seen = []
    for t in range(T):
        seen.append((eng.states[eng.cur].clone(), eng.u_ref[eng.cur].clone()))
        eng.step(0.5)
    assert algo.buffer.size == 0, "nothing reaches the buffer before flush"
    assert eng.flush() == B * T and eng.flush() == 0
    assert algo.buffer.size == B * T
    N, live = eng.N, 0
    for b in range(B):
        for t in range(T):
            # scene-major, each scene's steps in time order
            snap = algo.buffer.data[b * T + t]
            st, ur = seen[t][0][b], seen[t][1][b]
            assert snap.states is not None and snap.edge_index is not None
            assert getattr(snap, "ring_id", None) is None
            assert torch.equal(snap.states, st), (b, t)
            assert torch.equal(snap.pos, st[:, :eng.pos_dim])
            assert torch.equal(snap.u_ref, ur)
            assert torch.equal(snap.x, eng.x1)
            ei = snap.edge_index
            if ei.numel():
                assert int(ei.min()) >= 0 and int(ei.max()) < N
                assert int(ei[1].max()) < eng.n_rec
            want = _links(env, eng, st)
            assert torch.equal(ei, want.edge_index), (b, t)
            assert torch.equal(snap.edge_attr, want.edge_attr), (b, t)
            live += ei.shape[1] < _uncapped_edges(env, eng, st)
    if N - 1 > cfg["k"]:
        assert live >= 3, "the cap must decide some snapshots' edge lists"


# ------------------------------------------------------- CPU: real update
def test_macbf_update_over_a_flushed_buffer():
    env, algo = _setup(dev="cpu", batch_size=10, **CAR)
    eng = _engine(env, algo, 2)
    set_seed(11)
    for _ in range(5):
        eng.step(0.5)
    assert eng.flush() == 10
    out = algo.update(10, None)
    assert out and all(np.isfinite(v) for v in out.values()), out


# ----------------------------------------------------------- CPU: trainer
def _cadence(monkeypatch, tmp_path, capture_capped):
    from gcbf_amd.trainer import Trainer
    env, algo = _setup(dev="cpu", batch_size=6, **CAR)
    env_test = make_env("SimpleCar", 3, torch.device("cpu"), max_neighbors=2)
    updates = []

    def update(step, writer=None):
        updates.append((step, algo.buffer.size))
        algo.memory.merge(algo.buffer)
        algo.buffer.clear()
        return {"acc/safe": 1.0}

    monkeypatch.setattr(algo, "update", update)
    monkeypatch.setattr(algo, "save", lambda path: None)
    trainer = Trainer(env, env_test, algo, str(tmp_path), num_envs=3,
                      capture_capped=capture_capped)
    trainer.train(15, eval_interval=6, eval_epi=0, capture=False)
    return updates, algo


def test_trainer_takes_the_vectorized_path_with_capture_capped(
        monkeypatch, tmp_path, capsys):
    updates, algo = _cadence(monkeypatch, tmp_path, True)
    out = capsys.readouterr().out
    assert "vectorized rollout engine active (3 scenes" in out
    assert "unavailable" not in out
    # step advances 3, 6, 9, 12, 15
    assert updates == [(6, 6), (12, 6)]
    assert algo.memory.size == 12


def test_trainer_falls_back_without_capture_capped(monkeypatch, tmp_path,
                                                   capsys):
    updates, algo = _cadence(monkeypatch, tmp_path, False)
    out = capsys.readouterr().out
    assert "vectorized rollout unavailable" in out and "MACBF" in out
    assert "engine active" not in out
    # the single-scene loop: one update per batch_size steps
    assert updates == [(6, 6), (12, 6)]


# ----------------------------------------------------------------- GPU part
GPU_CASES = [
    dict(env_name="SimpleCar", n=4, k=2, B=3, params={"area_size": 1.0}),
    dict(env_name="DubinsCar", n=3, k=2, B=2,
         params={"num_obs": 3, "area_size": 1.5}),
]
NAMES = ("states", "u_ref", "flags+count", "reward", "reach", "coll", "ei",
         "seg", "ea")


def _run(monkeypatch, cfg, tail, glue, steps=20):
    cfg = dict(cfg)
    B = cfg.pop("B")
    monkeypatch.setenv("GCBF_AMD_VEC_TAIL", "1" if tail else "0")
    monkeypatch.setenv("GCBF_AMD_ACTOR_GLUE", "1" if glue else "0")
    from gcbf_amd.utils.amp import enable_bf16
    env, algo = _setup(dev="cuda", batch_size=512, **cfg)
    enable_bf16(algo)       # the library-GEMM plans the actor glue needs
    _short_episodes(monkeypatch, env, 8)
    eng = _engine(env, algo, B)
    assert (eng.g is not None) == tail
    assert eng._glue == glue and eng.topk == cfg["k"]
    assert getattr(algo, "_ring", None) is None
    set_seed(11)
    trace, gates, dones, live = [], [], 0, 0
    for _ in range(steps):
        dones += int(eng.step(0.0).sum())
        gates.append(eng.last_explore.copy())
        c, E = eng.cur, eng.E
        # real-edge prefix only; everything past it is pad
        assert bool((eng.seg[c][E:] == B * eng.N).all())
        trace.append([x.clone() for x in (
            eng.states[c], eng.u_ref[c], eng.fe, eng.reward_buf,
            eng.reach_buf, eng.coll_buf, eng.ei[c][:, :E], eng.seg[c][:E],
            eng.ea[c][:E])])
        for b in range(B):
            live += int(eng.counts[b]) < _uncapped_edges(
                env, eng, eng.states[c][b])
    eng.flush()
    stored = [(g.states.clone(), g.edge_index.clone(), g.edge_attr.clone(),
               g.u_ref.clone()) for g in algo.buffer.data]
    return trace, np.stack(gates), dones, live, stored, eng


def _assert_traces_equal(ref, got):
    for t, (a, b) in enumerate(zip(ref, got)):
        for name, x, y in zip(NAMES, a, b):
            assert torch.equal(x, y), f"step {t}: {name} differs"


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", GPU_CASES,
                         ids=["SimpleCar-B3", "DubinsCar-obstacles-B2"])
def test_captured_body_equals_plain_body_capped_macbf(monkeypatch, cfg):
    """MACBF under a cap of 2: ~20 steps of the captured body against the
    plain three-call body under one seed, per-scene resets included.  prob
    is 0.0, so the gate is MACBF's floor alone: mixed on several steps."""
    ref, ref_gates, ref_dones, _, ref_stored, _ = _run(
        monkeypatch, cfg, tail=False, glue=True)
    got, got_gates, got_dones, live, got_stored, eng = _run(
        monkeypatch, cfg, tail=True, glue=True)
    assert (ref_gates == got_gates).all()
    mixed = (ref_gates.any(axis=1) & ~ref_gates.all(axis=1)).sum()
    assert mixed >= 3, "the gate must be mixed on several steps"
    assert ref_dones == got_dones >= cfg["B"], "every scene must reset"
    assert live >= 5, "the cap must decide some scenes' edge lists"
    _assert_traces_equal(ref, got)
    # full-tensor snapshots with scene-local ids, equal in both runs
    assert len(ref_stored) == len(got_stored) == 20 * cfg["B"]
    for a, b in zip(ref_stored, got_stored):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        if b[1].numel():
            assert 0 <= int(b[1].min()) and int(b[1].max()) < eng.N


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", GPU_CASES,
                         ids=["SimpleCar-B3", "DubinsCar-obstacles-B2"])
def test_actor_glue_switch_changes_nothing_capped_macbf(monkeypatch, cfg):
    """GCBF_AMD_ACTOR_GLUE 0 against 1 on the captured engine: the switch
    changes the actor path only and that path is bit-equal, so the whole
    trajectory is.  The glue must really apply to the batch layouts
    (agent_index rows for B > 1 with obstacle rows; no mask for SimpleCar)."""
    off, off_gates, _, _, _, _ = _run(monkeypatch, cfg, tail=True,
                                      glue=False)
    on, on_gates, _, _, _, eng = _run(monkeypatch, cfg, tail=True, glue=True)
    assert (off_gates == on_gates).all()
    _assert_traces_equal(off, on)
    data = eng._graph(eng.cur)
    nm = data.agent_index if data.agent_index is not None \
        else data.agents_first_n if data.agents_first_n is not None \
        else data.agent_mask
    if cfg["env_name"] == "SimpleCar":
        assert nm is None
    else:
        assert nm is eng.agent_index and nm.dtype == torch.long
    with torch.no_grad():
        assert eng.algo.actor._glue_applies(data, nm)
        data.actor_glue = False
        assert not eng.algo.actor._glue_applies(data, nm)
