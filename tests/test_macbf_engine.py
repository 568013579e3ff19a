"""Captured rollout engine for MACBF on neighbour-capped scenes (opt-in).

The engine's one-launch tail against its multi-kernel body (bit-equal), the
captured loop against the eager MACBF loop on the same random stream, updates
between replays, and the opt-in plumbing: off by default, off without a GPU.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV, N_AGENTS, CAP = "SimpleCar", 8, 3
# half the default side, so that receivers have more than CAP agents inside
# the comm radius (1.0) and the cap decides the edge list
AREA = 2.0


def _build(dev, batch_size=512, seed=3):
    from gcbf_amd.algo import make_algo
    from gcbf_amd.env import make_env
    from gcbf_amd.trainer.utils import set_seed
    set_seed(seed)
    params = make_env(ENV, N_AGENTS, dev).default_params
    params["area_size"] = AREA
    env = make_env(ENV, N_AGENTS, dev, params=params, max_neighbors=CAP)
    env.train()
    algo = make_algo("macbf", env, N_AGENTS, env.node_dim, env.edge_dim,
                     env.action_dim, dev, batch_size=batch_size)
    return env, algo


def _pin_draws(monkeypatch):
    """np.random.rand() (no arguments: the exploration draw) returns the
    pinned value; calls with a shape keep drawing from the real stream.
    MACBF floors the exploration probability at 0.5, so only the draw pins
    the branch: 0.9 is the policy graph, 0.1 the exploration graph."""
    real = np.random.rand
    pin = {"v": 0.9}
    monkeypatch.setattr(np.random, "rand",
                        lambda *a: real(*a) if a else pin["v"])
    return pin


# ------------------------------------------------------- gpu: tail on vs off
def _run_engine(tail, monkeypatch, steps=24):
    """24 pinned steps (policy/explore pattern fixed, one reload) of a
    SimpleCar n=8 k=3 MACBF engine; returns what every step left behind."""
    from gcbf_amd.rollout import RolloutEngine, engine_supported
    from gcbf_amd.trainer.utils import set_seed
    dev = torch.device("cuda")
    env, algo = _build(dev)
    env.reset()
    assert engine_supported(env, algo, capped=True)
    monkeypatch.setenv("GCBF_AMD_ROLLOUT_TAIL", "1" if tail else "0")
    eng = RolloutEngine(env, algo)
    assert eng._tail == tail and eng.topk == CAP
    assert getattr(algo, "_ring", None) is None
    set_seed(11)
    np.random.seed(7)
    pin = _pin_draws(monkeypatch)
    trace = []
    for t in range(steps):
        if t == steps // 2:
            eng.reload()
        pin["v"] = 0.1 if t % 3 == 1 else 0.9
        if eng.step(prob=0.0):
            eng.reload()
        c, E = eng.cur, eng.E
        trace.append([x.clone() for x in (
            eng.states[c], eng.u_ref[c], eng.reward_buf, eng.reach_buf,
            eng.coll_buf, eng.flags, eng.ei[c][:, :E], eng.ea[c][:E],
            eng.seg[c])])
    stored = [(g.states.clone(), g.edge_index.clone(), g.edge_attr.clone(),
               g.u_ref.clone()) for g in algo.buffer.data]
    return trace, stored, eng


@pytest.mark.gpu
def test_macbf_engine_tail_equals_multi_kernel_body(monkeypatch):
    names = ("states", "u_ref", "reward", "reach", "coll", "flags", "ei",
             "ea", "seg")
    ref, stored_ref, _ = _run_engine(False, monkeypatch)
    got, stored_got, eng = _run_engine(True, monkeypatch)
    for t, (a, b) in enumerate(zip(ref, got)):
        for name, x, y in zip(names, a, b):
            assert torch.equal(x, y), f"step {t}: {name} differs"
    # the cap is live: receivers have more than CAP agents inside the comm
    # radius, and the edge list is shorter than the uncapped one
    capped_steps = 0
    for tr in got:
        p = tr[0][:, :2]
        d = (p[:, None] - p[None]).norm(dim=-1)
        in_radius = int((d < eng.env.params["comm_radius"]).sum()) - N_AGENTS
        assert 0 < tr[6].shape[1] <= in_radius
        capped_steps += tr[6].shape[1] < in_radius
    assert capped_steps >= len(got) // 2
    # tensor-clone snapshots (no ring on a capped env), equal in both runs
    assert len(stored_ref) == len(stored_got) == 24
    for a, b in zip(stored_ref, stored_got):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


# --------------------------------------------- gpu: captured vs eager loop
class _Recorder:
    """Stands in for a captured graph: notes which one was replayed."""

    def __init__(self, graph, key, log):
        self.graph, self.key, self.log = graph, key, log

    def replay(self):
        self.log.append(self.key[0])
        self.graph.replay()


@pytest.mark.gpu
def test_macbf_engine_matches_eager_loop(monkeypatch):
    """Same seeds, same exploration stream, prob = 0.3 (below MACBF's floor
    of 0.5): the trajectories agree and both loops explore on the same
    steps."""
    from gcbf_amd.rollout import RolloutEngine, engine_supported
    dev = torch.device("cuda")
    draws = []
    real = np.random.rand

    def rand(*a):
        v = real(*a)
        if not a:
            draws.append(float(v))
        return v

    monkeypatch.setattr(np.random, "rand", rand)

    # eager loop
    env_a, algo_a = _build(dev)
    data = env_a.reset()
    np.random.seed(7)
    states_a, explore_a = [], []
    for step in range(40):
        if data.u_ref is None:
            data.update(u_ref=env_a.u_ref(data))
        a = algo_a.step(data, prob=0.3)
        explore_a.append(bool((a == 0).all()))
        data, r, done, info = env_a.step(a)
        states_a.append(data.states.clone())
        if done:
            break
    draws_a = list(draws)
    draws.clear()

    # captured loop (same weights by construction: same seed -> same init)
    env_b, algo_b = _build(dev)
    env_b.reset()
    assert not engine_supported(env_b, algo_b)
    assert engine_supported(env_b, algo_b, capped=True)
    eng = RolloutEngine(env_b, algo_b)
    explore_b = []
    eng.g = {k: _Recorder(g, k, explore_b) for k, g in eng.g.items()}
    np.random.seed(7)
    draws.clear()
    states_b = []
    for step in range(len(states_a)):
        done = eng.step(prob=0.3)
        states_b.append(eng.states[eng.cur].clone())
        if done:
            break
    draws_b = list(draws)

    assert len(states_a) == len(states_b)
    worst = max(float((sa - sb).abs().max())
                for sa, sb in zip(states_a, states_b))
    print(f"macbf captured vs eager: {len(states_a)} steps, "
          f"max |dstate| = {worst:.3e}")
    for t, (sa, sb) in enumerate(zip(states_a, states_b)):
        assert torch.allclose(sa, sb, atol=5e-4), \
            (t, (sa - sb).abs().max())
    # one draw per step in both loops, the same stream, the same decisions
    assert len(draws_a) == len(draws_b) == len(states_a)
    assert draws_a == draws_b
    assert explore_a == explore_b == [v < 0.5 for v in draws_a]
    assert any(explore_a) and not all(explore_a)
    # the floor matters: a draw in [0.3, 0.5) explores
    assert any(0.3 <= v < 0.5 for v in draws_a)
    # buffers got the same number of graphs with matching edge counts
    assert algo_a.buffer.size == algo_b.buffer.size
    for ga, gb in zip(algo_a.buffer.data, algo_b.buffer.data):
        assert ga.num_edges == gb.num_edges


# ------------------------------------------- gpu: updates between replays
@pytest.mark.gpu
def test_macbf_engine_update_interleave(monkeypatch):
    """Engine + updates: weights change between replays and the captured
    policy graph picks them up."""
    from gcbf_amd.graph import GraphBatch
    from gcbf_amd.rollout import RolloutEngine
    dev = torch.device("cuda")
    env, algo = _build(dev, batch_size=32, seed=0)
    env.reset()
    eng = RolloutEngine(env, algo)

    def policy_step():
        """One policy replay from the current buffers; restores them."""
        c = eng.cur
        bufs = (eng.states, eng.u_ref, eng.ei, eng.seg, eng.ea)
        saved = [b[c].clone() for b in bufs]
        eng.g[(False, c)].replay()
        nxt = eng.states[1 - c].clone()
        for b, s in zip(bufs, saved):
            b[c].copy_(s)
        return nxt

    def actor_now():
        c = eng.cur
        data = GraphBatch(x=eng.x, pos=eng.states[c][:, :eng.pos_dim],
                          states=eng.states[c], edge_index=eng.ei[c],
                          edge_attr=eng.ea[c], agent_mask=eng.agent_mask,
                          u_ref=eng.u_ref[c])
        data.seg_dst = eng.seg[c]
        with torch.no_grad():
            return algo.actor(data).clone()

    outs, before = [], None
    for step in range(1, 65):
        if eng.step(prob=0.1):
            eng.reload()
        if algo.is_update(step):
            if step == 64:
                assert eng.E > 0
                before = (actor_now(), policy_step())
                assert torch.equal(policy_step(), before[1])   # repeatable
            outs.append(algo.update(step, None))
    assert len(outs) == 2
    for out in outs:
        assert out and all(np.isfinite(v) for v in out.values()), out
    # same inputs, updated weights: the actor and the captured policy graph
    # both give something else
    assert not torch.equal(actor_now(), before[0])
    assert not torch.equal(policy_step(), before[1])


# ------------------------------------------------------ CPU: applicability
def test_engine_supported_is_opt_in_and_needs_a_gpu():
    from gcbf_amd.rollout import engine_supported
    env, algo = _build(torch.device("cpu"), batch_size=6)
    env.reset()
    assert not engine_supported(env, algo)
    if not torch.cuda.is_available():
        assert not engine_supported(env, algo, capped=True)


def test_trainer_capture_capped_falls_back_on_cpu(monkeypatch, tmp_path):
    from gcbf_amd.trainer import Trainer
    env, algo = _build(torch.device("cpu"), batch_size=6)
    calls = []
    monkeypatch.setattr(algo, "update", lambda step, writer=None: (
        calls.append((step, algo.buffer.size)), algo.buffer.clear())[0])
    monkeypatch.setattr(algo, "save", lambda path: None)
    assert Trainer(env, env, algo, str(tmp_path)).capture_capped is False
    trainer = Trainer(env, env, algo, str(tmp_path), capture_capped=True)
    assert trainer.capture_capped is True
    assert trainer._make_engine() is None
    trainer.train(6, eval_interval=6, eval_epi=0)
    assert calls == [(6, 6)]


def test_train_cli_lists_capture_capped():
    res = subprocess.run(
        [sys.executable, os.path.join(REPO, "train.py"), "--help"],
        cwd=REPO, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "--capture-capped" in res.stdout
