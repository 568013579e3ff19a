"""Algorithm-level tests: buffer semantics, GCBF/MACBF update mechanics,
checkpoint round-trip, test-time refinement."""
import os

import numpy as np
import torch

from gcbf_amd.algo import make_algo
from gcbf_amd.algo.buffer import Buffer
from gcbf_amd.env import make_env
from gcbf_amd.graph import GraphBatch
from gcbf_amd.trainer.utils import set_seed


def _tiny_graph(tag: float):
    s = torch.full((3, 4), tag)
    return GraphBatch(x=torch.zeros(3, 4), pos=s[:, :2], states=s)


class TestBuffer:
    def test_append_and_classify(self):
        b = Buffer()
        b.append(_tiny_graph(0), True)
        b.append(_tiny_graph(1), False)
        b.append(_tiny_graph(2), True)
        assert b.size == 3
        assert b.safe_data == [0, 2]
        assert b.unsafe_data == [1]

    def test_segment_sampling_window(self):
        b = Buffer()
        for i in range(20):
            b.append(_tiny_graph(i), i % 2 == 0)
        np.random.seed(0)
        out = b.sample(4, 3)
        # segments are consecutive windows; tags must be consecutive runs
        tags = [float(g.states[0, 0]) for g in out]
        assert len(tags) <= 4 * 3
        assert sorted(tags) == tags  # clamped lb keeps order, no duplicates
        assert len(set(tags)) == len(tags)

    def test_balanced_sampling_draws_both_classes(self):
        b = Buffer()
        for i in range(40):
            b.append(_tiny_graph(i), i < 35)  # 35 safe, 5 unsafe
        import random
        random.seed(0)
        out = b.sample(20, 1, balanced_sampling=True)
        tags = [float(g.states[0, 0]) for g in out]
        n_unsafe = sum(t >= 35 for t in tags)
        assert n_unsafe >= 3  # half the draws target the unsafe list

    def test_merge_and_clear(self):
        a, b = Buffer(), Buffer()
        for i in range(3):
            a.append(_tiny_graph(i), True)
        for i in range(2):
            b.append(_tiny_graph(10 + i), False)
        a.merge(b)
        assert a.size == 5
        assert a.unsafe_data == [3, 4]
        b.clear()
        assert b.size == 0

    def test_max_size_eviction(self):
        b = Buffer()
        b.MAX_SIZE = 5
        for i in range(8):
            b.append(_tiny_graph(i), True)
        assert b.size == 5
        assert float(b.data[0].states[0, 0]) == 3.0
        assert b.safe_data == [0, 1, 2, 3, 4]


def _train_algo(algo_name, env_name="SimpleCar", n=4, steps=48, bs=20,
                max_neighbors=None):
    set_seed(0)
    dev = torch.device("cpu")
    env = make_env(env_name, n, dev, max_neighbors=max_neighbors)
    env.train()
    algo = make_algo(algo_name, env, n, env.node_dim, env.edge_dim,
                     env.action_dim, dev, batch_size=bs)
    data = env.reset()
    for step in range(1, steps + 1):
        data.update(u_ref=env.u_ref(data))
        a = algo.step(data, prob=0.5)
        data, r, done, info = env.step(a)
        if done:
            data = env.reset()
        if algo.is_update(step):
            out = algo.update(step, None)
    return algo, env, data, out


def test_gcbf_update_changes_params():
    algo, env, data, out = _train_algo("gcbf")
    assert set(out) == {"acc/safe", "acc/unsafe", "acc/derivative"}
    # memory rotated in at each update; buffer holds only post-update steps
    assert algo.memory.size > 0
    assert algo.buffer.size == 48 % 20


def test_gcbf_save_load_roundtrip(tmp_path):
    algo, env, data, _ = _train_algo("gcbf")
    d = str(tmp_path / "ckpt")
    algo.save(d)
    assert os.path.exists(os.path.join(d, "cbf.pkl"))
    assert os.path.exists(os.path.join(d, "actor.pkl"))

    set_seed(1)
    algo2 = make_algo("gcbf", env, 4, env.node_dim, env.edge_dim,
                      env.action_dim, torch.device("cpu"), batch_size=8)
    algo2.load(d)
    data.update(u_ref=env.u_ref(data))
    a1 = algo.act(data)
    a2 = algo2.act(data)
    assert torch.allclose(a1, a2, atol=1e-6)


def test_gcbf_apply_refinement_runs():
    algo, env, data, _ = _train_algo("gcbf", steps=24, bs=20)
    env.test()
    data = env.reset()
    data.update(u_ref=env.u_ref(data))
    act = algo.apply(data, rand=30)
    assert act.shape == (4, env.action_dim)
    assert not act.requires_grad


def test_macbf_update_and_apply():
    algo, env, data, out = _train_algo("macbf", max_neighbors=12)
    data.update(u_ref=env.u_ref(data))
    act = algo.apply(data)
    assert act.shape == (4, env.action_dim)


def test_nominal_act_is_zero():
    dev = torch.device("cpu")
    env = make_env("SimpleCar", 4, dev)
    env.test()
    algo = make_algo("nominal", env, 4, env.node_dim, env.edge_dim,
                     env.action_dim, dev)
    data = env.reset()
    data.update(u_ref=env.u_ref(data))
    assert (algo.apply(data) == 0).all()


def test_exploration_prob_zeroes_actions():
    set_seed(0)
    dev = torch.device("cpu")
    env = make_env("SimpleCar", 4, dev)
    env.train()
    algo = make_algo("gcbf", env, 4, env.node_dim, env.edge_dim,
                     env.action_dim, dev, batch_size=8)
    data = env.reset()
    data.update(u_ref=env.u_ref(data))
    a = algo.step(data, prob=1.0)  # always explore -> zero residual
    assert (a == 0).all()
    a = algo.step(data, prob=0.0)  # never -> raw actor output
    assert a.abs().sum() > 0


def test_update_residue_trick_value_uses_relinked_graph():
    """h_dot must incorporate the re-linked residue: check that update runs
    with topology changes between t and t+1 (agents crossing comm radius)."""
    algo, env, data, out = _train_algo("gcbf", env_name="DubinsCar", n=4,
                                       steps=24, bs=20)
    assert np.isfinite(out["acc/derivative"])


def test_hyperparams_table_matches_reference():
    from gcbf_amd.trainer.utils import read_params
    p = read_params("DubinsCar", "gcbf")
    assert p == {"alpha": 1.0, "eps": 0.02, "inner_iter": 10,
                 "loss_action_coef": 0.0001, "loss_unsafe_coef": 1.0,
                 "loss_safe_coef": 1.0, "loss_h_dot_coef": 0.2}
    assert read_params("SimpleCar", "macbf")["loss_h_dot_coef"] == 1.0
    assert read_params("NoSuchEnv", "gcbf") is None


def test_update_engine_not_built_on_cpu():
    """The captured update engine must gate itself off on CPU and leave the
    eager path untouched (on_append hook unset, ring ids absent)."""
    import os
    import torch
    from gcbf_amd.algo import make_algo
    from gcbf_amd.env import make_env
    from gcbf_amd.trainer.utils import set_seed
    set_seed(0)
    dev = torch.device("cpu")
    env = make_env("DubinsCar", 4, dev)
    env.train()
    algo = make_algo("gcbf", env, 4, env.node_dim, env.edge_dim,
                     env.action_dim, dev, batch_size=20)
    data = env.reset()
    os.environ["GCBF_AMD_UPDATE_CAPTURE"] = "1"
    try:
        for step in range(1, 21):
            data.update(u_ref=env.u_ref(data))
            a = algo.step(data, prob=0.5)
            data, r, done, info = env.step(a)
            if done:
                data = env.reset()
            if algo.is_update(step):
                algo.update(step, None)
    finally:
        os.environ.pop("GCBF_AMD_UPDATE_CAPTURE", None)
    assert algo._upd_engine is None
    assert algo._upd_engine_tried
    # the ring batcher MAY hook on_append (it works on CPU); the captured
    # engine must not have been built
    assert (algo.buffer.on_append is None
            or algo.buffer.on_append == getattr(algo._ring, "push", None))


import pytest


@pytest.mark.parametrize("env_name,obs", [("DubinsCar", 0),
                                          ("DubinsCar", 4),
                                          ("SimpleCar", None),
                                          ("SimpleDrone", None)])
def test_ring_batch_matches_from_list(env_name, obs):
    """RingStore.batch must reproduce GraphBatch.from_list exactly on
    sampled training graphs (states, u_ref, edges, attrs), across env
    families and with/without obstacle nodes."""
    import torch
    from gcbf_amd.algo import make_algo
    from gcbf_amd.env import make_env
    from gcbf_amd.graph import GraphBatch
    from gcbf_amd.trainer.utils import set_seed

    set_seed(2)
    dev = torch.device("cpu")
    e0 = make_env(env_name, 8, dev)
    p = e0.default_params
    if obs is not None:
        p["num_obs"] = obs
    env = make_env(env_name, 8, dev, params=p)
    env.train()
    algo = make_algo("gcbf", env, 8, env.node_dim, env.edge_dim,
                     env.action_dim, dev, batch_size=40)
    data = env.reset()
    for step in range(20):   # pre-ring appends (exercise backfill)
        data.update(u_ref=env.u_ref(data))
        a = algo.step(data, prob=0.5)
        data, r, done, info = env.step(a)
        data = env.reset() if done else data
    algo._make_ring()
    assert algo._ring is not None
    for step in range(20):   # post-ring appends (exercise the hook)
        data.update(u_ref=env.u_ref(data))
        a = algo.step(data, prob=0.5)
        data, r, done, info = env.step(a)
        data = env.reset() if done else data

    gl = algo.buffer.sample(8, 3)
    assert algo._ring.usable(gl)
    fast = algo._ring.batch(gl)
    ref = GraphBatch.from_list(gl)
    assert torch.equal(fast.states, ref.states)
    assert torch.equal(fast.u_ref, ref.u_ref)
    assert torch.equal(fast.edge_index, ref.edge_index)
    assert torch.allclose(fast.edge_attr, ref.edge_attr, atol=1e-6)
    assert torch.equal(fast.x, ref.x)
    assert fast.num_graphs == ref.num_graphs
    if ref.agent_mask is not None:
        assert torch.equal(fast.agent_mask, ref.agent_mask)


def test_ring_eviction_falls_back_to_from_list():
    """When replay memory outlives the ring window, sampled graphs may no
    longer be ring-resident; the update must fall back to from_list and
    stay correct."""
    set_seed(4)
    dev = torch.device("cpu")
    env = make_env("DubinsCar", 4, dev)
    env.train()
    algo = make_algo("gcbf", env, 4, env.node_dim, env.edge_dim,
                     env.action_dim, dev, batch_size=20)
    data = env.reset()
    # tiny windows: memory keeps 60 graphs; ring keeps only 30
    algo.memory.MAX_SIZE = 60
    algo._make_ring()  # created empty before any appends

    algo._ring.CAP = 30
    algo._ring.states = algo._ring.states[:30].clone()
    algo._ring.uref = algo._ring.uref[:30].clone()

    out = None
    for step in range(1, 101):
        data.update(u_ref=env.u_ref(data))
        a = algo.step(data, prob=0.5)
        data, r, done, info = env.step(a)
        if done:
            data = env.reset()
        if algo.is_update(step):
            out = algo.update(step, None)
    assert out is not None
    assert all(np.isfinite(v) for v in out.values())
    # appends must have rotated past the ring window (fallback exercised)
    assert algo._ring.next_id > 30


# ---------------------------------------------------------------- cbf_losses

_LOSS_PARAMS = {"alpha": 1.0, "eps": 0.02, "loss_action_coef": 0.001,
                "loss_unsafe_coef": 1.0, "loss_safe_coef": 1.0,
                "loss_h_dot_coef": 0.1}


def _loss_inputs(real=24, pad=8):
    """Random order-1 rows with both mask classes present, followed by pad
    rows of garbage (large values, masks True) that weight 0 must erase."""
    g = torch.Generator().manual_seed(0)
    R = real + pad
    h = torch.randn(R, 1, generator=g)
    h_dot = torch.randn(R, 1, generator=g)
    actions = torch.randn(R, 2, generator=g)
    unsafe = torch.zeros(R, dtype=torch.bool)
    safe = torch.zeros(R, dtype=torch.bool)
    unsafe[:7] = True
    safe[9:real] = True
    for t in (h, h_dot, actions):
        t[real:] = 1e6
    unsafe[real:] = True
    safe[real:] = True
    weight = torch.cat([torch.ones(real), torch.zeros(pad)])
    return h, h_dot, actions, unsafe, safe, weight


def test_cbf_losses_weighted_matches_unweighted():
    """The captured engine's form (weight 1 on real rows, 0 on pad rows)
    equals the eager form on the real rows alone, to the fp32 reordering
    bound for sums of at most 32 terms of order 1."""
    from gcbf_amd.algo.gcbf import cbf_losses
    real = 24
    h, h_dot, actions, unsafe, safe, weight = _loss_inputs(real)
    loss_w, log_w = cbf_losses(h, h_dot, actions, unsafe, safe,
                               _LOSS_PARAMS, weight=weight)
    loss_e, log_e = cbf_losses(h[:real], h_dot[:real], actions[:real],
                               unsafe[:real], safe[:real], _LOSS_PARAMS)
    assert log_w.shape == log_e.shape == (7,)
    assert (log_e[:4] > 0).all()          # every term is exercised
    rtol = 32 * 2.0 ** -23
    torch.testing.assert_close(loss_w, loss_e, rtol=rtol, atol=0)
    torch.testing.assert_close(log_w, log_e, rtol=rtol, atol=0)


@pytest.mark.parametrize("weighted", [False, True])
def test_cbf_losses_empty_mask_fallbacks(weighted):
    """No unsafe (safe) rows: that loss is 0 and that accuracy is 1."""
    from gcbf_amd.algo.gcbf import cbf_losses
    real = 24
    h, h_dot, actions, unsafe, safe, weight = _loss_inputs(real)
    if not weighted:
        h, h_dot, actions, unsafe, safe = (
            t[:real] for t in (h, h_dot, actions, unsafe, safe))
        weight = None
    none = torch.zeros_like(unsafe)
    _, log = cbf_losses(h, h_dot, actions, none, safe, _LOSS_PARAMS,
                        weight=weight)
    assert float(log[0]) == 0.0 and float(log[4]) == 1.0
    _, log = cbf_losses(h, h_dot, actions, unsafe, none, _LOSS_PARAMS,
                        weight=weight)
    assert float(log[1]) == 0.0 and float(log[5]) == 1.0


def test_macbf_degenerate_batch_size():
    """batch_size < 10 collapses the balanced quotas (n//2 draws) to zero
    once there is a replay memory; MACBF must then take the sampler's
    unbalanced fallback instead of batching an empty graph list."""

    class Recorder:
        def __init__(self):
            self.vals = []

        def add_scalar(self, name, val, t):
            self.vals.append(val)

    set_seed(0)
    dev = torch.device("cpu")
    # MACBF's h is per edge: keep every agent in range of the others, so
    # the only degenerate thing about the case is its batch_size
    params = make_env("SimpleCar", 3, dev).default_params
    params["comm_radius"] = 2 * params["area_size"]
    env = make_env("SimpleCar", 3, dev, params=params, max_neighbors=12)
    env.train()
    algo = make_algo("macbf", env, 3, env.node_dim, env.edge_dim,
                     env.action_dim, dev, batch_size=8)
    algo.params = dict(algo.params, inner_iter=1)
    rec = Recorder()
    data = env.reset()
    for step in range(1, 17):       # second update samples with a memory
        data.update(u_ref=env.u_ref(data))
        a = algo.step(data, prob=0.5)
        data, r, done, info = env.step(a)
        if done:
            data = env.reset()
        if algo.is_update(step):
            assert all(g.num_edges > 0 for g in algo.buffer.data)
            out = algo.update(step, rec)
    assert len(rec.vals) == 2 * 7
    assert all(np.isfinite(v) for v in rec.vals)
    assert all(np.isfinite(v) for v in out.values())
