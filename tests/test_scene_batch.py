"""SceneBatch, eval_ctrl_batched and the policies on a scene batch against
the single-scene env and eval_ctrl_epi.

CPU cases: n = 4, B = 3, fp32, distinct seeds, small arenas so that every
episode ends by reach well before the step limit and at different lengths
(which exercises the ``active`` mask).  On the CPU the batched oracle
evaluates the env's own formulas op for op, so trajectories are expected to
agree to the bit; the bound is the project's atol all the same.
"""
import pytest
import torch

from gcbf_amd.algo import make_algo
from gcbf_amd.env import SceneBatch, make_env
from gcbf_amd.graph import GraphBatch
from gcbf_amd.trainer.utils import eval_ctrl_batched, eval_ctrl_epi, set_seed

ATOL = {"states": 1e-5, "u_ref": 1e-4, "reward": 1e-4}
SEEDS = [1, 2, 3]
# env, area_size, num_obs
CASES = [("SimpleCar", 1.0, None), ("DubinsCar", 1.0, 3),
         ("SimpleDrone", 0.6, None)]
IDS = [c[0] for c in CASES]


def _env(name, area, num_obs, n=4, dev="cpu", device_reset=None):
    dev = torch.device(dev)
    params = make_env(name, n, dev).default_params
    params["area_size"] = area
    if num_obs is not None:
        params["num_obs"] = num_obs
    env = make_env(name, n, dev, params=params, device_reset=device_reset)
    env.train()
    return env


def _algo(name, env):
    return make_algo(name, env, env.num_agents, env.node_dim, env.edge_dim,
                     env.action_dim, env.device)


def _single(env, batch, b):
    """Point the env at scene b alone; returns its linked single graph."""
    n = env.num_agents
    env._goal = batch.goal[b]
    env._obs = None if env._step_kind == "car" else batch.states[b, n:]
    data = env.add_communication_links(
        env._build_data(batch.states[b, :n]))
    return data.update(u_ref=env.u_ref(data))


def _compare_eval(env, algo, seeds):
    seq = [eval_ctrl_epi(algo.apply, env, s, make_video=False, verbose=False)
           for s in seeds]
    rew, length, info = eval_ctrl_batched(
        algo.apply, env, seeds, verbose=False, return_states=True)
    assert length == [s[1] for s in seq]
    # ended by reach, and not all at the same step
    assert max(length) < env.max_episode_steps and len(set(length)) > 1
    for key in ("safe", "reach", "success"):
        assert info[key] == [s[3][key] for s in seq], key
    for b, s in enumerate(seq):
        assert info["states"][b].shape == s[3]["states"].shape
        err = (info["states"][b] - s[3]["states"]).abs().max().item()
        assert err <= ATOL["states"], f"scene {b}: trajectory off by {err}"
        assert abs(rew[b] - s[0]) <= ATOL["reward"] * length[b]


# ----------------------------------------------------------------------- CPU
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reset_is_three_seeded_env_resets(case):
    env = _env(*case)
    batch = SceneBatch(env, 3)
    batch.reset(SEEDS)
    n = env.num_agents
    for b, seed in enumerate(SEEDS):
        set_seed(seed)
        data = env.reset()
        assert torch.equal(batch.states[b], data.states)   # agents + obstacles
        assert torch.equal(batch.goal[b], env._goal)
        if env._obs is not None:
            assert torch.equal(batch.states[b, n:], env._obs)
    assert batch.data.num_graphs == 3
    assert bool(batch.active.all()) and not bool(batch.t.any())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_eval_ctrl_batched_matches_sequential(case):
    env = _env(*case)
    _compare_eval(env, _algo("nominal", env), SEEDS)


def test_max_steps_caps_the_episodes():
    env = _env(*CASES[0])
    rew, length, info = eval_ctrl_batched(
        _algo("nominal", env).apply, env, SEEDS, verbose=False, max_steps=7,
        return_states=True)
    assert length == [7.0, 7.0, 7.0]
    assert [s.shape[0] for s in info["states"]] == [7, 7, 7]


def test_box_world_modes_are_refused():
    env = _env(*CASES[1])
    for idx in (0, 1, 3):
        env.demo(idx)
        with pytest.raises(NotImplementedError):
            SceneBatch(env, 2)
    env.demo(2)
    SceneBatch(env, 2)


def _batch_with_reached_agent(env):
    """Three scenes, every agent moving, agent 1 of scene 1 on its goal."""
    batch = SceneBatch(env, 3)
    batch.reset(SEEDS)
    n, p = env.num_agents, env.pos_dim
    torch.manual_seed(0)
    batch.states[:, :n, p:] = torch.rand_like(batch.states[:, :n, p:]) * 0.5
    batch.goal[1, 1, :p] = batch.states[1, 1, :p]
    batch.data = batch._link(batch.states)
    return batch


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_graph_inside_scenes_is_per_scene(case):
    env = _env(*case)
    batch = _batch_with_reached_agent(env)
    n, N = env.num_agents, batch.nodes_per_scene
    action = torch.randn(3 * n, env.action_dim) * 0.3
    with batch.scenes():
        out = env.forward_graph(batch.data, action)
        u_ref = env.u_ref(batch.data)
    assert env._scenes == 1 and env._live_rows is None      # context undone
    parts = out.to_list()
    for b in range(3):
        data = _single(env, batch, b)
        one = env.forward_graph(data, action[b * n:(b + 1) * n])
        assert torch.equal(parts[b].edge_index, one.edge_index)
        assert (parts[b].states - one.states).abs().max() <= 1e-6
        assert (parts[b].edge_attr - one.edge_attr).abs().max() <= 1e-6
        assert (u_ref[b * n:(b + 1) * n] - env.u_ref(data)).abs().max() \
            <= ATOL["u_ref"]
    if env._step_kind != "car":   # the reached agent is frozen in the batch
        assert torch.equal(out.states[N + 1], batch.states[1, 1])
        assert not torch.equal(out.states[N], batch.states[1, 0])


@pytest.mark.parametrize("case", CASES[1:], ids=IDS[1:])
def test_batches_outside_scenes_stay_unfrozen(case):
    env = _env(*case)
    batch = _batch_with_reached_agent(env)
    graphs = [_single(env, batch, b) for b in (0, 1)]   # env now at scene 1
    p = env.pos_dim
    assert (graphs[1].states[1, :p] - env._goal[1, :p]).norm() \
        < env.params["dist2goal"]
    two = GraphBatch.from_list(graphs)
    N = batch.nodes_per_scene
    out = env.forward_graph(two, torch.zeros(2 * env.num_agents,
                                             env.action_dim))
    # update-path batches are not frozen: the reached agent moves on
    assert not torch.equal(out.states[N + 1, :p], two.states[N + 1, :p])
    # while the env's own single graph freezes it
    one = env.forward_graph(graphs[1], torch.zeros(env.num_agents,
                                                   env.action_dim))
    assert torch.equal(one.states[1], graphs[1].states[1])


def _ok_mask(env, algo, data):
    """The fallback mask of GCBF.apply: agents whose h-dot condition holds
    under the nominal action."""
    with torch.no_grad():
        h = algo.cbf(data)
        nxt = env.forward_graph(data, torch.zeros(
            h.shape[0], env.action_dim, dtype=h.dtype))
        h_dot = (algo.cbf(nxt) - h) / env.dt
        return (torch.relu(-h_dot - algo.params["alpha"] * h)[:, 0] <= 0)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gcbf_apply_on_scene_batch(case):
    """Batched fp32 GCBF.apply (rand=0, random-init networks).  The stack
    does not run in fp64 unchanged (the spectral-norm power iteration of
    nn/mlp.py casts to fp32), so there is no fp64 yardstick for the
    actions: this checks the fallback mask ``ok`` against the per-scene one
    and that the actions are finite, and prints the difference to the
    per-scene fp32 apply.  forward_graph parity is covered above.  The
    networks are put in eval mode so that the spectral-norm vectors do not
    advance between the batched and the per-scene calls."""
    env = _env(*case)
    torch.manual_seed(5)
    algo = _algo("gcbf", env)
    algo.cbf.eval()
    algo.actor.eval()
    batch = SceneBatch(env, 3)
    batch.reset(SEEDS)
    n = env.num_agents
    with batch.scenes():
        got = algo.apply(batch.data, rand=0)
        ok_batched = _ok_mask(env, algo, batch.data)
    assert got.shape == (3 * n, env.action_dim)
    assert torch.isfinite(got).all()
    one, ok = [], []
    for b in range(3):
        data = _single(env, batch, b)
        one.append(algo.apply(data, rand=0))
        ok.append(_ok_mask(env, algo, data))
    assert torch.equal(ok_batched, torch.cat(ok))
    print(f"\n{case[0]}: batched vs per-scene fp32 apply, largest "
          f"difference {(got - torch.cat(one)).abs().max().item():.3e}; "
          f"ok {ok_batched.tolist()}")


def test_gcbf_apply_leaves_finished_scenes_alone():
    env = _env(*CASES[0])
    torch.manual_seed(5)
    algo = _algo("gcbf", env)
    algo.cbf.eval()
    algo.actor.eval()
    batch = SceneBatch(env, 3)
    batch.reset(SEEDS)
    n = env.num_agents
    batch.active[1] = 0
    with batch.scenes():
        got = algo.apply(batch.data, rand=0)
    # a finished scene falls back to the nominal action and is not refined
    assert (got[n:2 * n] == 0).all()


def test_macbf_and_nominal_accept_a_scene_batch():
    env = _env("SimpleCar", 1.0, None)
    batch = SceneBatch(env, 3)
    batch.reset(SEEDS)
    for name in ("nominal", "macbf"):
        algo = _algo(name, env)
        with batch.scenes():
            got = algo.apply(batch.data)
        one = torch.cat([algo.apply(_single(env, batch, b))
                         for b in range(3)])
        assert got.shape == one.shape
        assert (got - one).abs().max() <= 1e-4


# ----------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_gpu_eval_ctrl_batched_matches_sequential():
    env = _env("DubinsCar", 1.0, 3, n=5, dev="cuda")
    _compare_eval(env, _algo("nominal", env), SEEDS)


@pytest.mark.gpu
def test_gpu_scene_batch_step_with_gcbf_actor():
    env = _env("DubinsCar", 1.0, 3, n=5, dev="cuda")
    torch.manual_seed(5)
    algo = _algo("gcbf", env)
    batch = SceneBatch(env, 3)
    data = batch.reset(SEEDS)
    n = env.num_agents
    start = batch.states.clone()
    action = algo.act(data)
    _, reward, done, info = batch.step(action)
    for b, seed in enumerate(SEEDS):
        set_seed(seed)
        one = env.reset()
        assert torch.equal(one.states, start[b])
        one.update(u_ref=env.u_ref(one))
        act_one = algo.act(one)
        assert (act_one - action[b * n:(b + 1) * n]).abs().max() <= 1e-4
        nxt, rew_one, done_one, info_one = env.step(act_one)
        assert torch.equal(info["reach"][b], info_one["reach"])
        assert torch.equal(info["collision"][b], info_one["collision"])
        assert bool(done[b]) == done_one
        assert (batch.states[b] - nxt.states).abs().max() <= ATOL["states"]
        assert (reward[b] - rew_one).abs().max() <= ATOL["reward"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["SimpleCar", "DubinsCar", "SimpleDrone"])
def test_gpu_device_reset_of_a_scene_batch(name):
    n, B = 16, 3
    env = _env(name, 4.0 if name != "SimpleDrone" else 2.0,
               8 if name == "DubinsCar" else None, n=n, dev="cuda",
               device_reset=True)
    batch = SceneBatch(env, B)
    batch.reset(SEEDS)
    p, r = env.pos_dim, env.agent_radius
    starts = batch.states[:, :n, :p].cpu()
    goals = batch.goal[..., :p].cpu()
    obs = batch.states[:, n:, :p].cpu()
    assert starts.shape == (B, n, p) and goals.shape == (B, n, p)   # count
    goal_sep = 5 * r if name == "DubinsCar" else 4 * r
    side = env.params["area_size"]
    for b in range(B):
        for pts, sep in ((starts[b], 4 * r), (goals[b], goal_sep)):
            assert ((pts >= 0) & (pts < side)).all()
            d = torch.cdist(pts.double(), pts.double())
            d.fill_diagonal_(float("inf"))
            assert d.min() > sep
            assert pts.norm(dim=1).min() > sep          # the origin quirk
            if obs.shape[1]:
                clearance = 2 * r + 2 * env.params["obs_point_r"]
                assert torch.cdist(pts.double(), obs[b].double()).min() \
                    > clearance
    for a in range(B):
        for b in range(a + 1, B):
            assert not torch.equal(starts[a], starts[b])
            assert not torch.equal(goals[a], goals[b])
    # the batch is steppable from the device layout
    with batch.scenes():
        batch.step(torch.zeros(B * n, env.action_dim, device="cuda"))
    assert int(batch.t.sum()) == B
