"""Device-side episode resets: the reset_sample HIP kernel against its eager
oracle (bitwise), the envs' opt-in device reset path, the rollout engine
on top of it, and the --device-reset CLI flag.

Kernel cases build their candidate stream and avoid set on the CPU from a
seeded ``torch.Generator`` and compare ``pts``/``count``/``used`` with the
oracle bitwise — accepted points are copies of candidates, so no tolerance
applies.  Every oracle run asserts that its smallest relative gap
``|d2 - thr²| / thr²`` is >= 1e-5: fp32 rounding of a 3-term squared distance
is below 1e-6 relative, so an FMA-contraction difference between kernel and
oracle cannot flip a decision on these inputs.  The seeds below were picked
on the CPU to satisfy that.
"""
import functools
import math
import os
import subprocess
import sys

import pytest
import torch

from gcbf_amd import ops
from gcbf_amd.env import make_env
from gcbf_amd.env.utils import device_rejection_sample
from gcbf_amd.graph import GraphBatch
from gcbf_amd.ops import eager
from gcbf_amd.trainer.utils import read_settings, set_seed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_GAP = 1e-5


# ------------------------------------------------------------------ helpers
def _stream(seed, B, C, dim, side, A):
    """Candidate pool (B, C, dim) then avoid points (A, dim), both scaled to
    [0, side), from one seeded CPU generator."""
    g = torch.Generator().manual_seed(seed)
    cand = torch.rand(B, C, dim, generator=g) * side
    avoid = torch.rand(A, dim, generator=g) * side
    return cand, avoid


def _oracle(cand, min_sep, avoid, avoid_dist, n, pts=None, count=None):
    B, _, dim = cand.shape
    if pts is None:
        pts = torch.zeros(B, n, dim)
        count = torch.zeros(B, dtype=torch.int32)
    else:
        pts, count = pts.clone(), count.clone()
    av = avoid.unsqueeze(0).expand(B, -1, -1) if avoid.dim() == 2 else avoid
    used, gap = eager.reset_sample(
        cand, torch.tensor(min_sep, dtype=torch.float32), av, avoid_dist,
        pts, count)
    print(f"oracle: used={used.tolist()} count={count.tolist()} "
          f"min_gap={gap:.3e}")
    assert gap >= MIN_GAP, gap
    return pts, count, used


def _kernel(cand, min_sep, avoid, avoid_dist, n, pts=None, count=None):
    dev = torch.device("cuda")
    B, _, dim = cand.shape
    if pts is None:
        pts = torch.zeros(B, n, dim, device=dev)
        count = torch.zeros(B, dtype=torch.int32, device=dev)
    else:
        pts, count = pts.clone().to(dev), count.clone().to(dev)
    used = ops.reset_sample(
        cand.to(dev), torch.tensor(min_sep, dtype=torch.float32, device=dev),
        avoid.to(dev), avoid_dist, pts, count)
    return pts.cpu(), count.cpu(), used.cpu()


def _assert_same(got, want):
    for name, g, w in zip(("pts", "count", "used"), got, want):
        assert g.dtype == w.dtype, name
        assert torch.equal(g, w), (name, g, w)


# config -> (seed, n, side, A, dim, min_sep (per problem), C)
CASES = {
    "partial": (0, 3, 4.0, 0, 2, (0.2,), 40),
    "dubins16": (0, 16, 4.0, 8, 2, (0.2,), 256),
    "tight130": (0, 130, 3.0, 0, 2, (0.2,), 2048),
    "stress256": (0, 256, 16.0, 32, 2, (0.2,), 512),
    "drone8": (1, 8, 2.0, 8, 3, (0.2,), 64),
    "a0": (1, 16, 4.0, 0, 2, (0.2,), 128),
    "batched": (0, 16, 4.0, 8, 2, (0.2, 0.25), 256),
    # problem 0 finishes in chunk 0, problem 1 needs more than 5 chunks
    "batched_uneven": (2, 16, 4.0, 8, 2, (0.2, 0.9), 1024),
}
AVOID_DIST = 0.2


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs and oracle result of a named case, computed once."""
    seed, n, side, A, dim, seps, C = CASES[name]
    cand, avoid = _stream(seed, len(seps), C, dim, side, A)
    want = _oracle(cand, list(seps), avoid, AVOID_DIST, n)
    return cand, avoid, list(seps), n, want


# ------------------------------------------------------------ oracle (CPU)
def _hand_built():
    p = torch.tensor([[1.0, 1.0],      # p0 valid
                      [1.1, 1.0],      # p1 within sep of p0: rejected
                      [1.25, 1.0],     # p2 within sep of p1 only: accepted
                      [0.1, 0.1],      # p3 within sep of the origin
                      [3.05, 3.0],     # p4 within avoid_dist of the avoid pt
                      [2.0, 2.0]])     # p5 valid
    avoid = torch.tensor([[3.0, 3.0]])
    return p.unsqueeze(0), avoid


def test_oracle_hand_built_chunk():
    cand, avoid = _hand_built()
    pts, count, used = _oracle(cand, [0.2], avoid, 0.2, 3)
    assert torch.equal(pts[0], cand[0, [0, 2, 5]])
    assert count.tolist() == [3] and used.tolist() == [6]


def test_oracle_matches_host_loop_on_same_stream(monkeypatch):
    """Fed the same candidate stream, the oracle accepts exactly what
    rejection_sample_positions accepts (origin quirk included)."""
    from gcbf_amd.env import utils
    seed, n, side, A, dim, seps, C = CASES["dubins16"]
    cand, avoid, _, _, (pts, count, used) = _case("dubins16")

    class Replay:
        """torch.rand stand-in replaying the scaled pool one row at a time
        (the host loop multiplies by side itself)."""
        i = 0

        def __call__(self, d, generator=None):
            row = cand[0, self.i] / side
            self.i += 1
            return row

    replay = Replay()
    monkeypatch.setattr(torch, "rand", replay)
    host = utils.rejection_sample_positions(
        n, dim, side, seps[0], avoid=avoid, avoid_dist=AVOID_DIST)
    monkeypatch.undo()
    # side is a power of two here, so /side then *side is exact
    assert torch.equal(host, pts[0])
    assert replay.i == int(used[0]) and int(count[0]) == n


def test_oracle_table_figures():
    """Consumption figures of the configurations the kernel cases use."""
    assert _case("dubins16")[4][2].tolist() == [18]
    assert _case("dubins16")[4][1].tolist() == [16]
    assert 64 * 5 < int(_case("batched_uneven")[4][2][1])
    assert int(_case("batched_uneven")[4][2][0]) <= 64
    assert _case("batched_uneven")[4][1].tolist() == [16, 16]


def test_cpu_dispatch_is_oracle():
    cand, avoid, seps, n, want = _case("dubins16")
    pts = torch.zeros(1, n, 2)
    count = torch.zeros(1, dtype=torch.int32)
    used = ops.reset_sample(cand, torch.tensor(seps), avoid, AVOID_DIST, pts,
                            count)
    _assert_same((pts, count, used), want)


# ------------------------------------------------------------ kernel (GPU)
@pytest.mark.gpu
def test_kernel_hand_built_chunk():
    cand, avoid = _hand_built()
    want = _oracle(cand, [0.2], avoid, 0.2, 3)
    got = _kernel(cand, [0.2], avoid, 0.2, 3)
    _assert_same(got, want)
    assert torch.equal(got[0][0], cand[0, [0, 2, 5]])
    assert got[1].tolist() == [3] and got[2].tolist() == [6]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["partial", "dubins16", "tight130",
                                  "stress256", "drone8", "a0"])
def test_kernel_matches_oracle(name):
    """partial: one partial chunk (C=40); dubins16: stop mid-chunk, used is
    the oracle's value, not 64 or 256; tight130/stress256: many chunks with
    n no multiple of 64 / a multiple of 64; drone8: dim=3; a0: empty avoid
    tensor."""
    cand, avoid, seps, n, want = _case(name)
    got = _kernel(cand, seps, avoid, AVOID_DIST, n)
    _assert_same(got, want)
    assert int(got[1][0]) == n
    if name == "dubins16":
        assert int(got[2][0]) not in (64, 256)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["batched", "batched_uneven"])
def test_kernel_batched(name):
    """B=2, per-problem min_sep, shared avoid set: each problem equals its
    own single-problem oracle."""
    cand, avoid, seps, n, want = _case(name)
    got = _kernel(cand, seps, avoid, AVOID_DIST, n)
    _assert_same(got, want)
    for b in range(2):
        single = _oracle(cand[b:b + 1], seps[b:b + 1], avoid, AVOID_DIST, n)
        for g, s in zip(got, single):
            assert torch.equal(g[b:b + 1], s)


@pytest.mark.gpu
def test_kernel_exhaust_and_resume():
    """dense65, seed 0: a 4096 pool runs out (count < n, used == C); a second
    call with a fresh pool on the same pts/count equals the oracle run on
    the concatenated stream."""
    n, side, C = 65, 2.0, 4096
    cand1, avoid = _stream(0, 1, C, 2, side, 8)
    cand2, _ = _stream(1000, 1, C, 2, side, 0)
    want1 = _oracle(cand1, [0.2], avoid, AVOID_DIST, n)
    assert int(want1[1][0]) < n and int(want1[2][0]) == C
    got1 = _kernel(cand1, [0.2], avoid, AVOID_DIST, n)
    _assert_same(got1, want1)

    got2 = _kernel(cand2, [0.2], avoid, AVOID_DIST, n, got1[0], got1[1])
    cat = _oracle(torch.cat([cand1, cand2], dim=1), [0.2], avoid, AVOID_DIST,
                  n)
    assert torch.equal(got2[0], cat[0])
    assert torch.equal(got2[1], cat[1])
    assert int(got2[1][0]) > int(got1[1][0])
    assert int(got2[2][0]) == int(cat[2][0]) - C


@pytest.mark.gpu
def test_kernel_resume_completes_mid_pool():
    """Resume from a part-filled state that the second pool completes:
    count reaches n and used stops inside the pool."""
    cand, avoid, seps, n, want = _case("tight130")
    first, second = cand[:, :640], cand[:, 640:]
    got1 = _kernel(first, seps, avoid, AVOID_DIST, n)
    assert int(got1[1][0]) < n and int(got1[2][0]) == 640
    got2 = _kernel(second, seps, avoid, AVOID_DIST, n, got1[0], got1[1])
    assert torch.equal(got2[0], want[0]) and torch.equal(got2[1], want[1])
    assert int(got2[2][0]) == int(want[2][0]) - 640


@pytest.mark.gpu
def test_kernel_deterministic():
    cand, avoid, seps, n, _ = _case("batched_uneven")
    a = _kernel(cand, seps, avoid, AVOID_DIST, n)
    b = _kernel(cand, seps, avoid, AVOID_DIST, n)
    _assert_same(a, b)


@pytest.mark.gpu
def test_kernel_rejects_n_over_lds_budget():
    dev = torch.device("cuda")
    with pytest.raises(RuntimeError, match="4096"):
        ops.reset_sample(torch.rand(1, 64, 2, device=dev),
                         torch.tensor([0.2], device=dev), None, 0.0,
                         torch.zeros(1, 4097, 2, device=dev),
                         torch.zeros(1, dtype=torch.int32, device=dev))


# ------------------------------------------------------------------- envs
ENVS = ["SimpleCar", "DubinsCar", "SimpleDrone"]


def _make(name, device, device_reset):
    params = make_env(name, 8, device).default_params
    if name == "DubinsCar":
        params["num_obs"] = 4
    env = make_env(name, 8, device, params=params, device_reset=device_reset)
    env.train()
    return env


def _layout(env):
    """(starts, goals, obstacles or None, pos_dim, radius)."""
    n = env.num_agents
    d = 3 if env.state_dim == 6 else 2
    starts = env.data.states[:n, :d]
    goals = env._goal[:, :d]
    obs = getattr(env, "_obs", None)
    r = env.params.get("car_radius", env.params.get("drone_radius"))
    return starts, goals, None if obs is None else obs[:, :d], d, r


def _min_pairwise(p):
    dist = torch.cdist(p.double(), p.double())
    dist = dist + torch.eye(p.shape[0], dtype=dist.dtype,
                            device=p.device) * 1e6
    return float(dist.min())


@pytest.mark.parametrize("name", ENVS)
def test_device_reset_layout_valid(name, device):
    env = _make(name, device, True)
    assert env.device_reset
    set_seed(0)
    data = env.reset()
    starts, goals, obs, d, r = _layout(env)
    n, side = env.num_agents, env.params["area_size"]
    goal_sep = 5 * r if name == "DubinsCar" else 4 * r

    assert data.states.device.type == device.type
    assert _min_pairwise(starts) > 4 * r
    assert _min_pairwise(goals) > goal_sep
    # reference quirk kept: the origin counts as occupied
    assert float(starts.norm(dim=1).min()) > 4 * r
    assert float(goals.norm(dim=1).min()) > goal_sep
    for p in (starts, goals):
        assert bool((p >= 0).all()) and bool((p < side).all())
    if obs is not None:
        n_obs = 4 if name == "DubinsCar" else n
        assert obs.shape[0] == n_obs
        avoid_dist = 2 * r + 2 * env.params["obs_point_r"]
        for p in (starts, goals):
            assert float(torch.cdist(p.double(), obs.double()).min()) \
                > avoid_dist
        assert bool((obs >= 0).all()) and bool((obs < side).all())

    agents = data.states[:n]
    if name == "DubinsCar":
        assert bool((agents[:, 3] == 0).all())
        assert bool((agents[:, 2] >= -math.pi).all())
        assert bool((agents[:, 2] < math.pi).all())
    else:
        assert bool((agents[:, d:] == 0).all())


@pytest.mark.parametrize("name", ENVS)
def test_device_reset_graph_consistent(name, device):
    env = _make(name, device, True)
    set_seed(0)
    data = env.reset()
    d = 3 if env.state_dim == 6 else 2
    fresh = GraphBatch(x=data.x, pos=data.states[:, :d].clone(),
                       states=data.states.clone(),
                       agent_mask=data.agent_mask)
    if data.agent_mask is not None:
        fresh.agents_first_n = env.num_agents
    fresh = env.add_communication_links(fresh)
    assert torch.equal(data.pos, data.states[:, :d])
    assert torch.equal(data.edge_index, fresh.edge_index)
    assert torch.equal(data.edge_attr, fresh.edge_attr)


@pytest.mark.parametrize("name", ENVS)
def test_device_reset_seed_reproducible(name, device):
    env = _make(name, device, True)
    out = []
    for _ in range(2):
        set_seed(0)
        data = env.reset()
        out.append((data.states.clone(), env._goal.clone()))
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])
    data = env.reset()   # the stream moves on without a re-seed
    assert not torch.equal(out[0][0], data.states)


@pytest.mark.parametrize("name", ENVS)
def test_switch_off_is_host_path(name, device, monkeypatch):
    """With the switch off, reset() under seed 0 equals a fresh env's reset
    under seed 0 and never touches ops.reset_sample."""
    env = _make(name, device, True)
    set_seed(1)
    env.reset()
    env.set_device_reset(False)
    assert not env.device_reset

    def boom(*a, **k):
        raise AssertionError("ops.reset_sample called on the host path")

    monkeypatch.setattr(ops, "reset_sample", boom)
    set_seed(0)
    a = env.reset()
    a_goal = env._goal.clone()
    fresh = _make(name, device, False)
    set_seed(0)
    b = fresh.reset()
    assert torch.equal(a.states, b.states)
    assert torch.equal(a_goal, fresh._goal)
    assert torch.equal(a.edge_index, b.edge_index)

    # ... and the patch does bite when the switch is on
    env.set_device_reset(True)
    with pytest.raises(AssertionError, match="host path"):
        env.reset()


def test_demo_2_stays_on_host_path(device, monkeypatch):
    env = _make("SimpleCar", device, True)
    env.demo(2)

    def boom(*a, **k):
        raise AssertionError("ops.reset_sample called in demo_2")

    monkeypatch.setattr(ops, "reset_sample", boom)
    set_seed(0)
    a = env.reset().states.clone()
    ref = _make("SimpleCar", device, False)
    ref.demo(2)
    set_seed(0)
    assert torch.equal(a, ref.reset().states)


def test_env_var_sets_default(device, monkeypatch):
    monkeypatch.delenv("GCBF_AMD_DEVICE_RESET", raising=False)
    assert not make_env("SimpleCar", 4, device).device_reset
    monkeypatch.setenv("GCBF_AMD_DEVICE_RESET", "1")
    assert make_env("SimpleCar", 4, device).device_reset
    assert not make_env("SimpleCar", 4, device,
                        device_reset=False).device_reset


@pytest.mark.parametrize("name", ["SimpleCar", "DubinsCar"])
def test_plot_limits_lazy(name, device):
    """Device path: limits are owed after reset and computed on demand, to
    the same values the eager host-path computation gives."""
    env = _make(name, device, True)
    set_seed(0)
    env.reset()
    assert env._xy_min is None and env._plot_pts is not None
    pts = env._plot_pts.clone()
    low, high = env.state_lim
    assert env._plot_pts is None and env._xy_min is not None
    ref = _make(name, device, False)
    ref._set_plot_limits(pts)
    assert (env._xy_min == ref._xy_min).all()
    assert (env._xy_max == ref._xy_max).all()
    assert float(low[0]) == pytest.approx(float(ref._xy_min[0]))
    # host path stays eager
    set_seed(0)
    ref.reset()
    assert ref._xy_min is not None and ref._plot_pts is None


def test_render_after_device_reset(device):
    import matplotlib
    matplotlib.use("Agg")
    env = _make("DubinsCar", device, True)
    set_seed(0)
    env.reset()
    frame = env.render()
    assert frame.ndim == 3 and frame.shape[2] == 3
    assert env._xy_min is not None


def test_device_rejection_sample_shapes_and_resume(device):
    """A pool of C = 64*ceil((2n+64)/64) is not enough for a tight layout:
    the helper keeps drawing pools and resumes from the pts/count state."""
    calls = []
    real = ops.reset_sample

    def counting(*a, **k):
        calls.append(a[0].shape)
        return real(*a, **k)

    set_seed(0)
    ops.reset_sample = counting
    try:
        pts = device_rejection_sample(60, 2, 2.0, (0.2,), None, 0.0, device)
    finally:
        ops.reset_sample = real
    assert pts.shape == (1, 60, 2)
    assert len(calls) > 1 and all(s == (1, 192, 2) for s in calls)
    assert _min_pairwise(pts[0]) > 0.2


def test_device_rejection_sample_infeasible_raises(device):
    # every point of [0, 0.1)^2 is within 0.2 of the origin
    with pytest.raises(RuntimeError, match="64 candidate pools"):
        device_rejection_sample(4, 2, 0.1, (0.2,), None, 0.0, device)


# ----------------------------------------------------------------- engine
@pytest.mark.gpu
def test_rollout_engine_reload_with_device_reset():
    from gcbf_amd.algo import make_algo
    from gcbf_amd.rollout import RolloutEngine, engine_supported
    dev = torch.device("cuda")
    set_seed(0)
    env = _make("DubinsCar", dev, True)
    algo = make_algo("gcbf", env, 8, env.node_dim, env.edge_dim,
                     env.action_dim, dev, batch_size=32)
    env.reset()
    assert engine_supported(env, algo)
    eng = RolloutEngine(env, algo)
    before = eng.states[eng.cur].clone()
    eng.reload()
    assert not torch.equal(before, eng.states[eng.cur])
    assert torch.equal(eng.states[eng.cur], env.data.states)
    assert torch.equal(eng.goal, env._goal)
    assert eng.E == env.data.num_edges
    for _ in range(5):
        eng.step(0.5)
    assert torch.isfinite(eng.states[eng.cur]).all()


# -------------------------------------------------------------------- CLI
def test_cli_device_reset_flag(tmp_path):
    """--device-reset parses, lands in the saved settings, and the run
    trains on device-path resets; test.py accepts the flag too."""
    log_root = str(tmp_path)
    r = subprocess.run(
        [sys.executable, "train.py", "--env", "SimpleCar", "-n", "4",
         "--steps", "10", "--batch-size", "20", "--cpu", "--log-path",
         log_root, "--eval-epi", "0", "--seed", "0", "--device-reset"],
        cwd=REPO, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    base = os.path.join(log_root, "SimpleCar", "gcbf")
    (run,) = os.listdir(base)
    assert read_settings(os.path.join(base, run))["device_reset"] is True

    r = subprocess.run(
        [sys.executable, "test.py", "--help"], cwd=REPO,
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--device-reset" in r.stdout
