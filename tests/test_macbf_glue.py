"""macbf_glue.hip and the MACBF actor over padded edge buffers.

``ops.segmax_rows_bf16`` is compared with the composition it replaces
(``ops.segment_max`` on the edge list, row select, zero pad, bf16 cast) by
torch.equal: a max selects one of its inputs, so nothing may differ by one
bit.  The controller over a padded edge list (sentinel segment ids, static
row count) is compared with the same controller on the exact list and the
boolean agent mask, and on the GPU the whole actor with the glue chain on
and off, eagerly and through three policy steps of captured engines.
"""
import numpy as np
import pytest
import torch

from gcbf_amd import ops

ROWS = 256
NUM_NODES = 7
LENS = [1, 3, 0, 70, 0]
N_SENTINEL = 17
# rows of a LONG index: skips nodes, ends on nodes without edges
INDEX = [1, 3, 4, 6]
ROW_CASES = [5, INDEX]
ROW_IDS = ["first5", "index"]


def _pad_rows(t, rows):
    return torch.cat([t, t.new_zeros(rows - t.shape[0], t.shape[1])])


def _segmax_case(D):
    """The segment pattern of test_mlp_glue._attn_case: 7 nodes, segment
    lengths 1, 3, 0, 70, 0 (an empty one in the middle, one at the end, one
    longer than a wave) and 17 sentinel entries whose messages are NaN."""
    g = torch.Generator().manual_seed(D)
    seg = torch.cat([torch.full((n,), r, dtype=torch.long)
                     for r, n in enumerate(LENS)]
                    + [torch.full((N_SENTINEL,), NUM_NODES,
                                  dtype=torch.long)])
    msg = torch.randn(seg.numel(), D, generator=g)
    msg[3, 0] = -0.0                     # a signed zero among the candidates
    msg[-N_SENTINEL:] = float("nan")
    return msg.bfloat16(), seg


def _loop_reference(msg, seg, rows):
    """Row by row: max over the messages of the row's node, 0 if none."""
    nodes = list(range(rows)) if isinstance(rows, int) else rows
    out = torch.zeros(ROWS, msg.shape[1])
    for r, node in enumerate(nodes):
        sel = msg[:seg.shape[0]][seg == node].float()
        if sel.shape[0] > 0:
            out[r] = sel.max(dim=0).values
    return out.bfloat16()


def _composition(msg, seg, rows, drop_sentinels):
    """What the op replaces.  On the GPU the sentinel entries stay in the
    list (they fall outside every CSR segment), as in the actor."""
    E = seg.shape[0]
    m, s = msg[:E].float(), seg
    if drop_sentinels:
        real = seg < NUM_NODES
        m, s = m[real], s[real]
    aggr = ops.segment_max(m, s, NUM_NODES)
    if isinstance(rows, int):
        sel = aggr[:rows]
    else:
        sel = aggr[torch.tensor(rows, dtype=torch.long, device=msg.device)]
    return _pad_rows(sel, ROWS).bfloat16()


def _check_op(msg, seg, rows, drop_sentinels):
    dev = msg.device
    D = msg.shape[1]
    arg = rows if isinstance(rows, int) else torch.tensor(
        rows, dtype=torch.long, device=dev)
    out = ops.segmax_rows_bf16(msg, seg, arg, NUM_NODES, ROWS)
    assert out.dtype == torch.bfloat16 and out.shape == (ROWS, D)
    assert out.is_contiguous() and out.device == dev
    assert bool(torch.isfinite(out.float()).all())
    assert torch.equal(out, _composition(msg, seg, rows, drop_sentinels))
    assert torch.equal(out.cpu(), _loop_reference(msg.cpu(), seg.cpu(), rows))
    nodes = list(range(rows)) if isinstance(rows, int) else rows
    for r, node in enumerate(nodes):
        empty = node >= len(LENS) or LENS[node] == 0
        assert bool((out[r] == 0).all()) == empty, f"row {r}"
    assert bool((out[len(nodes):] == 0).all())          # pad rows


# ----------------------------------------------------------- CPU: op twin
@pytest.mark.parametrize("rows", ROW_CASES, ids=ROW_IDS)
@pytest.mark.parametrize("D", [128, 12])
def test_segmax_rows_bf16_eager_twin(D, rows):
    msg, seg = _segmax_case(D)
    # φ's padded output has more rows than the edge list
    msg = torch.cat([msg, torch.full((5, D), float("nan")).bfloat16()])
    _check_op(msg, seg, rows, drop_sentinels=True)


# -------------------------------------------------- CPU: padded controller
def _padded(data, N, cap):
    """The engine's padded layout of an exact edge list: pad entries
    src = dst = 0, zero attributes, sentinel segment id N."""
    E = data.num_edges
    assert 0 < E < cap
    ei = torch.zeros(2, cap, dtype=torch.long)
    ei[:, :E] = data.edge_index
    ea = torch.zeros(cap, data.edge_attr.shape[1])
    ea[:E] = data.edge_attr
    seg = torch.full((cap,), N, dtype=torch.long)
    seg[:E] = data.edge_index[1]
    return ei, ea, seg


# four agents at rest inside each other's comm radius, two obstacle rows
AGENT_XY = [(0.0, 0.0), (0.25, 0.0), (0.5, 0.0625), (0.0625, 0.3125)]
OBSTACLES = [[0.125, 0.1875, 0.4, 0.0], [0.3125, -0.25, 1.1, 0.05]]


def _cpu_scene(name, n_obs):
    """A capped CPU env holding a fixed clustered scene, so the exact edge
    list has at least n * k = 8 edges whatever the reset sampler would draw.  (The
    CPU BLAS computes a one- or two-row GEMM in another summation order
    than a wider one, so an exact list that short would differ from its
    padded twin in the last bit through no doing of the controller's.)"""
    from gcbf_amd.env import make_env
    dev = torch.device("cpu")
    n = len(AGENT_XY)
    params = make_env(name, n, dev).default_params
    params["num_obs"] = n_obs
    env = make_env(name, n, dev, params=params, max_neighbors=2)
    env.train()
    env.reset()
    f = torch.float32
    if name == "SimpleCar":
        states = torch.tensor([[x, y, 0.0, 0.0] for x, y in AGENT_XY],
                              dtype=f)
        env._goal = torch.tensor([[x + 0.75, y + 0.5] for x, y in AGENT_XY],
                                 dtype=f)
    else:
        states = torch.tensor([[x, y, 0.3 * k, 0.2]
                               for k, (x, y) in enumerate(AGENT_XY)], dtype=f)
        env._goal = torch.tensor([[x + 0.75, y + 0.5, 0.0, 0.0]
                                  for x, y in AGENT_XY], dtype=f)
        env._obs = torch.tensor(OBSTACLES[:n_obs], dtype=f)
    env._data = env.add_communication_links(env._build_data(states))
    return env, env._data


@pytest.mark.parametrize("case", [("SimpleCar", 4, 0), ("DubinsCar", 4, 2)],
                         ids=["car4", "dubins4obs2"])
def test_controller_over_padded_edges_cpu(case):
    from gcbf_amd.controller import MACBFController
    from gcbf_amd.graph import GraphBatch
    from gcbf_amd.trainer.utils import set_seed
    name, n, n_obs = case
    set_seed(5)
    env, data = _cpu_scene(name, n_obs)
    data.update(u_ref=env.u_ref(data))
    N = data.num_nodes
    assert N == n + n_obs and (data.agent_mask is not None) == (n_obs > 0)
    # the cap is live (ties at the k-th distance are kept)
    assert 2 * n <= data.num_edges < n * (N - 1)
    actor = MACBFController(num_agents=n, node_dim=env.node_dim,
                            edge_dim=env.edge_dim, phi_dim=128,
                            action_dim=env.action_dim)
    with torch.no_grad():
        for p in actor.parameters():
            p.add_(torch.randn_like(p) * 0.05)
        want = actor(data)
        ei, ea, seg = _padded(data, N, n * (N - 1) + 3)
        pad = GraphBatch(x=data.x, pos=data.pos, states=data.states,
                         edge_index=ei, edge_attr=ea,
                         agent_mask=data.agent_mask, u_ref=data.u_ref)
        pad.seg_dst = seg
        pad.agents_first_n = n if data.agent_mask is not None else None
        got = actor(pad)
    assert want.shape == (n, env.action_dim)
    assert bool(want.abs().sum() > 0)
    assert torch.equal(got, want)


# ------------------------------------------------- CPU: exploration floor
def test_explore_prob_floor():
    from gcbf_amd.algo import make_algo
    from gcbf_amd.env import make_env
    dev = torch.device("cpu")
    env = make_env("SimpleCar", 3, dev, max_neighbors=2)
    macbf = make_algo("macbf", env, 3, env.node_dim, env.edge_dim,
                      env.action_dim, dev, batch_size=8)
    gcbf = make_algo("gcbf", env, 3, env.node_dim, env.edge_dim,
                     env.action_dim, dev, batch_size=8)
    assert macbf.explore_prob(0.2) == 0.5
    assert macbf.explore_prob(0.8) == 0.8
    assert gcbf.explore_prob(0.2) == 0.2


# ------------------------------------------------------------------ GPU: op
@pytest.mark.gpu
@pytest.mark.parametrize("rows", ROW_CASES, ids=ROW_IDS)
@pytest.mark.parametrize("D", [128, 12])
def test_segmax_rows_bf16_kernel(D, rows):
    msg, seg = _segmax_case(D)
    msg = torch.cat([msg, torch.full((5, D), float("nan")).bfloat16()])
    _check_op(msg.cuda(), seg.cuda(), rows, drop_sentinels=False)
    # and the CPU twin computes the same rows
    arg = rows if isinstance(rows, int) else torch.tensor(rows)
    arg_dev = arg if isinstance(arg, int) else arg.cuda()
    assert torch.equal(
        ops.segmax_rows_bf16(msg.cuda(), seg.cuda(), arg_dev, NUM_NODES,
                             ROWS).cpu(),
        ops.segmax_rows_bf16(msg, seg, arg, NUM_NODES, ROWS))


@pytest.mark.gpu
def test_segmax_rows_bf16_is_forward_only():
    msg, seg = _segmax_case(12)
    msg = msg.cuda().requires_grad_(True)
    with pytest.raises(RuntimeError, match="forward only"):
        ops.segmax_rows_bf16(msg, seg.cuda(), 5, NUM_NODES, ROWS)
    with torch.no_grad():
        out = ops.segmax_rows_bf16(msg, seg.cuda(), 5, NUM_NODES, ROWS)
    assert not out.requires_grad


# ---------------------------------------------------------- GPU: whole actor
ACTOR_CASES = [("SimpleCar", 5, 0), ("DubinsCar", 5, 2)]
ACTOR_IDS = ["car5", "dubins5obs2"]
CAP = 2


# five agents inside each other's comm radius (the reset sampler spreads five
# agents so far apart that the graph can be empty), two obstacle rows
ACTOR_XY = [(1.0, 1.0), (1.25, 1.0), (1.5, 1.0625), (1.0625, 1.3125),
            (1.375, 1.4375)]
ACTOR_OBS = [[1.125, 1.1875, 0.4, 0.0], [1.3125, 0.75, 1.1, 0.05]]


def _cluster(env, name):
    """Replace the reset scene's states by the fixed cluster (goals stay)."""
    dev = env.device
    if name == "SimpleCar":
        rows = [[x, y, 0.1, -0.05] for x, y in ACTOR_XY]
    else:
        rows = [[x, y, 0.3 * k, 0.2] for k, (x, y) in enumerate(ACTOR_XY)]
        env._obs = torch.tensor(ACTOR_OBS, device=dev)
    env._data = env.add_communication_links(
        env._build_data(torch.tensor(rows, device=dev)))


def _make_engine(case, glue, monkeypatch):
    """Fresh capped env, MACBF (random weights and biases, bf16) and
    captured engine; the same seeds give the same scene and weights every
    call."""
    from gcbf_amd.algo import make_algo
    from gcbf_amd.env import make_env
    from gcbf_amd.rollout import RolloutEngine, engine_supported
    from gcbf_amd.trainer.utils import set_seed
    from gcbf_amd.utils.amp import enable_bf16
    name, n, n_obs = case
    dev = torch.device("cuda")
    set_seed(3)
    params = make_env(name, n, dev).default_params
    params["num_obs"] = n_obs
    env = make_env(name, n, dev, params=params, max_neighbors=CAP)
    env.train()
    algo = make_algo("macbf", env, n, env.node_dim, env.edge_dim,
                     env.action_dim, dev, batch_size=32)
    with torch.no_grad():
        for p in algo.actor.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    enable_bf16(algo)
    env.reset()
    _cluster(env, name)
    assert not engine_supported(env, algo)
    assert engine_supported(env, algo, capped=True)
    monkeypatch.setenv("GCBF_AMD_ACTOR_GLUE", "1" if glue else "0")
    eng = RolloutEngine(env, algo)
    assert eng._glue == glue and eng.topk == CAP
    return eng


def _engine_data(eng, glue):
    from gcbf_amd.graph import GraphBatch
    c = eng.cur
    data = GraphBatch(x=eng.x, pos=eng.states[c][:, :eng.pos_dim],
                      states=eng.states[c], edge_index=eng.ei[c],
                      edge_attr=eng.ea[c], agent_mask=eng.agent_mask,
                      u_ref=eng.u_ref[c])
    data.seg_dst = eng.seg[c]
    data.agents_first_n = eng.n if eng.agent_mask is not None else None
    data.actor_glue = glue
    return data


@pytest.mark.gpu
@pytest.mark.parametrize("case", ACTOR_CASES, ids=ACTOR_IDS)
def test_macbf_actor_glue_equals_eager_composition(case, monkeypatch):
    """Eagerly on identical buffers, then three policy steps of a captured
    engine of each kind from the same start."""
    eng = _make_engine(case, True, monkeypatch)
    actor = eng.algo.actor
    if case[2] > 0:                          # agents_first_n path
        assert eng.agent_mask is not None and eng.N == case[1] + case[2]
    # the cap is live and pad entries follow the real edges
    assert CAP * case[1] <= eng.E < eng.E_max
    with torch.no_grad():
        on, off = _engine_data(eng, True), _engine_data(eng, False)
        assert actor._glue_applies(on, on.agents_first_n)
        assert not actor._glue_applies(off, off.agents_first_n)
        a_ref = actor(off)
        a_new = actor(on)
    assert a_new.dtype == a_ref.dtype and a_new.shape == a_ref.shape
    assert bool(a_ref.abs().sum() > 0)
    assert torch.equal(a_new, a_ref)
    # grad mode keeps the differentiable path
    assert not actor._glue_applies(on, on.agents_first_n)

    ref_eng = _make_engine(case, False, monkeypatch)
    for k in ("states", "u_ref", "ei", "seg", "ea"):
        assert torch.equal(getattr(eng, k)[eng.cur],
                           getattr(ref_eng, k)[ref_eng.cur]), f"start: {k}"
    # MACBF floors the exploration probability at 0.5, so prob = 0 does not
    # pin the branch: a draw of 0.9 does (0.9 < 0.5 never: policy graph)
    monkeypatch.setattr(np.random, "rand", lambda *a: 0.9)
    for t in range(3):
        done_new = eng.step(prob=0.0)
        done_ref = ref_eng.step(prob=0.0)
        assert done_new == done_ref and not done_new
        assert eng.E == ref_eng.E
        for k in ("states", "u_ref", "ei", "seg", "ea"):
            assert torch.equal(getattr(eng, k)[eng.cur],
                               getattr(ref_eng, k)[ref_eng.cur]), \
                f"step {t}: {k}"
    assert bool((eng.states[eng.cur] != eng.states[1 - eng.cur]).any())
