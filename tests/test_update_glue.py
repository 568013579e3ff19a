"""Update glue: the grad-mode padded-bf16 chain of the GNN layers
(ops/hip/mlp_glue.hip backwards, nn/fused.run_plan_padded_bf16_train).

As in test_mlp_glue.py the reference of every test is the composition of
existing ops that the glue replaces, on the same GPU tensors, and the
comparison is torch.equal on outputs and on every gradient: the glue only
moves, pads and rounds values, and the attention arithmetic is the device
functions seg_attn_fwd / seg_attn_bwd run.
"""
import copy

import numpy as np
import pytest
import torch

from gcbf_amd import ops

ROWS = 256

# values around 1 whose bf16 rounding (ulp 2^-7) goes each way (see
# test_mlp_glue.py)
_ROUNDING = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20,
             1 + 2.0 ** -9, -(1 + 3 * 2.0 ** -8), -(1 + 2.0 ** -9)]

CASES = [("DubinsCar", 3, 0), ("DubinsCar", 5, 2), ("SimpleDrone", 4, 0)]
IDS = ["dubins3", "dubins5obs2", "drone4"]


def _pad_rows(t, rows):
    return torch.cat([t, t.new_zeros(rows - t.shape[0], t.shape[1])])


def _make_env(case, dev):
    from gcbf_amd.env import make_env
    name, n, n_obs = case
    params = make_env(name, n, dev).default_params
    params["num_obs"] = n_obs
    env = make_env(name, n, dev, params=params)
    env.train()
    return env


# ------------------------------------------------------------ dst-sorted
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_builder_edges_are_dst_sorted(case):
    """The glue finds a node's edges by binary search over dst.  These
    envs with 16 agents, so that every scene has edges."""
    from gcbf_amd.graph import GraphBatch
    from gcbf_amd.trainer.utils import set_seed
    set_seed(1)
    case = (case[0], 16, case[2])
    env = _make_env(case, torch.device("cpu"))
    singles = []
    data = env.reset()
    for _ in range(3):
        singles.append(data)
        dst = data.edge_index[1]
        assert bool((dst[1:] >= dst[:-1]).all())
        data, *_ = env.step(torch.zeros(case[1], env.action_dim))
    dst = GraphBatch.from_list(singles).edge_index[1]
    assert dst.numel() > 0 and bool((dst[1:] >= dst[:-1]).all())

    # the batches of an eager update iteration: ring batch, its forward
    # graph, the doubled batch and the re-linked graph
    from gcbf_amd.ring import RingStore
    ring = RingStore(env, 8)
    for g in singles:
        g.update(u_ref=env.u_ref(g))
        ring.push(g)
    graphs = ring.batch(singles)
    nxt = env.forward_graph(graphs, torch.full(
        (3 * case[1], env.action_dim), 0.3))
    both = GraphBatch.from_list([graphs, nxt])
    relinked = env.add_communication_links_batched(nxt.detach())
    for g in (graphs, nxt, both, relinked):
        dst = g.edge_index[1]
        assert dst.numel() > 0 and bool((dst[1:] >= dst[:-1]).all())


# ------------------------------------------------------------ edge inputs
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["DubinsCar", "SimpleDrone"])
def test_edge_inputs_grad(name):
    env = _make_env((name, 3, 0), torch.device("cpu"))
    nd, ed = env.node_dim, env.edge_dim
    g = torch.Generator().manual_seed(7)
    N, E = 9, 101
    x = torch.randn(N, nd, generator=g).cuda()
    x.view(-1)[:6] = torch.tensor(_ROUNDING, device="cuda")
    ei = torch.randint(0, N, (2, E), generator=g).cuda()
    ea = torch.randn(E, ed, generator=g).cuda()
    ea.view(-1)[:6] = torch.tensor(_ROUNDING, device="cuda")
    d_in = torch.randn(ROWS, 2 * nd + ed, generator=g).bfloat16().cuda()

    ea_ref = ea.clone().requires_grad_(True)
    ref = _pad_rows(torch.cat([x.index_select(0, ei[1]),
                               x.index_select(0, ei[0]), ea_ref], dim=1),
                    ROWS).bfloat16()
    ref.backward(d_in)
    ea_new = ea.clone().requires_grad_(True)
    out = ops.edge_inputs_bf16_grad(x, ei, ea_new, ROWS)
    out.backward(d_in)
    assert torch.equal(out, ref)
    assert ea_new.grad.dtype == torch.float32
    assert torch.equal(ea_new.grad, ea_ref.grad)
    assert bool((ea_new.grad != 0).any())


# ------------------------------------------------- gate + attention -> γ in
def _attn_case(D, nd, with_idx):
    """9 nodes.  Segment lengths 1, 3, 0, 70, 0, 9 over nodes 0..5 (an empty
    segment in the middle, a 70-edge one for a second trip of the
    block-stride loops), nodes 6..8 without edges (an empty end), then 17
    sentinel slots with NaN messages: 103 slots.  The index skips nodes 1
    and 2 (whose edges then belong to no row) and ends on an empty node."""
    g = torch.Generator().manual_seed(D + nd)
    num_nodes = 9
    lens = [1, 3, 0, 70, 0, 9]
    seg = torch.cat([torch.full((n,), r, dtype=torch.long)
                     for r, n in enumerate(lens)]
                    + [torch.full((17,), num_nodes, dtype=torch.long)])
    E = seg.numel()
    msg = _pad_rows(torch.randn(E, D, generator=g), ROWS)
    msg[E - 17:E] = float("nan")
    msg[E:] = 0.25                  # a GEMM's pad rows are not zero
    x = torch.randn(num_nodes, nd, generator=g)
    x.view(-1)[:6] = torch.tensor(_ROUNDING)
    idx = torch.tensor([0, 3, 4, 5, 7]) if with_idx else None
    n_rows = 5 if with_idx else 6
    d_out = torch.randn(ROWS, D + nd, generator=g).bfloat16()
    return (msg.bfloat16().cuda(), seg.cuda(), x.cuda(),
            None if idx is None else idx.cuda(), n_rows, num_nodes, E,
            d_out.cuda())


def _gate_mlp(D):
    from gcbf_amd.nn import MLP
    torch.manual_seed(D)
    mlp = MLP(in_channels=D, out_channels=1, hidden_layers=(128, 128)).cuda()
    with torch.no_grad():
        for p in mlp.parameters():
            p.add_(torch.randn_like(p) * 0.3)
    mlp.fused_mfma = True            # run_plan, as under enable_bf16
    return mlp


@pytest.mark.gpu
@pytest.mark.parametrize("msg_bf16", [False, True], ids=["msg32", "msg16"])
@pytest.mark.parametrize("with_idx", [False, True], ids=["rows", "idx"])
@pytest.mark.parametrize("D,name", [(4, "DubinsCar"), (256, "DubinsCar"),
                                    (256, "SimpleDrone")])
def test_gate_attn_gamma_in_grad(D, name, with_idx, msg_bf16):
    """msg32: φ ended in a plain layer, its fp32 output met both gradients
    in fp32 (actor).  msg16: φ ended in a spectral-normed layer, its bf16
    output met them in bf16 (CBF)."""
    from gcbf_amd.nn import fused
    nd = _make_env((name, 3, 0), torch.device("cpu")).node_dim
    msg, seg, x, idx, n_rows, num_nodes, E, d_out = _attn_case(D, nd,
                                                               with_idx)
    mlp = _gate_mlp(D)

    # the composition: exit of φ, gate MLP with its pad / cast / slice,
    # CSR pointer + seg_attn_fwd, cat, row selection, entry of γ
    m_ref = msg.clone().requires_grad_(True)
    m_out = m_ref[:E] if msg_bf16 else m_ref.float()[:E]
    gate = mlp(m_out)
    assert gate.dtype == torch.float32 and gate.shape == (E, 1)
    aggr = ops.segment_attn_aggregate(m_out, gate, seg, num_nodes)
    gamma_in = torch.cat([aggr.float(), x], dim=1)
    gamma_in = gamma_in[:n_rows] if idx is None else gamma_in[idx]
    ref = _pad_rows(gamma_in, ROWS).bfloat16()
    ref.backward(d_out)
    p_ref = [p.grad.clone() for p in mlp.parameters()]
    mlp.zero_grad(set_to_none=True)

    m_new = msg.clone().requires_grad_(True)
    out = ops.gate_attn_gamma_in(
        m_new, lambda m: fused.run_plan_padded_bf16_train(mlp._plan, m),
        fused.plan_params(mlp._plan), x, seg, idx, n_rows, num_nodes, ROWS,
        round_prod=msg_bf16)
    out.backward(d_out)

    assert out.dtype == torch.bfloat16 and out.shape == (ROWS, D + nd)
    assert torch.equal(out, ref)
    assert bool((out[n_rows:] == 0).all())
    assert bool(torch.isfinite(out.float()).all())
    got, want = m_new.grad, m_ref.grad
    assert got.dtype == torch.bfloat16 and got.shape == (ROWS, D)
    real = E - 17
    assert bool(torch.isfinite(want[:real].float()).all())
    assert torch.equal(got[:real], want[:real])
    assert bool((got[:real] != 0).any())
    # sentinel and pad slots: exactly zero
    assert bool((got[real:] == 0).all()) and bool((want[real:] == 0).all())
    # the gate MLP's wgrads see 0 * NaN on the sentinel rows in both paths;
    # compare them bit for bit, NaN included
    for a, b in zip(mlp.parameters(), p_ref):
        assert torch.equal(a.grad.view(torch.int32), b.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("with_idx", [False, True], ids=["rows", "idx"])
@pytest.mark.parametrize("D", [4, 256])
def test_backward_kernels_write_every_slot(D, with_idx):
    """The backward kernels into NaN-prefilled buffers: every slot is
    written, the ones outside the selected nodes' segments with exactly 0
    (dgate) or the gate MLP's gradient / 0 on sentinel and pad slots
    (dmsg)."""
    from gcbf_amd import _C
    msg, seg, x, idx, n_rows, num_nodes, E, d_out = _attn_case(D, 4,
                                                               with_idx)
    g = torch.Generator().manual_seed(D)
    gate = torch.randn(ROWS, generator=g).bfloat16().cuda()
    dmsg_gate = torch.randn(ROWS, D, generator=g).bfloat16().cuda()
    _, att = _C.attn_gamma_in_fwd(msg, gate, seg, x, idx, n_rows, num_nodes,
                                  ROWS)
    nodes = torch.arange(n_rows, device="cuda") if idx is None else idx
    covered = torch.zeros(ROWS, dtype=torch.bool, device="cuda")
    covered[:E] = torch.isin(seg, nodes)
    real = torch.zeros(ROWS, dtype=torch.bool, device="cuda")
    real[:E] = seg < num_nodes
    assert bool(covered.any()) and bool((real & ~covered).any()) == with_idx

    nan = float("nan")
    dgate = torch.full((ROWS, 1), nan, dtype=torch.bfloat16, device="cuda")
    res = _C.attn_gamma_in_bwd_gate(d_out, msg, att, seg, idx, n_rows,
                                    num_nodes, out=dgate)
    assert res.data_ptr() == dgate.data_ptr()
    assert bool(torch.isfinite(dgate.float()).all())
    assert bool((dgate[~covered] == 0).all())
    assert bool((dgate[covered] != 0).any())
    assert torch.equal(dgate, _C.attn_gamma_in_bwd_gate(
        d_out, msg, att, seg, idx, n_rows, num_nodes))

    for round_prod in (False, True):
        dmsg = torch.full((ROWS, D), nan, dtype=torch.bfloat16,
                          device="cuda")
        _C.attn_gamma_in_bwd_msg(d_out, att, seg, idx, dmsg_gate, n_rows,
                                 num_nodes, round_prod, out=dmsg)
        assert bool(torch.isfinite(dmsg.float()).all())
        assert bool((dmsg[~real] == 0).all())
        assert torch.equal(dmsg[real & ~covered],
                           dmsg_gate[real & ~covered])
        assert bool((dmsg[covered] != dmsg_gate[covered]).any())

    da = torch.full((ROWS, 8), nan, dtype=torch.bfloat16, device="cuda")
    d_in = torch.randn(ROWS, 11, generator=g).bfloat16().cuda()
    _C.rows_cat_bwd(d_in, 8, 5, out=da)
    assert torch.equal(da[:5], d_in[:5, :8]) and bool((da[5:] == 0).all())


# ------------------------------------------------------- cat + pad + cast
@pytest.mark.gpu
@pytest.mark.parametrize("widths", [(1024, 2), (8, 3)])
def test_rows_cat_pad_grad(widths):
    Da, Db = widths
    g = torch.Generator().manual_seed(Da)
    n_rows = 5
    a = torch.randn(ROWS, Da, generator=g).bfloat16().cuda()
    b = torch.randn(n_rows, Db, generator=g).cuda()
    d_in = torch.randn(ROWS, Da + Db, generator=g).bfloat16().cuda()
    a_ref = a.clone().requires_grad_(True)
    ref = _pad_rows(torch.cat([a_ref.float()[:n_rows], b], dim=1),
                    ROWS).bfloat16()
    ref.backward(d_in)
    a_new = a.clone().requires_grad_(True)
    out = ops.rows_cat_pad_bf16_grad(a_new, b, n_rows, ROWS)
    out.backward(d_in)
    assert torch.equal(out, ref)
    assert torch.equal(a_new.grad, a_ref.grad)
    assert bool((a_new.grad[:n_rows] != 0).any())
    assert bool((a_new.grad[n_rows:] == 0).all())


# ---------------------------------------------------------- whole networks
def _make_algo(case, batch_size=32):
    from gcbf_amd.algo import make_algo
    from gcbf_amd.trainer.utils import set_seed
    from gcbf_amd.utils.amp import enable_bf16
    dev = torch.device("cuda")
    set_seed(3)
    env = _make_env(case, dev)
    algo = make_algo("gcbf", env, case[1], env.node_dim, env.edge_dim,
                     env.action_dim, dev, batch_size=batch_size)
    with torch.no_grad():
        for net in (algo.actor, algo.cbf):
            for p in net.parameters():
                p.add_(torch.randn_like(p) * 0.05)
    enable_bf16(algo)
    return env, algo


def _count_glue(monkeypatch):
    calls = []
    real = ops.gate_attn_gamma_in

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(ops, "gate_attn_gamma_in", counted)
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_networks_equal_with_and_without_glue(case, monkeypatch):
    """Actor and CBF forward + backward over 4 ring graphs, switch 0 / 1,
    identical weights: outputs, edge_attr's gradient and every parameter's
    gradient are equal."""
    from gcbf_amd.ring import RingStore
    env, algo = _make_algo(case)
    data = env.reset()
    ring = RingStore(env, 16)
    singles = []
    for _ in range(4):
        data.update(u_ref=env.u_ref(data))
        ring.push(data)
        singles.append(data)
        data, *_ = env.step(torch.full((case[1], env.action_dim), 0.3,
                                       device="cuda"))
    algo._ring = ring
    states = [copy.deepcopy(net.state_dict())
              for net in (algo.actor, algo.cbf)]
    calls = _count_glue(monkeypatch)

    def run(glue):
        for net, st in zip((algo.actor, algo.cbf), states):
            net.load_state_dict(st)         # the power-iteration vectors too
            net.zero_grad(set_to_none=True)
        algo._update_glue = glue
        graphs = ring.batch(singles)
        graphs.edge_attr.requires_grad_(True)
        algo._stamp_glue(graphs)
        assert bool(graphs.update_glue) == glue
        actions = algo.actor(graphs)
        h = algo.cbf(graphs)
        w = torch.linspace(-1, 1, h.shape[0], device="cuda").unsqueeze(1)
        ((actions * actions).sum() + (h * w).sum()).backward()
        with torch.no_grad():               # the re-linked forward
            h_ng = algo.cbf(algo._stamp_glue(graphs.detach()))
        grads = {f"{k}.{n}": p.grad.clone()
                 for k, net in (("actor", algo.actor), ("cbf", algo.cbf))
                 for n, p in net.named_parameters()}
        grads["edge_attr"] = graphs.edge_attr.grad.clone()
        return actions.detach(), h.detach(), h_ng, grads

    ref = run(False)
    assert not calls
    new = run(True)
    assert len(calls) == 3, "glue path not taken"
    if case[2] > 0:
        assert ring._am1 is not None
    for a, b in zip(new[:3], ref[:3]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert bool(ref[0].abs().sum() > 0) and bool(ref[1].abs().sum() > 0)
    assert new[3].keys() == ref[3].keys()
    for k in ref[3]:
        assert bool(torch.isfinite(ref[3][k]).all()), k
        assert torch.equal(new[3][k], ref[3][k]), k
    assert bool((ref[3]["edge_attr"] != 0).any())


# -------------------------------------------------------- one whole update
@pytest.mark.gpu
def test_update_equal_with_and_without_glue(monkeypatch):
    """One algo.update at batch_size=20 from identical seeds: metrics,
    every parameter and every bf16 mirror are equal."""
    def run(glue):
        monkeypatch.setenv("GCBF_AMD_UPDATE_GLUE", "1" if glue else "0")
        env, algo = _make_algo(("DubinsCar", 5, 0), batch_size=20)
        assert algo._update_glue == glue
        np.random.seed(11)
        torch.manual_seed(11)
        data = env.reset()
        for _ in range(20):
            data.update(u_ref=env.u_ref(data))
            action = algo.step(data, prob=0.5)
            data, _, done, _ = env.step(action)
            if done:
                data = env.reset()
        info = algo.update(20, None)
        tensors = {}
        for k, net in (("actor", algo.actor), ("cbf", algo.cbf)):
            for n, p in net.named_parameters():
                tensors[f"{k}.{n}"] = p.detach().clone()
            for n, m in net.named_modules():
                for i, t in enumerate(getattr(m, "_bf16_mirror", None)
                                      or ()):
                    if torch.is_tensor(t):
                        tensors[f"{k}.{n}.mirror{i}"] = t.clone()
        return info, tensors, algo.params["inner_iter"]

    calls = _count_glue(monkeypatch)
    info_ref, ref, _ = run(False)
    assert not calls
    info_new, new, inner = run(True)
    assert len(calls) == 3 * inner, "glue path not taken"
    assert info_new == info_ref
    assert new.keys() == ref.keys()
    assert any("mirror" in k for k in ref)
    for k in ref:
        assert torch.equal(new[k], ref[k]), k
