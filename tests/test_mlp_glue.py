"""mlp_glue.hip: the kernels between the actor's library GEMMs, and the
one-launch bf16 mirror refresh.

The reference in every test is the composition of existing ops that the
glue replaces, on the same GPU tensors, and the comparison is torch.equal:
the glue only moves, pads and rounds values (round-to-nearest-even, as
``.bfloat16()``), and the attention sum runs the device function
``seg_attn_fwd`` runs, so nothing may differ by one bit.
"""
import copy

import pytest
import torch

from gcbf_amd import ops

ROWS = 256


def _pad_rows(t, rows):
    return torch.cat([t, t.new_zeros(rows - t.shape[0], t.shape[1])])


# values around 1 whose bf16 rounding (ulp 2^-7) goes each way: two ties
# (to even: down, up), one just above a tie (up), one below half (down)
_ROUNDING = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20,
             1 + 2.0 ** -9, -(1 + 3 * 2.0 ** -8), -(1 + 2.0 ** -9)]


def _with_rounding_cases(t):
    flat = t.view(-1)
    k = min(len(_ROUNDING), flat.numel())
    flat[:k] = torch.tensor(_ROUNDING[:k], device=t.device)
    return t


def _env_dims(name):
    from gcbf_amd.env import make_env
    env = make_env(name, 3, torch.device("cpu"))
    return env.node_dim, env.edge_dim


# ------------------------------------------------------------- edge inputs
@pytest.mark.gpu
@pytest.mark.parametrize("dims", ["DubinsCar", "SimpleDrone", (3, 5)],
                         ids=["dubins", "drone", "3x5"])
def test_edge_inputs_bf16(dims):
    nd, ed = _env_dims(dims) if isinstance(dims, str) else dims
    g = torch.Generator().manual_seed(5)
    N = 5
    x = _with_rounding_cases(torch.randn(N, nd, generator=g).cuda())
    # 7 slots: 4 real edges, 3 pads (src = dst = 0, zero attributes)
    ei = torch.tensor([[1, 4, 0, 2, 0, 0, 0],
                       [0, 0, 3, 4, 0, 0, 0]], device="cuda")
    ea = torch.randn(7, ed, generator=g).cuda()
    _with_rounding_cases(ea[1])
    ea[4:] = 0
    ref = _pad_rows(torch.cat([x.index_select(0, ei[1]),
                               x.index_select(0, ei[0]), ea], dim=1),
                    ROWS).bfloat16()
    rounded = ref[:4].float()
    exact = torch.cat([x[ei[1, :4]], x[ei[0, :4]], ea[:4]], dim=1)
    assert bool((rounded > exact).any()) and bool((rounded < exact).any())
    out = ops.edge_inputs_bf16(x, ei, ea, ROWS)
    assert out.dtype == torch.bfloat16 and out.is_contiguous()
    assert out.shape == (ROWS, 2 * nd + ed)
    assert out.stride() == (2 * nd + ed, 1)
    assert torch.equal(out, ref)
    assert bool((out[7:] == 0).all())


# ------------------------------------------------ aggregation -> γ input
def _attn_case(D, gate_dtype):
    """7 nodes, 5 receivers; segment lengths 1, 3, 0, 70, 0 (an empty one
    in the middle, one at the end, one longer than a wave) and 17 sentinel
    entries whose messages are NaN."""
    g = torch.Generator().manual_seed(D)
    num_nodes, n_rows, nd = 7, 5, 4
    lens = [1, 3, 0, 70, 0]
    seg = torch.cat([torch.full((n,), r, dtype=torch.long)
                     for r, n in enumerate(lens)]
                    + [torch.full((17,), num_nodes, dtype=torch.long)])
    E = seg.numel()
    msg = torch.randn(E, D, generator=g)
    msg[-17:] = float("nan")
    gate = (torch.randn(E, 1, generator=g) * 30 + 60).to(gate_dtype)
    x = torch.randn(num_nodes, nd, generator=g)
    return (msg.bfloat16().cuda(), gate.cuda(), seg.cuda(), x.cuda(),
            n_rows, num_nodes)


@pytest.mark.gpu
@pytest.mark.parametrize("gate_dtype", [torch.float32, torch.bfloat16],
                         ids=["gate32", "gate16"])
@pytest.mark.parametrize("D", [256, 12])
def test_attn_aggregate_gamma_in(D, gate_dtype):
    msg, gate, seg, x, n_rows, num_nodes = _attn_case(D, gate_dtype)
    aggr = ops.segment_attn_aggregate(msg, gate, seg, num_nodes)
    assert aggr.dtype == torch.float32
    ref = _pad_rows(torch.cat([aggr, x], dim=1)[:n_rows], ROWS).bfloat16()
    out = ops.attn_aggregate_gamma_in(msg, gate, seg, x, n_rows, num_nodes,
                                      ROWS)
    assert out.dtype == torch.bfloat16 and out.shape == (ROWS, D + 4)
    assert bool(torch.isfinite(out.float()).all())
    assert torch.equal(out, ref)
    assert bool((out[[2, 4], :D] == 0).all())       # empty segments
    assert bool((out[3, :D] != 0).any())
    assert bool((out[n_rows:] == 0).all())


# ------------------------------------------------------- cat + pad + cast
@pytest.mark.gpu
@pytest.mark.parametrize("widths", [(1024, 2), (8, 3)])
def test_rows_cat_pad_bf16(widths):
    Da, Db = widths
    g = torch.Generator().manual_seed(Da)
    n_rows = 5
    # a carries non-zero rows past n_rows, as a GEMM's padded output does
    a = torch.randn(ROWS, Da, generator=g).bfloat16().cuda()
    b = _with_rounding_cases(torch.randn(n_rows, Db, generator=g).cuda())
    ref = _pad_rows(torch.cat([a[:n_rows].float(), b], dim=1),
                    ROWS).bfloat16()
    out = ops.rows_cat_pad_bf16(a, b, n_rows, ROWS)
    assert out.dtype == torch.bfloat16 and out.shape == (ROWS, Da + Db)
    assert torch.equal(out, ref)
    assert bool((out[n_rows:] == 0).all())


# ------------------------------------------------------------- whole actor
ACTOR_CASES = [("DubinsCar", 3, 0), ("DubinsCar", 5, 2), ("SimpleDrone", 4, 0)]
ACTOR_IDS = ["dubins3", "dubins5obs2", "drone4"]


def _make_engine(case, glue, monkeypatch):
    """Fresh env, algo (random weights and biases, bf16) and captured
    engine; the same seeds give the same scene and weights every call."""
    from gcbf_amd.algo import make_algo
    from gcbf_amd.env import make_env
    from gcbf_amd.rollout import RolloutEngine
    from gcbf_amd.trainer.utils import set_seed
    from gcbf_amd.utils.amp import enable_bf16
    name, n, n_obs = case
    dev = torch.device("cuda")
    set_seed(3)
    params = make_env(name, n, dev).default_params
    params["num_obs"] = n_obs
    env = make_env(name, n, dev, params=params)
    env.train()
    algo = make_algo("gcbf", env, n, env.node_dim, env.edge_dim,
                     env.action_dim, dev, batch_size=32)
    with torch.no_grad():
        for p in algo.actor.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    enable_bf16(algo)
    env.reset()
    monkeypatch.setenv("GCBF_AMD_ACTOR_GLUE", "1" if glue else "0")
    eng = RolloutEngine(env, algo)
    assert eng._glue == glue
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
def test_actor_glue_equals_eager_composition(case, monkeypatch):
    """Eagerly on identical buffers, then three policy steps of a captured
    engine of each kind from the same start."""
    eng = _make_engine(case, True, monkeypatch)
    actor = eng.algo.actor
    if case[2] > 0:                          # agents_first_n path
        assert eng.agent_mask is not None and eng.N == case[1] + case[2]
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
    for t in range(3):
        done_new = eng.step(prob=0.0)       # rand() < 0 never: policy graph
        done_ref = ref_eng.step(prob=0.0)
        assert done_new == done_ref and not done_new
        assert eng.E == ref_eng.E
        for k in ("states", "u_ref", "ei", "seg", "ea"):
            assert torch.equal(getattr(eng, k)[eng.cur],
                               getattr(ref_eng, k)[ref_eng.cur]), \
                f"step {t}: {k}"
    assert bool((eng.states[eng.cur] != eng.states[1 - eng.cur]).any())


# ---------------------------------------------------------- mirror refresh
@pytest.mark.gpu
def test_refresh_mirrors_equals_per_layer():
    from gcbf_amd.nn import fused
    torch.manual_seed(2)
    net = torch.nn.Sequential(
        torch.nn.Linear(9, 128),            # K padded to 64
        torch.nn.Linear(128, 1),
        torch.nn.Linear(70, 128, bias=False)).cuda()
    for lin in net:
        fused._mirror(lin)

    def tensors(m):
        return [t for lin in m for t in lin._bf16_mirror[1:] if t is not None]

    ptrs = [t.data_ptr() for t in tensors(net)]
    idents = [id(t) for t in tensors(net)]
    for round_ in range(2):
        with torch.no_grad():
            for p in net.parameters():
                p.add_(torch.randn_like(p) * 0.1)
        ref = copy.deepcopy(net)
        for lin in ref:
            fused._mirror(lin, force=True)
        for t in tensors(net):              # a stale value must not survive
            t.fill_(float("nan"))
        fused.sync_bf16_mirrors(net)
        assert net._mirror_table is not None, "one-launch path not taken"
        for lin, rlin in zip(net, ref):
            K = lin.weight.shape[1]
            for got, want in zip(lin._bf16_mirror[1:], rlin._bf16_mirror[1:]):
                assert (got is None) == (want is None)
                if got is not None:
                    assert got.dtype == want.dtype
                    assert torch.equal(got, want), f"round {round_}"
            assert torch.equal(lin._bf16_mirror[1][:, :K],
                               lin.weight.detach().bfloat16())
            assert bool((lin._bf16_mirror[1][:, K:] == 0).all())
            assert lin._bf16_mirror[0] == fused._mirror_version(lin)
            # the lazy path sees a fresh mirror and hands back the same one
            assert fused._mirror(lin)[0] is lin._bf16_mirror[1]
        assert [t.data_ptr() for t in tensors(net)] == ptrs
        assert [id(t) for t in tensors(net)] == idents
