"""Branch-covering parity tests for env_step.hip, masks.hip, segops.hip and
segmax.hip.

Step and mask kernels are driven with hand-built scenes
(tests/kernel_branch_scenes.py) and compared with an fp64 reference written
out in the test code.  The un-marked tests run anywhere: they require that
every scene (a) keeps every decision at least 1e-3 away from its threshold,
(b) fires the branch it is named for and (c) is reproduced by the eager fp32
CPU path.  The @pytest.mark.gpu tests then compare the kernels with the same
reference; booleans exactly.

Float allowance of the GPU step comparisons: the project's atol (1e-5
states, 1e-4 u_ref, 1e-4 reward) plus rtol 1e-5 for the large clamped and
over-speed magnitudes.  Largest eager-fp32-CPU error against the fp64
reference over all scenes of an env, as printed by
test_step_scene_eager_fp32_matches_fp64 (-s):

    env          states    u_ref     reward
    DubinsCar    4.8e-07   2.7e-07   1.3e-07
    SimpleCar    3.5e-07   4.3e-06   1.6e-08
    SimpleDrone  2.2e-07   1.2e-06   7.3e-08

None exceeds its base atol, so the base values are used unchanged.

Segment attention (600-edge segment, gates randn*30+60): largest eager fp32
CPU error against fp64 over D in {3, 262, 1028}:
    out 5.8e-07   dmsg 6.2e-07   dgate 2.8e-06
within the existing 1e-5 (out, dmsg) / 1e-4 (dgate), which are used as is.
"""
import functools
import math
from unittest import mock

import pytest
import torch

from gcbf_amd import ops
from gcbf_amd.graph import GraphBatch

import kernel_branch_scenes as ks

ATOL = {"states": 1e-5, "u_ref": 1e-4, "reward": 1e-4}
RTOL = 1e-5

STEP_SCENES = {(s["env"], s["name"]): s for s in ks.step_scenes()}
STEP_KEYS = sorted(STEP_SCENES)
STEP_IDS = [f"{e}-{n}" for e, n in STEP_KEYS]


# ------------------------------------------------------------------ plumbing
def _inject(sc, dev):
    """Env holding the scene: goal, obstacle rows and a freshly linked
    graph of the scene's states."""
    from gcbf_amd.env import make_env
    env = make_env(sc["env"], len(sc["names"]), torch.device(dev))
    env.train()
    env._goal = sc["goal"].to(dev)
    env._obs = None if sc["env"] == "SimpleCar" else sc["obs"].to(dev)
    env._data = env.add_communication_links(
        env._build_data(sc["states"].to(dev)))
    return env


@functools.lru_cache(maxsize=None)
def _gain(env_name):
    """fp32 LQR gain the env itself builds (None for the PID Dubins car)."""
    sc = next(s for k, s in STEP_SCENES.items() if k[0] == env_name)
    K = _inject(sc, "cpu")._get_K_tensor()
    return None if K is None else K.clone()


@functools.lru_cache(maxsize=None)
def _step_ref(key):
    sc = STEP_SCENES[key]
    all_states = torch.cat([sc["states"], sc["obs"]], dim=0)
    return ks.REF_STEP[sc["env"]](all_states, sc["goal"], sc["action"],
                                  _gain(sc["env"]))


def _assert_close(name, got, ref):
    got, ref = got.double().cpu(), ref.double()
    err = (got - ref).abs()
    ok = err <= ATOL[name] + RTOL * ref.abs()
    assert bool(ok.all()), \
        f"{name}: max err {err.max().item():.3e} (atol {ATOL[name]})"
    return err.max().item()


# ------------------------------------------------- (a) margins, all scenes
@pytest.mark.parametrize("key", STEP_KEYS, ids=STEP_IDS)
def test_step_scene_margins(key):
    sc = STEP_SCENES[key]
    _, margins, _ = _step_ref(key)
    n = len(sc["names"])
    for mname, m in margins.items():
        bad = m.abs() < ks.MARGIN
        for pos in bad.nonzero().tolist():
            who = sc["names"][pos[0]] if m.shape[0] == n else f"row {pos[0]}"
            value = m[tuple(pos)].item()
            assert value == 0.0 and (mname, who) in sc["exact"], \
                f"{key}: margin {mname}[{who}{pos[1:]}] = {value:.3e}"
    # a declared exact tie must be one
    for mname, who in sc["exact"]:
        assert margins[mname][sc["idx"][who]].item() == 0.0, (mname, who)


# --------------------------------------- (b) each scene fires its branch
def _rew(c, reach_term, coll, cost):
    return reach_term * c["reach_rew"] - coll * c["coll_rew"] \
        + c["step_rew"] - cost


def _check_reach_freeze_collide_t1(sc, out, aux, c):
    i = sc["idx"]
    s64 = torch.cat([sc["states"], sc["obs"]]).double()
    k = i["reach_in"]
    assert not out["prev_reach"][k] and out["reach"][k]
    k = i["inside_moving"]
    assert out["prev_reach"][k] and out["reach"][k]
    assert s64[k, c["P"]:].abs().max() > 0.1          # it has velocity
    assert torch.equal(out["states"][k], s64[k])      # and stays frozen
    a, b = i["coll_a"], i["coll_b"]
    assert aux["dist_t"][a, b] > 2 * c["r"] > aux["dist_t1"][a, b]
    # with the neighbour left at t the pair would not touch
    assert aux["dist_nbr_t"][a, b] > 2 * c["r"]
    assert out["collision"][a] and out["collision"][b]
    assert out["collision"].sum() == 2


def _check_collide_t_only_frozen_nbr(sc, out, aux, c):
    i = sc["idx"]
    a, b = i["apart_a"], i["apart_b"]
    assert aux["dist_t"][a, b] < 2 * c["r"] < aux["dist_t1"][a, b]
    assert not out["collision"][a] and not out["collision"][b]
    f, x = i["frozen"], i["beside_frozen"]
    assert out["prev_reach"][f]
    assert aux["dist_t1"][x, f] < 2 * c["r"] < aux["dist_nbr_free"][x, f]
    assert out["collision"][x] and out["collision"][f]


def _check_obstacles(sc, out, aux, c):
    i = sc["idx"]
    n, n_obs = len(sc["names"]), sc["obs"].shape[0]
    assert n + n_obs > 64 and n_obs >= 2 * n + 1
    g, y = i["frozen_toward"], i["ahead_of_frozen"]
    assert out["prev_reach"][g]
    assert aux["dist_nbr_free"][y, g] < 2 * c["r"] < aux["dist_t1"][y, g]
    assert not out["collision"][y] and not out["collision"][g]
    if sc["env"] == "DubinsCar":
        h, node = i["hit_by_obstacle"], n + 63
        assert sc["obs"][63, 3] != 0                  # a moving obstacle
        k, capped = i["near_capped_obstacle"], n + 61
        assert sc["obs"][61, 3] > c["sl"]
        assert aux["dist_nbr_uncapped"][k, capped] < 2 * c["r"] \
            < aux["dist_t1"][k, capped]
        assert not out["collision"][k]
    else:
        h, node = i["hits_obstacle"], n + 63
        # static although its row carries a velocity
        assert sc["obs"][63, 3:].abs().max() > 1
        assert torch.equal(out["states"][node], sc["obs"][63].double())
    assert node >= 64
    assert aux["dist_t"][h, node] > 2 * c["r"] > aux["dist_t1"][h, node]
    assert out["collision"][h] and out["collision"].sum() == 1


def _check_clamped(sc, out, aux, c):
    i = sc["idx"]
    assert (sc["action"].abs() == 100).all()
    assert (out["a_plus_ur"].abs() > c["lim"] + 1).all()
    assert (out["u"].abs() == c["lim"]).all()
    v = sc["states"][:, c["P"]:]
    if sc["env"] == "DubinsCar":
        assert v[i["fast"], 1] > c["sl"] and v[i["fast_reverse"], 1] < -c["sl"]
        assert v[i["still"], 1] == 0
    else:
        assert v[i["fast"]].norm() > c["sl"] and aux["u_ref_t"]["over"][i["fast"]]
        assert aux["u_ref_t1"]["over"][i["fast"]]
        assert (v[i["still"]] == 0).all()
        assert not aux["u_ref_t"]["over"][i["still"]]


def _check_u_ref_quadrants(sc, out, aux, c):
    i, u = sc["idx"], aux["u_ref_t"]
    small, anti, clock = u["small"], u["anti"], u["clock"]
    assert small[i["le_pi_anti"]] and anti[i["le_pi_anti"]]
    assert small[i["le_pi_not_anti"]] and not anti[i["le_pi_not_anti"]]
    assert not small[i["gt_pi_clock"]] and clock[i["gt_pi_clock"]]
    assert not small[i["gt_pi_not_clock"]] and not clock[i["gt_pi_not_clock"]]
    k = i["negative_theta"]
    assert sc["states"][k, 2] < 0 and not small[k] and u["theta"][k] > 0
    assert u["sign"].tolist() == [1.0, -1.0, -1.0, 1.0, 1.0]


def _check_u_ref_edges(sc, out, aux, c):
    i, u = sc["idx"], aux["u_ref_t"]
    s, g = sc["states"], sc["goal"]
    assert s[i["over_two_pi"], 2] > ks.TWO_PI
    for k, side in ((i["goal_straight_left"], -1), (i["goal_straight_right"], 1)):
        assert s[k, 1] == g[k, 1] and (g[k, 0] - s[k, 0]) * side > 0.5
        assert out["states"][k, 1] == s[k, 1].double()     # dy stays 0
    # sign(0) = 0: the target heading collapses to 0 on both sides
    assert u["td"][i["goal_straight_left"]] == -u["theta"][i["goal_straight_left"]]
    k = i["on_goal"]
    assert (s[k, :2] == g[k, :2]).all() and out["prev_reach"][k]
    k = i["le_pi_td_over_pi"]
    assert u["small"][k] and u["td"][k] > math.pi and not u["anti"][k]


def _check_summed_action_cost(sc, out, aux, c):
    assert len(sc["names"]) == 70
    assert (sc["action"].norm(dim=1) > 0).sum() > 64


def _check_reach_leave_stay_collide_t1(sc, out, aux, c):
    i = sc["idx"]
    k = i["reach_in"]
    assert not out["prev_reach"][k] and out["reach"][k]
    k = i["inside_leaving"]
    assert out["prev_reach"][k] and not out["reach"][k]
    cost = c["act_cost"] * sc["action"][k].double().norm()
    assert out["reward"][k] == pytest.approx(_rew(c, -1, 0, cost), abs=1e-12)
    k = i["inside_staying"]
    assert out["prev_reach"][k] and out["reach"][k]
    assert not torch.equal(out["states"][k], sc["states"][k].double())
    a, b = i["coll_a"], i["coll_b"]
    assert aux["dist_t"][a, b] > 2 * c["r"] > aux["dist_t1"][a, b]
    assert aux["dist_nbr_t"][a, b] > 2 * c["r"]
    assert out["collision"].tolist() == [False, False, False, True, True]


def _check_collide_t_only_clamped(sc, out, aux, c):
    i = sc["idx"]
    a, b = i["apart_a"], i["apart_b"]
    assert aux["dist_t"][a, b] < 2 * c["r"] < aux["dist_t1"][a, b]
    assert not out["collision"].any()
    _check_clamped(sc, out, aux, c)


def _check_far_neighbour(sc, out, aux, c):
    i = sc["idx"]
    a, b = i["a2"], i["a67"]
    assert len(sc["names"]) == 70 and b >= 64
    assert aux["dist_t"][a, b] > 2 * c["r"] > aux["dist_t1"][a, b]
    assert out["collision"].nonzero().flatten().tolist() == [a, b]


_FIRES = {
    "reach_freeze_collide_t1": _check_reach_freeze_collide_t1,
    "collide_t_only_frozen_nbr": _check_collide_t_only_frozen_nbr,
    "obstacles": _check_obstacles,
    "clamped": _check_clamped,
    "u_ref_quadrants": _check_u_ref_quadrants,
    "u_ref_edges": _check_u_ref_edges,
    "summed_action_cost": _check_summed_action_cost,
    "reach_leave_stay_collide_t1": _check_reach_leave_stay_collide_t1,
    "collide_t_only_clamped": _check_collide_t_only_clamped,
    "far_neighbour": _check_far_neighbour,
}


@pytest.mark.parametrize("key", STEP_KEYS, ids=STEP_IDS)
def test_step_scene_fires_its_branch(key):
    sc = STEP_SCENES[key]
    out, _, aux = _step_ref(key)
    _FIRES[sc["name"]](sc, out, aux, ks.CONST[sc["env"]])
    if sc["name"] == "reach_freeze_collide_t1" and sc["env"] != "SimpleCar":
        # frozen on reach: no +/- reach reward
        c, k = ks.CONST[sc["env"]], sc["idx"]["inside_moving"]
        a = sc["action"].double().norm(dim=1)
        cost = c["act_cost"] * (a.sum() if sc["env"] == "DubinsCar" else a[k])
        assert out["reward"][k].item() == pytest.approx(
            _rew(c, 0, 0, cost).item(), abs=1e-12)


# --------------------------------- (c) eager fp32 CPU path vs fp64 reference
_EAGER_ERR = {}


@pytest.mark.parametrize("key", STEP_KEYS, ids=STEP_IDS)
def test_step_scene_eager_fp32_matches_fp64(key):
    sc = STEP_SCENES[key]
    out, _, _ = _step_ref(key)
    env = _inject(sc, "cpu")
    data, reward, _, info = env.step(sc["action"].clone())
    assert torch.equal(info["reach"], out["reach"])
    assert torch.equal(info["collision"], out["collision"])
    errs = (_assert_close("states", data.states, out["states"]),
            _assert_close("u_ref", env.u_ref(data), out["u_ref"]),
            _assert_close("reward", reward, out["reward"]))
    worst = _EAGER_ERR.setdefault(sc["env"], [0.0, 0.0, 0.0])
    for j, e in enumerate(errs):
        worst[j] = max(worst[j], e)
    print(f"\neager fp32 vs fp64 {key}: states {errs[0]:.2e} u_ref "
          f"{errs[1]:.2e} reward {errs[2]:.2e}; env max so far "
          + " ".join(f"{w:.2e}" for w in worst))


# ------------------------------------------------------ GPU: fused step
@pytest.mark.gpu
@pytest.mark.parametrize("key", STEP_KEYS, ids=STEP_IDS)
def test_step_kernel_matches_fp64(key):
    sc = STEP_SCENES[key]
    ref, _, _ = _step_ref(key)
    c = ks.CONST[sc["env"]]
    env = _inject(sc, "cuda")
    n, N = len(sc["names"]), env._data.states.shape[0]
    nan = float("nan")
    # NaN / inverted prefill: a row nobody writes cannot pass by luck
    bufs = [torch.full((N, c["S"]), nan, device="cuda"),
            torch.full((n, c["A"]), nan, device="cuda"),
            torch.full((n,), nan, device="cuda"),
            ~ref["reach"].cuda(), ~ref["collision"].cuda()]
    got = ops.env_step_fused(*env.fused_step_args(
        env._data.states, env._goal, sc["action"].cuda()), out=bufs)
    new_states, u_ref_next, reward, reach, collision = got
    assert new_states.data_ptr() == bufs[0].data_ptr()
    assert torch.equal(reach.cpu(), ref["reach"])
    assert torch.equal(collision.cpu(), ref["collision"])
    assert torch.isfinite(new_states).all()           # every row written
    _assert_close("states", new_states, ref["states"])
    _assert_close("u_ref", u_ref_next, ref["u_ref"])
    _assert_close("reward", reward, ref["reward"])
    frozen = ref["prev_reach"] if sc["env"] != "SimpleCar" \
        else torch.zeros(n, dtype=torch.bool)
    # frozen agents and drone obstacles are copied, bit for bit
    assert torch.equal(new_states.cpu()[:n][frozen], sc["states"][frozen])
    if sc["env"] == "SimpleDrone":
        assert torch.equal(new_states.cpu()[n:], sc["obs"])


@pytest.mark.gpu
@pytest.mark.parametrize("key", [("DubinsCar", "obstacles"),
                                 ("SimpleCar", "reach_leave_stay_collide_t1"),
                                 ("SimpleDrone", "obstacles")],
                         ids=["DubinsCar", "SimpleCar", "SimpleDrone"])
def test_env_step_fused_equals_eager_on_scene(key):
    """env.step end to end: the fused path and the eager path (kernel
    patched out) on the same injected scene."""
    sc = STEP_SCENES[key]
    ref, _, _ = _step_ref(key)
    res = []
    for fused in (True, False):
        env = _inject(sc, "cuda")
        if fused:
            data, reward, done, info = env.step(sc["action"].cuda())
            u_ref = data.u_ref
        else:
            with mock.patch.object(ops, "env_step_fused",
                                   lambda *a, **k: None):
                data, reward, done, info = env.step(sc["action"].cuda())
            u_ref = env.u_ref(data)
        res.append((data, reward, done, info, u_ref))
        assert torch.equal(info["reach"].cpu(), ref["reach"])
        assert torch.equal(info["collision"].cpu(), ref["collision"])
        _assert_close("states", data.states, ref["states"])
        _assert_close("u_ref", u_ref, ref["u_ref"])
        _assert_close("reward", reward, ref["reward"])
    assert res[0][2] == res[1][2]
    assert torch.equal(res[0][0].edge_index, res[1][0].edge_index)


# ------------------------------------------------------------------- masks
MASK_KEYS = [(e, s) for e in ("SimpleCar", "DubinsCar", "SimpleDrone")
             for s in ks.MASK_SCENES if ks.mask_scene(e, s) is not None]
MASK_IDS = [f"{e}-{s}" for e, s in MASK_KEYS]
WHICH = ("safe", "unsafe", "collision")


@functools.lru_cache(maxsize=None)
def _mask_case(key):
    sc = ks.mask_scene(*key)
    return sc, ks.ref_masks(sc["env"], sc["states"], ks.MASK_B, ks.MASK_NREC)


def _mask_data(sc, dev):
    from gcbf_amd.env import make_env
    env = make_env(sc["env"], ks.MASK_NREC, torch.device(dev))
    states = sc["states"].to(dev)
    B = ks.MASK_B
    N = states.shape[0] // B
    am = None
    if sc["env"] != "SimpleCar":
        am = torch.zeros(B, N, dtype=torch.bool, device=dev)
        am[:, :ks.MASK_NREC] = True
        am = am.view(-1)
    data = GraphBatch(
        x=torch.zeros(B * N, env.node_dim, device=dev),
        pos=states[:, :env.pos_dim], states=states, agent_mask=am,
        ptr=torch.arange(B + 1, device=dev) * N)
    return env, data


def _mask(env, data, which):
    return {"safe": env.safe_mask, "unsafe": env.unsafe_mask,
            "collision": env.collision_mask}[which](data)


@pytest.mark.parametrize("key", MASK_KEYS, ids=MASK_IDS)
def test_mask_scene_valid_and_eager_matches_fp64(key):
    sc, (out, margins, aux) = _mask_case(key)
    n = ks.MASK_NREC
    N = sc["states"].shape[0] // ks.MASK_B
    assert N == (5 if sc["env"] == "SimpleCar" else 70)
    # (a) margins
    for mname, m in margins.items():
        assert m.abs().min() >= ks.MARGIN, (key, mname, m.abs().min().item())
    # (b) the named rows of graph 1 decide as designed; graphs 0, 2 clean
    for which, rows in sc["expect"].items():
        for row, want in rows.items():
            assert out[which][n + row].item() == want, (key, which, row)
    for b in (0, 2):
        rows = slice(b * n, (b + 1) * n)
        assert out["safe"][rows].all()
        assert not out["unsafe"][rows].any()
        assert not out["collision"][rows].any()
    if sc["name"] == "overlap":
        assert aux["ratio"][1, 0, 1] > 1 and torch.isnan(aux["thr"][1, 0, 1])
    if sc["name"] == "zero_velocity":
        assert aux["inner"][1, 0, 1].abs() < 1e-6
    if sc["name"] == "drone_vz_quirk":
        assert aux["cone"][1, 0, 1] and not aux["cone_norm"][1, 0, 1]
    if sc["name"] == "far_obstacle":
        assert aux["d"][1, 0, 69] < 2 * ks.CONST[sc["env"]]["r"]
        assert aux["cone"][1, 2, 66] and aux["cone"][1].sum() == 1
    # (c) eager fp32 on CPU
    env, data = _mask_data(sc, "cpu")
    for which in WHICH:
        assert torch.equal(_mask(env, data, which), out[which]), (key, which)


@pytest.mark.gpu
@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("key", MASK_KEYS, ids=MASK_IDS)
def test_mask_kernel_matches_eager_and_fp64(key, which):
    """Each mask requested alone (the other two output pointers null),
    B = 3 graphs of 5 receiver rows: a partial last workgroup."""
    sc, (out, _, _) = _mask_case(key)
    env, data = _mask_data(sc, "cuda")
    got = _mask(env, data, which)
    assert got.dtype == torch.bool and got.shape == (15,)
    with mock.patch.object(type(env), "_fused_mask", lambda self, d, w: None):
        eager = _mask(env, data, which)
    assert torch.equal(got, eager), (key, which)
    assert torch.equal(got.cpu(), out[which]), (key, which)


# ------------------------------------------------------- segment attention
SEG_N = 6
SEG_DEG = [3, 600, 0, 5, 1, 7]      # one 600-edge segment, one empty
SEG_PAD = 17


@functools.lru_cache(maxsize=None)
def _seg_case(D):
    g = torch.Generator().manual_seed(100 + D)
    dst = torch.repeat_interleave(torch.arange(SEG_N),
                                  torch.tensor(SEG_DEG))
    E = dst.numel()
    msg = torch.randn(E, D, generator=g)
    gate = torch.randn(E, 1, generator=g) * 30 + 60
    grad = torch.randn(SEG_N, D, generator=g)
    assert torch.isinf(gate.max().exp())          # raw exp overflows fp32
    return msg, gate, dst, grad


def _seg_attn_ref64(msg, gate, dst, grad):
    m = msg.double().requires_grad_(True)
    g = gate.double().requires_grad_(True)
    rows, att = [], torch.zeros(msg.shape[0], dtype=torch.float64)
    for seg in range(SEG_N):
        idx = (dst == seg).nonzero()[:, 0]
        if idx.numel():
            a = torch.softmax(g[idx, 0], dim=0)
            att[idx] = a.detach()
            rows.append((a[:, None] * m[idx]).sum(dim=0))
        else:
            rows.append(torch.zeros(msg.shape[1], dtype=torch.float64))
    out = torch.stack(rows)
    out.backward(grad.double())
    return out.detach(), m.grad, g.grad, att


def _close(got, ref, atol, what):
    err = (got.double().cpu() - ref).abs().max().item()
    assert err <= atol, f"{what}: max err {err:.3e} > {atol}"
    return err


@pytest.mark.parametrize("D", [3, 262, 1028])
def test_segment_attn_eager_fp32_matches_fp64(D):
    msg, gate, dst, grad = _seg_case(D)
    out64, dm64, dg64, _ = _seg_attn_ref64(msg, gate, dst, grad)
    m = msg.clone().requires_grad_(True)
    g = gate.clone().requires_grad_(True)
    out = ops.eager.segment_attn_aggregate(m, g, dst, SEG_N)
    out.backward(grad)
    errs = (_close(out, out64, 1e-5, "out"), _close(m.grad, dm64, 1e-5, "dmsg"),
            _close(g.grad, dg64, 1e-4, "dgate"))
    print(f"\neager fp32 segment_attn D={D}: out {errs[0]:.2e} dmsg "
          f"{errs[1]:.2e} dgate {errs[2]:.2e}")


def _with_sentinels(msg, gate, dst):
    """17 trailing pad edges: dst == num_nodes, NaN message rows."""
    pad_msg = torch.full((SEG_PAD, msg.shape[1]), float("nan"),
                         dtype=msg.dtype)
    pad_gate = torch.full((SEG_PAD, 1), 75.0)
    pad_dst = torch.full((SEG_PAD,), SEG_N, dtype=dst.dtype)
    return torch.cat([msg, pad_msg]), torch.cat([gate, pad_gate]), \
        torch.cat([dst, pad_dst])


@pytest.mark.gpu
@pytest.mark.parametrize("sentinels", [False, True], ids=["plain", "padded"])
@pytest.mark.parametrize("D", [3, 262, 1028])
def test_segment_attn_kernel_matches_fp64(D, sentinels):
    msg, gate, dst, grad = _seg_case(D)
    out64, dm64, dg64, att64 = _seg_attn_ref64(msg, gate, dst, grad)
    E = msg.shape[0]
    if sentinels:
        msg, gate, dst = _with_sentinels(msg, gate, dst)
    m = msg.cuda().requires_grad_(True)
    g = gate.cuda().requires_grad_(True)
    out = ops.segment_attn_aggregate(m, g, dst.cuda(), SEG_N)
    out.backward(grad.cuda())
    assert out.shape == (SEG_N, D)
    for t in (out, m.grad, g.grad):
        assert torch.isfinite(t).all()
    assert out[2].abs().max().item() == 0.0            # the empty segment
    _close(out, out64, 1e-5, "out")
    _close(m.grad[:E], dm64, 1e-5, "dmsg")
    _close(g.grad[:E], dg64, 1e-4, "dgate")
    from gcbf_amd import _C
    att, out2 = _C.segment_attn_fwd(
        msg.cuda(), gate.cuda().reshape(-1).contiguous(),
        ops._csr_ptr(dst.cuda(), SEG_N))
    assert torch.equal(out2, out.detach())
    _close(att[:E], att64, 1e-6, "att")
    if sentinels:
        assert (m.grad[E:] == 0).all() and (g.grad[E:] == 0).all()
        assert (att[E:] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("D", [3, 262, 1028])
def test_segment_attn_kernel_bf16_messages(D):
    """bf16 messages are upcast at the dispatch boundary; the gradient goes
    back in bf16."""
    msg, gate, dst, grad = _seg_case(D)
    msg = msg.bfloat16()
    out64, dm64, dg64, _ = _seg_attn_ref64(msg.float(), gate, dst, grad)
    m = msg.cuda().requires_grad_(True)
    g = gate.cuda().requires_grad_(True)
    out = ops.segment_attn_aggregate(m, g, dst.cuda(), SEG_N)
    out.backward(grad.cuda())
    # same dtypes as the eager op gives for the same inputs
    ref_dtype = ops.eager.segment_attn_aggregate(msg, gate, dst, SEG_N).dtype
    assert out.dtype == ref_dtype == torch.float32
    assert m.grad.dtype == torch.bfloat16 and g.grad.dtype == torch.float32
    for t in (out, m.grad, g.grad):
        assert torch.isfinite(t).all()
    _close(out, out64, 1e-5, "out")                    # computed in fp32
    _close(g.grad, dg64, 1e-4, "dgate")
    # dmsg is rounded to bf16 once: half an ulp, eps = 2^-8 relative
    err = (m.grad.double().cpu() - dm64).abs()
    assert bool((err <= 1e-5 + 2.0 ** -8 * dm64.abs()).all()), err.max()


# -------------------------------------------------------------- segment max
def _seg_max_case(E, n, D):
    """dst-sorted edges with an empty segment in the middle and at the end,
    an all-negative segment and an exact tie (a segment's maximal row
    repeated later in the same segment)."""
    g = torch.Generator().manual_seed(E + D)
    empty = {n // 2, n - 1}
    live = [s for s in range(n) if s not in empty]
    base = E // len(live)
    deg = [0] * n
    for s in live:
        deg[s] = base
    deg[live[0]] += E - base * len(live)
    dst = torch.repeat_interleave(torch.arange(n), torch.tensor(deg))
    vals = torch.randn(E, D, generator=g)
    neg = live[1]
    rows = (dst == neg).nonzero()[:, 0]
    vals[rows] = -vals[rows].abs() - 0.5
    tie = live[2]
    rows = (dst == tie).nonzero()[:, 0]
    first, second = rows[1].item(), rows[-1].item()
    vals[first] = vals[rows].max(dim=0).values + 1.0
    vals[second] = vals[first]
    grad = torch.randn(n, D, generator=g)
    return vals, dst, grad, dict(empty=sorted(empty), neg=neg, tie=tie,
                                 first=first, second=second)


def _check_seg_max(out, dval, vals, dst, grad, info, n):
    """Against a per-segment loop in fp64 (max is exact in any precision)."""
    D = vals.shape[1]
    want = torch.zeros(n, D, dtype=torch.float64)
    dwant = torch.zeros(vals.shape, dtype=torch.float64)
    for seg in range(n):
        idx = (dst == seg).nonzero()[:, 0]
        if idx.numel():
            mx, am = vals[idx].double().max(dim=0)
            # first maximal edge
            am = (vals[idx].double() == mx).int().argmax(dim=0)
            want[seg] = mx
            dwant[idx[am], torch.arange(D)] = grad[seg].double()
    assert torch.equal(out.double(), want)
    assert torch.equal(dval.double(), dwant)
    assert (out[info["empty"]] == 0).all()
    assert (out[info["neg"]] < 0).all()
    assert (dval[info["first"]] == grad[info["tie"]]).all()
    assert (dval[info["second"]] == 0).all()
    # the empty segments' gradient rows land nowhere
    live = torch.ones(n, dtype=torch.bool)
    live[info["empty"]] = False
    assert torch.equal(dval.double().sum(dim=0), dwant.sum(dim=0))
    assert (dval != 0).sum().item() == int(live.sum()) * D


SEG_MAX_SHAPES = [(40, 9, 1), (300, 7, 300)]


@pytest.mark.parametrize("E,n,D", SEG_MAX_SHAPES)
def test_segment_max_eager_matches_fp64(E, n, D):
    vals, dst, grad, info = _seg_max_case(E, n, D)
    v = vals.clone().requires_grad_(True)
    out = ops.segment_max(v, dst, n)
    out.backward(grad)
    _check_seg_max(out.detach(), v.grad, vals, dst, grad, info, n)


@pytest.mark.gpu
@pytest.mark.parametrize("E,n,D", SEG_MAX_SHAPES)
def test_segment_max_kernel_matches_eager_bitwise(E, n, D):
    vals, dst, grad, info = _seg_max_case(E, n, D)
    v = vals.cuda().requires_grad_(True)
    out = ops.segment_max(v, dst.cuda(), n)
    out.backward(grad.cuda())
    ve = vals.clone().requires_grad_(True)
    oute = ops._SegmentMax.apply(ve, dst, n)
    oute.backward(grad)
    assert torch.equal(out.detach().cpu(), oute.detach())
    assert torch.equal(v.grad.cpu(), ve.grad)
    _check_seg_max(out.detach().cpu(), v.grad.cpu(), vals, dst, grad, info, n)
