"""Record tests/golden/reference_parity.pt from the EXECUTING reference.

    python tools/ref_baseline/record_parity_golden.py --ref <reference checkout>

Runs the unmodified reference (MIT-REALM/gcbf-pytorch) through the
dependency shim (pygshim.py) on fixed, seeded inputs and stores the inputs
together with the reference's outputs.  tests/test_reference_parity.py
replays the same inputs through gcbf_amd and compares, so the suite needs
no reference checkout.  The file holds data only (tensors, numbers, lists).

Network weights are not stored (12M parameters per GNN): they come from
``seeded_net`` in the test module, loaded here into the reference nets with
a strict state-dict load (the layouts are key-compatible); a per-tensor
fingerprint is stored instead.

Re-run after any intended change to the networks' initialisation, the
environments' default parameters or the shim.
"""
import argparse
import importlib
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))


def _random_graph(n=8, node_dim=4, edge_dim=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    states = torch.randn(n, 4, generator=g)
    x = torch.zeros(n, node_dim)
    src, dst = [], []
    for i in range(n):
        for j in range(n):
            if i != j and (i + j) % 3 != 0:
                src.append(j)
                dst.append(i)
    ei = torch.tensor([src, dst], dtype=torch.long)
    ea = torch.randn(ei.shape[1], edge_dim, generator=g)
    return {"x": x, "states": states, "edge_index": ei, "edge_attr": ea}


def _edges(d):
    return sorted(map(tuple, d.edge_index.t().tolist()))


def _masks(env, d):
    return {name: getattr(env, name)(d).bool().clone()
            for name in ("safe_mask", "unsafe_mask", "collision_mask")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True,
                    help="checkout of the reference (MIT-REALM/gcbf-pytorch)")
    ap.add_argument("--out", default=os.path.join(
        REPO, "tests", "golden", "reference_parity.pt"))
    args = ap.parse_args()

    sys.path[:0] = [REPO, os.path.join(REPO, "tests"), HERE]
    import pygshim
    pygshim.install()
    sys.path.insert(0, os.path.abspath(args.ref))
    from test_reference_parity import seeded_net, weight_fingerprint
    Data = sys.modules["torch_geometric.data"].Data

    from gcbf_amd.algo.gcbf import CBFGNN as MyCBFGNN
    from gcbf_amd.algo.macbf import CBFNet as MyCBFNet
    from gcbf_amd.controller import GNNController as MyCtrl
    from gcbf_amd.controller import MACBFController as MyMC
    from gcbf_amd.env import make_env

    ref_gcbf = importlib.import_module("gcbf.algo.gcbf")
    ref_ctrl = importlib.import_module("gcbf.controller.gnn_controller")
    ref_macbf = importlib.import_module("gcbf.algo.macbf")
    ref_mc = importlib.import_module("gcbf.controller.macbf_controller")
    ref_sc = importlib.import_module("gcbf.env.simple_car")
    ref_dc = importlib.import_module("gcbf.env.dubins_car")
    ref_sd = importlib.import_module("gcbf.env.simple_drone")
    ref_buffer = importlib.import_module("gcbf.algo.buffer")

    dev = torch.device("cpu")
    out = {}

    def ref_twin(ref_net, mine):
        ref_net.load_state_dict(mine.state_dict(), strict=True)
        return ref_net.eval()

    def ref_data(g, **extra):
        return Data(x=g["x"], pos=g["states"][:, :2], states=g["states"],
                    edge_index=g["edge_index"], edge_attr=g["edge_attr"],
                    **extra)

    # ---- CBFGNN forward / attention ----
    for name, seed, gseed in (("cbfgnn", 0, 0), ("attention", 21, 23)):
        mine = seeded_net(lambda: MyCBFGNN(num_agents=8, node_dim=4,
                                           edge_dim=5, phi_dim=256), seed)
        net = ref_twin(ref_gcbf.CBFGNN(num_agents=8, node_dim=4, edge_dim=5,
                                       phi_dim=256), mine)
        g = _random_graph(seed=gseed)
        with torch.no_grad():
            if name == "cbfgnn":
                g["h"] = net(ref_data(g)).clone()
            else:
                g["attention"] = net.attention(ref_data(g)).clone()
        g.update(seed=seed, weights=weight_fingerprint(mine))
        out[name] = g

    # ---- GNNController ----
    mine = seeded_net(lambda: MyCtrl(num_agents=8, node_dim=4, edge_dim=5,
                                     phi_dim=256, action_dim=2), 1)
    net = ref_twin(ref_ctrl.GNNController(num_agents=8, node_dim=4,
                                          edge_dim=5, phi_dim=256,
                                          action_dim=2), mine)
    g = _random_graph(seed=3)
    g["u_ref"] = torch.randn(8, 2, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        g["action"] = net(ref_data(g, u_ref=g["u_ref"])).clone()
    g.update(seed=1, weights=weight_fingerprint(mine))
    out["controller"] = g

    # ---- MACBF nets ----
    m_cbf = seeded_net(lambda: MyCBFNet(num_agents=8, node_dim=4,
                                        edge_dim=4), 2)
    m_ctrl = seeded_net(lambda: MyMC(num_agents=8, node_dim=4, edge_dim=4,
                                     phi_dim=128, action_dim=2), 3)
    r_cbf = ref_twin(ref_macbf.CBFNet(num_agents=8, node_dim=4, edge_dim=4),
                     m_cbf)
    r_ctrl = ref_twin(ref_mc.MACBFController(num_agents=8, node_dim=4,
                                             edge_dim=4, phi_dim=128,
                                             action_dim=2), m_ctrl)
    g = _random_graph(n=8, node_dim=4, edge_dim=4, seed=5)
    g["u_ref"] = torch.randn(8, 2, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        d = ref_data(g, u_ref=g["u_ref"])
        g["h"] = r_cbf(d).clone()
        g["action"] = r_ctrl(d).clone()
    g.update(seed=2, weights_cbf=weight_fingerprint(m_cbf),
             weights_ctrl=weight_fingerprint(m_ctrl))
    out["macbf"] = g

    # ---- SimpleCar: graph / u_ref / masks, then stepped dynamics ----
    def inject_simple_car(env, states, goal):
        env._t = 0
        env._goal = goal.clone()
        d = Data(x=torch.zeros_like(states), pos=states[:, :2],
                 states=states.clone())
        env._data = env.add_communication_links(d)
        return env._data

    def simple_car_scene(n, seed):
        torch.manual_seed(seed)
        side = make_env("SimpleCar", n, dev).default_params["area_size"]
        pos = torch.rand(n, 2) * side
        states = torch.cat([pos, 0.3 * torch.randn(n, 2)], dim=1)
        goal = torch.rand(n, 2) * side
        env = ref_sc.SimpleCar(n, dev)
        env.train()
        return env, {"states": states, "goal": goal, "area_size": side}

    env, g = simple_car_scene(8, 5)
    d = inject_simple_car(env, g["states"], g["goal"])
    g.update(edges=_edges(d), u_ref=env.u_ref(d).clone(), **_masks(env, d))
    out["simple_car_graph"] = g

    env, g = simple_car_scene(6, 7)
    inject_simple_car(env, g["states"], g["goal"])
    g.update(actions=[], next_states=[], rewards=[], dones=[])
    for i in range(5):
        action = 0.1 * torch.randn(6, 2)
        nd, r, done, info = env.step(action.clone())
        g["actions"].append(action)
        g["next_states"].append(nd.states.clone())
        g["rewards"].append(torch.as_tensor(r).clone())
        g["dones"].append(bool(done))
        if done:
            break
    out["simple_car_step"] = g

    # ---- DubinsCar with obstacles ----
    torch.manual_seed(11)
    n, n_obs = 8, 4
    p = make_env("DubinsCar", n, dev).default_params
    p["num_obs"] = n_obs
    env = ref_dc.DubinsCar(n, dev, params=p)
    env.train()
    side = p["area_size"]
    ag = torch.cat([torch.rand(n, 2) * side,
                    (torch.rand(n, 1) * 2 - 1) * torch.pi,
                    torch.rand(n, 1) * 0.5], dim=1)
    obs = torch.cat([torch.rand(n_obs, 2) * side,
                     torch.zeros(n_obs, 2)], dim=1)
    states = torch.cat([ag, obs], dim=0)
    goal = torch.cat([torch.rand(n, 2) * side, torch.zeros(n, 2)], dim=1)
    agent_mask = torch.zeros(n + n_obs, dtype=torch.bool)
    agent_mask[:n] = True
    x = torch.cat([torch.zeros(n, 4), torch.ones(n_obs, 4)], dim=0)
    env._goal = goal.clone()
    d = env.add_communication_links(
        Data(x=x, pos=states[:, :2], states=states.clone(),
             agent_mask=agent_mask))
    key = d.edge_index[0] * (n + n_obs) + d.edge_index[1]
    out["dubins"] = dict(
        n=n, n_obs=n_obs, x=x, states=states, goal=goal,
        agent_mask=agent_mask,
        params={k: v for k, v in p.items()
                if isinstance(v, (int, float, bool))},
        edges=_edges(d), edge_attr_sorted=d.edge_attr[torch.argsort(key)],
        u_ref=env.u_ref(d).clone(), **_masks(env, d))

    # ---- SimpleDrone (the reference spawns num_agents obstacles) ----
    torch.manual_seed(13)
    n = 6
    side = make_env("SimpleDrone", n, dev).default_params["area_size"]
    env = ref_sd.SimpleDrone(n, dev)
    env.train()
    ag = torch.cat([torch.rand(n, 3) * side, 0.2 * torch.randn(n, 3)],
                   dim=1)
    obs = torch.zeros(n, 6)
    obs[:, :3] = torch.rand(n, 3) * side
    states = torch.cat([ag, obs], dim=0)
    goal = torch.cat([torch.rand(n, 3) * side, torch.zeros(n, 3)], dim=1)
    agent_mask = torch.zeros(2 * n, dtype=torch.bool)
    agent_mask[:n] = True
    x = torch.cat([torch.zeros(n, 4), torch.ones(n, 4)], dim=0)
    env._goal = goal.clone()
    env._obs = obs.clone()
    d = env.add_communication_links(
        Data(x=x, pos=states[:, :3], states=states.clone(),
             agent_mask=agent_mask))
    out["simple_drone"] = dict(
        n=n, area_size=side, x=x, states=states, goal=goal, obs=obs,
        agent_mask=agent_mask, edges=_edges(d),
        u_ref=env.u_ref(d).clone(), **_masks(env, d))

    # ---- replay-buffer sampling index streams ----
    class _Tag:
        def __init__(self, i):
            self.i = i
        ring_id = None

    rb = ref_buffer.Buffer()
    for i in range(200):
        rb.append(_Tag(i), is_safe=(i % 3 != 0))
    g = {}
    for balanced in (False, True):
        np.random.seed(42)
        random.seed(43)
        drawn = rb.sample(20, 3, balanced) if balanced else rb.sample(20, 3)
        g["balanced" if balanced else "plain"] = [t.i for t in drawn]
    out["buffer"] = g

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    torch.save(out, args.out)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
