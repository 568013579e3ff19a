"""Diagnostic v2: captured update engine — gradient and staleness probes.

    PYTHONPATH=. python tools/upde_repro.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

os.environ["GCBF_AMD_UPDATE_CAPTURE"] = "1"      # engine is opt-in
os.environ["GCBF_AMD_UPDATE_CAPTURE_DEBUG"] = "1"

from gcbf_amd.env import make_env
from gcbf_amd.algo import make_algo
from gcbf_amd.algo.gcbf import cbf_losses
from gcbf_amd.graph import GraphBatch
from gcbf_amd.rollout import RolloutEngine
from gcbf_amd.trainer.utils import set_seed
from gcbf_amd.utils.amp import enable_bf16

set_seed(11)
dev = torch.device("cuda")
env = make_env("DubinsCar", 16, dev)
env.train()
algo = make_algo("gcbf", env, 16, env.node_dim, env.edge_dim,
                 env.action_dim, dev, batch_size=512)
enable_bf16(algo)
env.reset()
eng = RolloutEngine(env, algo)
for _ in range(512):
    if eng.step(prob=0.7):
        eng.reload()
algo.update(512)
e = algo._upd_engine
print("engine:", type(e).__name__ if e else None)
assert e is not None
for _ in range(512):
    if eng.step(prob=0.7):
        eng.reload()

names = [f"cbf.{n}" for n, p in algo.cbf.named_parameters()
         if p.requires_grad] + \
        [f"actor.{n}" for n, p in algo.actor.named_parameters()
         if p.requires_grad]


def eager_loss(gl):
    """GCBF._iter_eager's loss on the ring batch (no optimizer step)."""
    graphs = algo._ring.batch(gl)   # buffer snaps are metadata-only
    actions = algo.actor(graphs)
    graphs_next = env.forward_graph(graphs, actions)
    both = GraphBatch.from_list([graphs, graphs_next])
    h_both = algo.cbf(both)
    n_ag = h_both.shape[0] // 2
    h, h_next = h_both[:n_ag], h_both[n_ag:]
    with torch.no_grad():
        relinked = env.add_communication_links_batched(graphs_next.detach())
        h_new = algo.cbf(relinked)
    h_dot = (h_next - h) / env.dt
    residue = ((h_new - h) / env.dt - h_dot).detach()
    loss, log7 = cbf_losses(h, residue + h_dot, actions,
                            env.unsafe_mask(graphs), env.safe_mask(graphs),
                            algo.params)
    return loss, list(log7[:4])


gl = algo._sample_batch()
params = [p for p in algo.cbf.parameters() if p.requires_grad] + \
         [p for p in algo.actor.parameters() if p.requires_grad]

def run_graphed():
    e.gFront.replay()
    assert int(e._ecounts.max().cpu()) <= e.E_cap
    return e._graphed(e._nodes, e._uref, e._ei, e._ea, e._seg, e._h_new,
                      e.w_dev)

# ---- probe 0: FRONT outputs vs ring-materialized batch (same sample)
e._fill_inputs(gl)
e.gFront.replay()
mat = algo._ring.batch(gl)
L = len(gl)
nA = L * e.n
print("uref maxdiff  :", (e._uref[:nA] - mat.u_ref).abs().max().item())
print("nodes maxdiff :",
      (e._nodes[:L * e.N] - mat.states).abs().max().item())
with torch.no_grad():
    from gcbf_amd.graph import GraphBatch
    gchk = GraphBatch(x=e.x_tile, pos=e._nodes[:, :e.pd], states=e._nodes,
                      edge_index=e._ei, edge_attr=e._ea,
                      agent_mask=e.agent_mask_tile, u_ref=e._uref,
                      ptr=e.ptr)
    gchk.seg_dst = e._seg
    gchk.agent_index = e.agent_index
    a_front = algo.actor(gchk)          # eager actor on FRONT buffers
    a_mat = algo.actor(mat)             # eager actor on ring batch
print("eager-actor(front bufs) vs eager-actor(ring batch) maxdiff:",
      (a_front[:nA] - a_mat).abs().max().item())
print("mean |a|^2 front:", a_front[:nA].pow(2).sum(1).mean().item(),
      " ring:", a_mat.pow(2).sum(1).mean().item())

# ---- probe 1: replayed grads vs eager grads on the SAME batch
e._fill_inputs(gl)
lcap, log_cap = run_graphed()
algo._zero_grad()
lcap.backward()
g_cap = [p.grad.clone() for p in params]
log_cap = log_cap.clone()

loss, parts = eager_loss(gl)
g_eag = torch.autograd.grad(loss, params)
print("log7 cap :", [round(float(x), 5) for x in log_cap[:4]])
print("loss eag :", [round(float(x), 5) for x in parts])
rows = []
for n, a, b in zip(names, g_cap, g_eag):
    an, bn = a.float().norm().item(), b.float().norm().item()
    cos = torch.nn.functional.cosine_similarity(
        a.float().flatten(), b.float().flatten(), dim=0).item()
    rows.append((cos, n, an, bn))
rows.sort()
print("worst grad cosines:")
for cos, n, an, bn in rows[:8]:
    print(f"  {cos:+.4f} {n}  |cap|={an:.3e} |eag|={bn:.3e}")
print(f"median cosine: {sorted(r[0] for r in rows)[len(rows)//2]:+.4f}")

# ---- probe 2: does the captured forward see weight changes?
for p, g in zip(params, g_cap):
    p.grad = g
algo._optimizer_step()
e._fill_inputs(gl)
_, log_cap2 = run_graphed()
log_cap2 = log_cap2.clone()
with torch.no_grad():
    pass
loss2, parts2 = eager_loss(gl)
print("post-step cap:", [round(float(x), 5) for x in log_cap2[:4]])
print("post-step eag:", [round(float(x), 5) for x in parts2])

# ---- probe 3: replay determinism (same weights, same inputs)
_, log_cap3 = run_graphed()
print("replay determinism maxdiff:",
      (log_cap3 - log_cap2).abs().max().item())
