"""Branch-covering parity tests for graph_build.hip / graph_build_common.h.

Hand-built scenes (tests/graph_build_scenes.py) against an fp64 loop over
graph, receiver and sender written out in the test code.  The un-marked
tests run anywhere: every scene (a) keeps every non-self pair at least
1e-4*r away from the radius and, in capped rows, every distance either equal
to the k-th or 1e-4*r away from it (declared exact cases excepted: those use
coordinates that are multiples of 1/8 and must then be exact), (b) fires the
branch it is named for and (c) is reproduced by the eager fp32 CPU builder.
The @pytest.mark.gpu tests compare ``ops.build_graph`` and
``_C.build_graph_padded`` with the same reference: edge lists with
torch.equal, ATTR_DIFF and the first three ATTR_DUBINS columns with
torch.equal against the fp32 CPU subtraction (one IEEE operation).

ATTR_DUBINS columns 3, 4 (v cos th, v sin th differences).  The HIP
documentation installed with the toolchain carries no ulp table for cosf /
sinf, so the allowance is the measured one: largest error of the eager fp32
CPU edge_attr against fp64 over the two Dubins scenes, as printed by
test_eager_fp32_matches_fp64 (-s):

    dubins_dense   1.93e-07      dubins_sparse   5.27e-08

DUBINS_EAGER_ERR is that figure; both the eager check and the kernel check
allow 4x it (the kernel may contract one multiply-subtract that eager does
not).
"""
import functools

import pytest
import torch

from gcbf_amd import ops
from gcbf_amd.env.dubins_car import DubinsCar
from gcbf_amd.env.point_agent import PointAgentEnv
from gcbf_amd.ops import eager

import graph_build_scenes as gs

DUBINS_EAGER_ERR = 1.93e-7
DUBINS_TOL = 4 * DUBINS_EAGER_ERR

SCENES = gs.scenes()
KEYS = sorted(SCENES)
CAP_KEYS = [k for k in KEYS if k.startswith("cap_")]
PADDED_KEYS = CAP_KEYS + ["dubins_dense", "isolation"]


@functools.lru_cache(maxsize=None)
def _ref(key, k="scene"):
    sc = SCENES[key]
    edges, rows = gs.ref_rows(sc, k)
    ei = gs.ref_edge_index(sc, k)
    assert ei.shape[1] == len(edges)
    return ei, rows, gs.ref_attr64(sc, ei)


def _attr_fn(sc):
    """The env's own eager edge_attr function for the scene's kind."""
    cls = DubinsCar if sc["attr"] == gs.ATTR_DUBINS else PointAgentEnv
    return functools.partial(cls.edge_attr, None)


def _attr_dim(sc):
    return 5 if sc["attr"] == gs.ATTR_DUBINS else sc["S"]


def _sub32(sc, ei, cols=None):
    """fp32 CPU subtraction states[src] - states[dst]."""
    s = sc["states"] if cols is None else sc["states"][:, :cols]
    return s[ei[0]] - s[ei[1]]


def _check_attr(sc, got, ei, ref64):
    """``got`` (E, A) fp32 on CPU against the references; returns the
    largest error of the two trigonometric columns (0.0 for ATTR_DIFF)."""
    assert got.dtype == torch.float32 and got.shape == ref64.shape
    if sc["attr"] == gs.ATTR_DIFF:
        assert torch.equal(got, _sub32(sc, ei))
        return 0.0
    assert torch.equal(got[:, :3], _sub32(sc, ei, 3))
    err = (got[:, 3:].double() - ref64[:, 3:]).abs()
    worst = err.max().item() if err.numel() else 0.0
    assert worst <= DUBINS_TOL, f"dubins attr err {worst:.3e} > {DUBINS_TOL}"
    return worst


# ------------------------------------------------- (a) margins, all scenes
@pytest.mark.parametrize("key", KEYS)
def test_scene_margins(key):
    sc = SCENES[key]
    _, rows, _ = _ref(key)
    r, tol = sc["r"], gs.MARGIN * sc["r"]
    seen_exact, seen_ties = set(), set()
    for (b, i), row in rows.items():
        for j, d in enumerate(row["d"]):
            if j == i:
                continue
            if (b, i, j) in sc["exact"]:
                assert d == r, (key, b, i, j, d)
                seen_exact.add((b, i, j))
            else:
                assert abs(d - r) >= tol, (key, b, i, j, d)
        if row["kth"] is None:
            continue
        gaps = [abs(d - row["kth"]) for d in row["d"]]
        assert all(g == 0.0 or g >= tol for g in gaps), (key, b, i, gaps)
        n_at_kth = sum(g == 0.0 for g in gaps)
        if (b, i) in sc["ties"]:
            assert n_at_kth > 1, (key, b, i)
            seen_ties.add((b, i))
        else:
            assert n_at_kth == 1, (key, b, i, n_at_kth)
    # a declared exact case must exist
    assert seen_exact == sc["exact"] and seen_ties == sc["ties"]
    # exact cases use coordinates that are multiples of 1/8
    if sc["exact"] or sc["ties"]:
        near = sc["states"][:, :sc["P"]]
        near = near[(near.abs() < 9).all(dim=1)]
        assert torch.equal(near * 8, (near * 8).round())


# --------------------------------------- (b) each scene fires its branch
def _deg(rows, b, i):
    return len(rows[(b, i)]["keep"])


def _fires_lanes(sc, ei, rows):
    N = sc["N"]
    assert all(_deg(rows, 0, i) == N - 1 for i in range(N))   # full ballots
    assert _deg(rows, 1, 0) == 0
    assert rows[(1, 1)]["keep"] == [N - 1]
    assert N - 1 >= {63: 62, 64: 63, 65: 64, 130: 128}[N]
    assert ei.shape[1] == N * (N - 1) + 2
    diam = max(max(d for j, d in enumerate(rows[(0, i)]["d"]) if j != i)
               for i in range(N))
    assert diam < sc["r"] / 2


def _fires_partial_wg(sc, ei, rows):
    assert sc["B"] * sc["n_rec"] == 15 and 15 % 4 != 0
    for b in range(3):
        assert rows[(b, 2)]["keep"] == [5] and rows[(b, 4)]["keep"] == [6]
        assert rows[(b, 0)]["keep"] == [1] and _deg(rows, b, 3) == 0
    local_dst = ei[1] % sc["N"]
    assert (local_dst < sc["n_rec"]).all()
    assert ((ei[0] % sc["N"]) >= sc["n_rec"]).sum() == 6
    # rows >= n_rec would receive if they were receivers
    full = dict(sc, n_rec=sc["N"])
    assert gs.ref_edge_index(full).shape[1] == ei.shape[1] + 6


def _fires_isolation(sc, ei, rows):
    N = sc["N"]
    pos = sc["states"][:, :2]
    assert torch.equal(pos[:5], pos[N:N + 5])          # on top of each other
    assert (ei[0] // N == ei[1] // N).all()            # no cross-graph edge
    g1 = ei[:, ei[1] >= N]
    assert g1.shape[1] > 0 and (g1 >= N).all()         # ids carry gbase
    assert _deg(rows, 0, 5) > 0 and _deg(rows, 1, 5) == 0


def _fires_strict_radius(sc, ei, rows):
    assert rows[(0, 0)]["d"][1] == sc["r"] == 1.25
    assert ei.t().tolist() == [[3, 2], [2, 3]]
    assert abs(rows[(0, 2)]["d"][3] / sc["r"] - (1 - 1e-3)) < 1e-6


def _fires_cap_line(sc, ei, rows):
    k, N, r = sc["k"], sc["N"], sc["r"]
    free = gs.ref_edge_index(sc, None)
    in_range = {i: sum(d < r for d in rows[(0, i)]["d"]) for i in range(N)}
    if k == 1:
        assert rows[(0, 0)]["kth"] < r and in_range[0] == 2
        assert _deg(rows, 0, 0) == 1                   # the cap binds
        assert rows[(0, 5)]["kth"] > r and _deg(rows, 0, 5) == 0
        assert all(_deg(rows, 0, i) <= 1 for i in range(N))
    elif k == 2:
        assert rows[(0, 1)]["kth"] < r and in_range[1] == 3
        assert _deg(rows, 0, 1) == 2
        assert rows[(0, 4)]["kth"] > r and _deg(rows, 0, 4) == in_range[4] == 1
    elif k == N - 1:
        assert all(rows[(0, i)]["kth"] > r for i in range(N))
        assert torch.equal(ei, free)
    else:
        assert k >= N and all(rows[(0, i)]["kth"] is None for i in range(N))
        assert torch.equal(ei, free)
    if k < N - 1:
        assert ei.shape[1] < free.shape[1]


def _fires_cap_tie70(sc, ei, rows):
    row = rows[(0, 0)]
    assert sc["N"] == 70 and sc["k"] == 5
    assert [j for j, d in enumerate(row["d"]) if d == row["kth"]] \
        == [62, 63, 64, 65]                            # straddles lane 63|64
    assert row["keep"] == [1, 2, 3, 62, 63, 64, 65]    # 7 edges for k = 5
    assert row["kth"] < row["d"][66] < sc["r"]         # dropped by the cap


def _fires_cap_colocated(sc, ei, rows):
    for i in range(3):
        assert sorted(rows[(0, i)]["d"])[:2] == [0.0, 0.0]
        assert rows[(0, i)]["kth"] == 0.0
        assert _deg(rows, 0, i) == 2
    assert _deg(rows, 0, 3) == 3 and sc["k"] < 3       # more than k edges


def _fires_cap_nrec(sc, ei, rows):
    assert sc["B"] == 2 and sc["n_rec"] < sc["N"] and sc["k"] == 2
    free, _ = gs.ref_rows(sc, None)
    assert len(free) > ei.shape[1]                     # the cap binds
    assert ((ei[0] % sc["N"]) >= sc["n_rec"]).any()    # an obstacle sender
    assert (ei[1] >= sc["N"]).any()
    assert all(_deg(rows, b, i) <= 2 for b in range(2) for i in range(5))


def _fires_dubins(sc, ei, rows):
    N, n = sc["N"], sc["n_rec"]
    th, v = sc["states"][:, 2], sc["states"][:, 3]
    for special in (100.0, -50.0, 0.0, torch.tensor(torch.pi).item()):
        assert (th == special).any()
    assert th[:10].min() == -8 and th[:10].max() == 8
    for special in (0.0, 1.5, -1.5):
        assert (v == special).any()
    if sc["name"] == "dubins_dense":
        assert ei.shape[1] == 2 * n * (N - 1)
        assert set(ei[0].tolist()) == set(range(2 * N))  # every node sends
    else:
        assert ei.t().tolist() == [[1, 0], [12, 0], [0, 1], [12, 1]]


_FIRES = {"lanes": _fires_lanes, "partial_wg": _fires_partial_wg,
          "isolation": _fires_isolation,
          "strict_radius": _fires_strict_radius, "cap_line": _fires_cap_line,
          "cap_tie70": _fires_cap_tie70,
          "cap_colocated": _fires_cap_colocated, "cap_nrec": _fires_cap_nrec,
          "dubins": _fires_dubins}


@pytest.mark.parametrize("key", KEYS)
def test_scene_fires_its_branch(key):
    sc = SCENES[key]
    ei, rows, _ = _ref(key)
    fire = [f for name, f in _FIRES.items() if key.startswith(name)]
    assert len(fire) == 1
    fire[0](sc, ei, rows)
    # edges are ordered (graph, dst, src)
    order = (ei[1] * sc["B"] * sc["N"] + ei[0]).tolist()
    assert order == sorted(order) and len(set(order)) == len(order)


# --------------------------------- (c) eager fp32 CPU path vs fp64 reference
@pytest.mark.parametrize("key", KEYS)
def test_eager_fp32_matches_fp64(key):
    sc = SCENES[key]
    ref_ei, _, ref_ea = _ref(key)
    pos = sc["states"][:, :sc["P"]].contiguous()
    ei = eager.dense_radius_graph(pos, gs.agent_mask(sc), sc["r"], sc["k"],
                                  sc["B"])
    assert torch.equal(ei, ref_ei)
    # the CPU branch of the dispatcher
    n_rec = None if sc["n_rec"] == sc["N"] else sc["n_rec"]
    ei2, ea = ops.build_graph(pos, sc["states"], n_rec, sc["r"], sc["k"],
                              sc["B"], sc["attr"], _attr_dim(sc),
                              _attr_fn(sc))
    assert torch.equal(ei2, ref_ei)
    worst = _check_attr(sc, ea, ref_ei, ref_ea)
    # every column is within one fp32 rounding of fp64 where it is a plain
    # subtraction
    plain = ea if sc["attr"] == gs.ATTR_DIFF else ea[:, :3]
    ref_plain = ref_ea[:, :plain.shape[1]]
    assert ((plain.double() - ref_plain).abs()
            <= 2.0 ** -24 * ref_plain.abs()).all()
    if sc["attr"] == gs.ATTR_DUBINS:
        print(f"\neager fp32 dubins attr vs fp64 {key}: {worst:.2e}")


def test_cap_at_or_above_N_is_no_cap():
    free = _ref("cap_line_k6", None)[0]
    for key in ("cap_line_k5", "cap_line_k6", "cap_line_k9"):
        assert torch.equal(_ref(key)[0], free)


# ------------------------------------------------------- GPU: build_graph
def _gpu_inputs(sc):
    st = sc["states"].cuda()
    return st[:, :sc["P"]].contiguous(), st


def _build_gpu(sc):
    pos, st = _gpu_inputs(sc)
    n_rec = None if sc["n_rec"] == sc["N"] else sc["n_rec"]
    return ops.build_graph(pos, st, n_rec, sc["r"], sc["k"], sc["B"],
                           sc["attr"], _attr_dim(sc), None)


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS)
def test_build_graph_kernel_matches_fp64(key):
    sc = SCENES[key]
    ref_ei, _, ref_ea = _ref(key)
    ei, ea = _build_gpu(sc)
    assert ei.dtype == torch.int64 and ei.shape == ref_ei.shape
    assert torch.equal(ei.cpu(), ref_ei)
    worst = _check_attr(sc, ea.cpu(), ref_ei, ref_ea)
    if sc["attr"] == gs.ATTR_DUBINS:
        print(f"\nkernel dubins attr vs fp64 {key}: {worst:.2e}")


@pytest.mark.gpu
def test_build_graph_without_receivers_is_empty():
    from gcbf_amd import _C
    sc = SCENES["isolation"]
    pos, st = _gpu_inputs(sc)
    ei, ea = _C.build_graph(pos, st, sc["B"], 0, sc["r"], -1, gs.ATTR_DIFF, 4)
    assert ei.shape == (2, 0) and ei.dtype == torch.int64
    assert ea.shape == (0, 4) and ea.dtype == torch.float32
    out = _C.build_graph_padded(pos, st, sc["B"], 0, sc["r"], -1,
                                gs.ATTR_DIFF, 4, 9)
    _check_padded(sc, out, torch.zeros(2, 0, dtype=torch.long),
                  torch.zeros(0, 4, dtype=torch.float64), 9)


# ------------------------------------------------ GPU: build_graph_padded
def _padded(sc, E_max, k="scene", out=None):
    from gcbf_amd import _C
    pos, st = _gpu_inputs(sc)
    k = sc["k"] if k == "scene" else k
    return _C.build_graph_padded(
        pos, st, sc["B"], sc["n_rec"], sc["r"], -1 if k is None else k,
        sc["attr"], _attr_dim(sc), E_max, out=out)


def _check_padded(sc, got, ref_ei, ref_ea, E_max):
    ei, seg, ea, ecount = [t.cpu() for t in got]
    E = ref_ei.shape[1]
    assert ei.shape == (2, E_max) and seg.shape == (E_max,)
    assert ea.shape == (E_max, _attr_dim(sc)) and ecount.shape == (1,)
    assert ecount.item() == E
    assert torch.equal(ei[:, :E], ref_ei)
    assert torch.equal(seg[:E], ref_ei[1])
    _check_attr(sc, ea[:E], ref_ei, ref_ea)
    # pads: src = dst = 0, seg = B*N, attr = 0, exactly
    assert (ei[:, E:] == 0).all()
    assert (seg[E:] == sc["B"] * sc["N"]).all()
    assert (ea[E:] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("key", PADDED_KEYS)
def test_build_graph_padded_fresh_buffers(key):
    sc = SCENES[key]
    ref_ei, _, ref_ea = _ref(key)
    E_max = ref_ei.shape[1] + 17
    _check_padded(sc, _padded(sc, E_max), ref_ei, ref_ea, E_max)


def _prefilled(E_max, A):
    return [torch.full((2, E_max), -7, dtype=torch.int64, device="cuda"),
            torch.full((E_max,), -7, dtype=torch.int64, device="cuda"),
            torch.full((E_max, A), float("nan"), device="cuda"),
            torch.full((1,), -1, dtype=torch.int32, device="cuda")]


@pytest.mark.gpu
@pytest.mark.parametrize("dense,sparse", [
    (("dubins_dense", "scene"), ("dubins_sparse", "scene")),
    (("cap_line_k1", None), ("cap_line_k1", "scene"))],
    ids=["dubins", "cap_line"])
def test_build_graph_padded_out_buffers_reused(dense, sparse):
    """One buffer set, as the engines use it: a dense scene, then a sparse
    one of the same shape.  No stale real edge may survive as a pad."""
    (dkey, dk), (skey, sk) = dense, sparse
    dsc, ssc = SCENES[dkey], SCENES[skey]
    d_ei, _, d_ea = _ref(dkey, dk)
    s_ei, _, s_ea = _ref(skey, sk)
    assert d_ei.shape[1] > s_ei.shape[1] + 3 and s_ei.shape[1] > 0
    assert dsc["states"].shape == ssc["states"].shape
    E_max = d_ei.shape[1] + 3
    bufs = _prefilled(E_max, _attr_dim(dsc))
    got = _padded(dsc, E_max, dk, out=bufs)
    assert all(g.data_ptr() == b.data_ptr() for g, b in zip(got, bufs))
    _check_padded(dsc, got, d_ei, d_ea, E_max)
    got = _padded(ssc, E_max, sk, out=bufs)
    assert all(g.data_ptr() == b.data_ptr() for g, b in zip(got, bufs))
    _check_padded(ssc, got, s_ei, s_ea, E_max)
    fresh = _padded(ssc, E_max, sk)
    for g, f in zip(got, fresh):
        assert torch.equal(g, f)                       # bit for bit, no NaN


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["cap_line_k2", "cap_tie70", "cap_nrec_b2"])
def test_build_graph_padded_exact_capacity_with_cap(key):
    sc = SCENES[key]
    ref_ei, _, ref_ea = _ref(key)
    E = ref_ei.shape[1]
    got = _padded(sc, E, out=_prefilled(E, _attr_dim(sc)))
    _check_padded(sc, got, ref_ei, ref_ea, E)


# ----------------------------------------------------- GPU: binding checks
@pytest.mark.gpu
def test_build_graph_bindings_reject_bad_arguments():
    """Every call must raise from the binding's checks, before any launch."""
    from gcbf_amd import _C
    sc = SCENES["isolation"]                           # B=2, N=6, S=4, P=2
    pos, st = _gpu_inputs(sc)
    B, n, r = 2, 6, 1.0
    st6 = torch.cat([st, st[:, :2]], dim=1).contiguous()
    pos5 = torch.cat([st, st[:, :1]], dim=1).contiguous()
    D, U = gs.ATTR_DIFF, gs.ATTR_DUBINS
    bad = {
        "pos fp64": (pos.double(), st, B, n, r, -1, D, 4),
        "states fp64": (pos, st.double(), B, n, r, -1, D, 4),
        "pos on CPU": (pos.cpu(), st, B, n, r, -1, D, 4),
        "pos not contiguous": (st[:, :2], st, B, n, r, -1, D, 4),
        "B = 0": (pos, st, 0, n, r, -1, D, 4),
        "rows % B": (pos, st, 5, 2, r, -1, D, 4),
        "states rows": (pos, st[:6].contiguous(), B, n, r, -1, D, 4),
        "P = 0": (pos[:, :0].contiguous(), st, B, n, r, -1, D, 4),
        "P > S": (pos5, st, B, n, r, -1, D, 4),
        "n_rec < 0": (pos, st, B, -1, r, -1, D, 4),
        "n_rec > N": (pos, st, B, n + 1, r, -1, D, 4),
        "attr_kind 2": (pos, st, B, n, r, -1, 2, 4),
        "attr_kind -1": (pos, st, B, n, r, -1, -1, 4),
        "diff attr_dim != S": (pos, st, B, n, r, -1, D, 5),
        "dubins S != 4": (pos, st6, B, n, r, -1, U, 5),
        "dubins attr_dim != 5": (pos, st, B, n, r, -1, U, 4),
    }
    for what, args in bad.items():
        with pytest.raises(RuntimeError):
            _C.build_graph(*args)
            pytest.fail(f"build_graph accepted: {what}")
        with pytest.raises(RuntimeError):
            _C.build_graph_padded(*args, 40)
            pytest.fail(f"build_graph_padded accepted: {what}")
    good = (pos, st, B, n, r, -1, D, 4)
    with pytest.raises(RuntimeError):
        _C.build_graph_padded(*good, -1)

    def out(**change):
        bufs = dict(zip(("ei", "seg", "ea", "ec"), _prefilled(40, 4)))
        bufs.update(change)
        return list(bufs.values())

    bad_out = {
        "edge_index int32": out(ei=torch.zeros(2, 40, dtype=torch.int32,
                                               device="cuda")),
        "seg int32": out(seg=torch.zeros(40, dtype=torch.int32,
                                         device="cuda")),
        "edge_attr fp64": out(ea=torch.zeros(40, 4, dtype=torch.float64,
                                             device="cuda")),
        "e_count int64": out(ec=torch.zeros(1, dtype=torch.int64,
                                            device="cuda")),
        "edge_attr columns": out(ea=torch.zeros(40, 5, device="cuda")),
        "e_count numel": out(ec=torch.zeros(2, dtype=torch.int32,
                                            device="cuda")),
        "E_max mismatch": out(seg=torch.zeros(39, dtype=torch.int64,
                                              device="cuda")),
        "three buffers": out()[:3],
    }
    for what, bufs in bad_out.items():
        with pytest.raises(RuntimeError):
            _C.build_graph_padded(*good, 40, out=bufs)
            pytest.fail(f"build_graph_padded accepted out: {what}")
    # the good call still goes through, into the given buffers
    bufs = out()
    got = _C.build_graph_padded(*good, 40, out=bufs)
    ref_ei, _, ref_ea = _ref("isolation")
    _check_padded(sc, got, ref_ei, ref_ea, 40)
