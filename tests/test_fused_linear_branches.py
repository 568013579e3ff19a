"""Branch-covering parity tests for fused_linear.hip (the MFMA bf16 linear).

Integer GEMMs (tests/fused_linear_cases.py) are compared position by
position with no tolerance: every product and partial sum is an integer
below 2^24, so fp32 accumulation is exact in any order, and a swapped, stale
or missing K tile, a wrong fragment offset or a wrong block index changes
the sum.  Real-valued GEMMs on bf16-rounded operands are compared with an
fp64 reference under the standard summation bound
(K + 2) * 2^-24 * (|A| |W|^T + |b|) per element.

Epilogues: relu and tanh are 1-Lipschitz, so the pre-activation bound
carries over; the bf16 store adds 2^-8 * |ref| (one rounding, 8 significand
bits).  tanhf's own error: the HIP documentation installed with the
toolchain carries no ulp table, so the allowance is the measured one,
largest error of the fp32 CPU ``torch.tanh`` against fp64 ``tanh`` on the
fp32-rounded reference pre-activations of the two real shapes, as printed by
test_real_cases_and_eager_fp32 (-s):

    (128, 192, 128)   3.18e-08      (256, 2048, 128)   3.17e-08

TANH_EAGER_ERR is that figure and 4x it is allowed.

The un-marked tests validate the operands and the fp32 CPU path against the
same references; the @pytest.mark.gpu tests run the kernel.
"""
import pytest
import torch
import torch.nn.functional as F

import fused_linear_cases as fc

ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2
TANH_EAGER_ERR = 3.18e-8
TANH_TOL = 4 * TANH_EAGER_ERR
BF16_EPS = 2.0 ** -8

INT_IDS = ["x".join(map(str, s)) for s in fc.INT_SHAPES]
REAL_IDS = ["x".join(map(str, s)) for s in fc.REAL_SHAPES]
BF16_OUT_SHAPE = (256, 320, 384)
NAN_SHAPE, NAN_ROW, NAN_COL = (256, 192, 128), 200, 100


def _bf16_exact(t):
    return torch.equal(t.float().bfloat16().float(), t.float())


def _relu_case(shape):
    """relu reference, bound and the mask of elements that are compared:
    those whose pre-activation is at least the bound away from 0."""
    _, _, _, ref, bound = fc.real_case(*shape)
    return torch.relu(ref), bound, ref.abs() >= bound


# -------------------------------------------------- operands, on any machine
@pytest.mark.parametrize("shape", fc.INT_SHAPES, ids=INT_IDS)
def test_integer_cases_are_exact_in_fp32(shape):
    M, K, N = shape
    A, W, b, prod = fc.int_case(*shape)
    assert _bf16_exact(A) and _bf16_exact(W)
    # every partial sum, in any order, is bounded by the sum of magnitudes
    assert (A.abs() @ W.abs().t() + b.abs()).max().item() < 2 ** 24
    ref = (prod + b).float()
    assert ref.abs().max().item() < 2 ** 24
    # the column pattern differs inside a tile and between tiles
    scale = fc.column_scale(K)
    assert scale.unique().numel() == K
    # a dropped, doubled or swapped K tile changes the result
    for t in range(K // fc.BK):
        cols = slice(t * fc.BK, (t + 1) * fc.BK)
        part = A[:, cols] @ W[:, cols].t()
        assert (part != 0).any()
        if t:
            prev = slice((t - 1) * fc.BK, t * fc.BK)
            assert not torch.equal(A[:, prev] @ W[:, cols].t(), part)
    # blocks along x (A rows) and y (W rows) are told apart
    for i in range(1, M // 128):
        assert not torch.equal(ref[:128], ref[i * 128:(i + 1) * 128])
    for j in range(1, N // 128):
        assert not torch.equal(ref[:, :128], ref[:, j * 128:(j + 1) * 128])
    # so are the 64x64 wave quadrants of the first block tile
    quads = [ref[r:r + 64, c:c + 64] for r in (0, 64) for c in (0, 64)]
    assert all(not torch.equal(quads[p], quads[q])
               for p in range(4) for q in range(p))
    # the fp32 CPU path is exact too
    assert torch.equal(F.linear(A.float(), W.float(), b.float()), ref)


def test_bf16_store_case_is_exact():
    A, W, b, prod = fc.int_case(*BF16_OUT_SHAPE, scaled=False)
    ref = prod + b
    assert ref.abs().max().item() <= 256 and _bf16_exact(ref)
    assert ref.abs().max().item() > 128            # 8 significand bits used


@pytest.mark.parametrize("shape", fc.REAL_SHAPES, ids=REAL_IDS)
def test_real_cases_and_eager_fp32(shape):
    A, W, b, ref, bound = fc.real_case(*shape)
    assert _bf16_exact(A) and _bf16_exact(W)
    out = F.linear(A, W, b)
    err = (out.double() - ref).abs()
    assert (err <= bound).all(), (err / bound).max().item()
    # relu: under 1 % of the output sits within the bound of 0
    _, _, keep = _relu_case(shape)
    assert (~keep).float().mean().item() < 0.01
    assert ((torch.relu(out).double() - torch.relu(ref)).abs() <= bound).all()
    # tanh: the measured allowance
    x32 = ref.float()
    terr = (torch.tanh(x32).double() - torch.tanh(x32.double())).abs().max()
    assert terr.item() <= TANH_TOL
    assert ((torch.tanh(out).double() - torch.tanh(ref)).abs()
            <= bound + TANH_TOL).all()
    print(f"\neager fp32 {shape}: gemm err/bound "
          f"{(err / bound).max().item():.3f}, tanh err {terr.item():.2e}")


def test_nan_case_reference():
    A, W, b, _, _ = fc.real_case(*NAN_SHAPE)
    A = A.clone()
    A[NAN_ROW, NAN_COL] = float("nan")
    ref = torch.relu(F.linear(A.double(), W.double(), b.double()))
    nan_rows = torch.isnan(ref).any(dim=1).nonzero().flatten().tolist()
    assert nan_rows == [NAN_ROW] and torch.isnan(ref[NAN_ROW]).all()
    assert NAN_ROW >= 128 and NAN_COL >= fc.BK     # second block, second tile


# ------------------------------------------------------------ GPU: integers
def _run(A, W, b, act, out_f32):
    from gcbf_amd import _C
    return _C.fused_linear(
        A.float().bfloat16().cuda(), W.float().bfloat16().cuda(),
        None if b is None else b.float().cuda(), act, out_f32)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", fc.INT_SHAPES, ids=INT_IDS)
def test_integer_gemm_exact(shape):
    A, W, b, prod = fc.int_case(*shape)
    out = _run(A, W, b, ACT_NONE, True)
    assert out.dtype == torch.float32 and out.shape == prod.shape
    want = (prod + b).float()
    wrong = (out.cpu() != want).nonzero()
    assert wrong.numel() == 0, \
        f"{wrong.shape[0]} wrong elements, first at {wrong[0].tolist()}"


@pytest.mark.gpu
def test_integer_gemm_exact_without_bias():
    A, W, _, prod = fc.int_case(256, 320, 384)
    out = _run(A, W, None, ACT_NONE, True)
    assert torch.equal(out.cpu(), prod.float())


@pytest.mark.gpu
def test_integer_gemm_exact_bf16_store():
    A, W, b, prod = fc.int_case(*BF16_OUT_SHAPE, scaled=False)
    out = _run(A, W, b, ACT_NONE, False)
    assert out.dtype == torch.bfloat16
    assert torch.equal(out.float().cpu(), (prod + b).float())
    # relu on exact integers is exact as well
    out = _run(A, W, b, ACT_RELU, False)
    assert torch.equal(out.float().cpu(), torch.relu(prod + b).float())


# --------------------------------------------------------- GPU: real values
def _assert_within(out, ref, bound, keep=None, what=""):
    err = (out.double().cpu() - ref).abs()
    ok = err <= bound
    if keep is not None:
        ok = ok | ~keep
    ratio = (err / bound)[keep].max() if keep is not None \
        else (err / bound).max()
    print(f"\n{what}: worst err/bound {ratio.item():.3f}, "
          f"max abs err {err.max().item():.2e}")
    assert ok.all(), f"{what}: {(~ok).sum().item()} elements over the bound"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", fc.REAL_SHAPES, ids=REAL_IDS)
def test_real_gemm_within_summation_bound(shape):
    A, W, b, ref, bound = fc.real_case(*shape)
    out = _run(A, W, b, ACT_NONE, True)
    _assert_within(out, ref, bound, what=f"linear {shape}")
    out = _run(A, W, b, ACT_NONE, False)
    _assert_within(out, ref, bound + BF16_EPS * ref.abs(),
                   what=f"linear bf16 {shape}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", fc.REAL_SHAPES, ids=REAL_IDS)
def test_relu_epilogue(shape):
    A, W, b, _, _ = fc.real_case(*shape)
    ref, bound, keep = _relu_case(shape)
    out = _run(A, W, b, ACT_RELU, True)
    assert (out >= 0).all()
    _assert_within(out, ref, bound, keep, what=f"relu {shape}")
    out = _run(A, W, b, ACT_RELU, False)
    _assert_within(out, ref, bound + BF16_EPS * ref.abs(), keep,
                   what=f"relu bf16 {shape}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", fc.REAL_SHAPES, ids=REAL_IDS)
def test_tanh_epilogue(shape):
    A, W, b, pre, bound = fc.real_case(*shape)
    ref = torch.tanh(pre)
    out = _run(A, W, b, ACT_TANH, True)
    _assert_within(out, ref, bound + TANH_TOL, what=f"tanh {shape}")
    out = _run(A, W, b, ACT_TANH, False)
    _assert_within(out, ref, bound + TANH_TOL + BF16_EPS * ref.abs(),
                   what=f"tanh bf16 {shape}")


@pytest.mark.gpu
def test_relu_epilogue_propagates_nan():
    """A NaN pre-activation stays NaN, as torch.relu on the library path;
    the other rows are untouched."""
    A, W, b, _, _ = fc.real_case(*NAN_SHAPE)
    clean = _run(A, W, b, ACT_RELU, True).cpu()
    A = A.clone()
    A[NAN_ROW, NAN_COL] = float("nan")
    ref = torch.relu(F.linear(A.double(), W.double(), b.double()))
    for out_f32 in (True, False):
        out = _run(A, W, b, ACT_RELU, out_f32).cpu()
        assert torch.equal(torch.isnan(out), torch.isnan(ref))
        assert torch.isnan(out[NAN_ROW]).all()
    out = _run(A, W, b, ACT_RELU, True).cpu()
    rows = torch.arange(NAN_SHAPE[0]) != NAN_ROW
    assert torch.equal(out[rows], clean[rows])


# ----------------------------------------------------- GPU: binding checks
@pytest.mark.gpu
def test_fused_linear_binding_rejects_bad_arguments():
    """Every call must raise from the binding's checks, before any launch."""
    from gcbf_amd import _C

    def z(*shape, dtype=torch.bfloat16):
        return torch.zeros(*shape, dtype=dtype, device="cuda")

    x, w, b = z(128, 64), z(128, 64), z(128, dtype=torch.float32)
    bad = {
        "bias too short": (x, w, z(64, dtype=torch.float32), 0, True),
        "bias too long": (x, w, z(256, dtype=torch.float32), 0, True),
        "bias bf16": (x, w, z(128), 0, True),
        "act 3": (x, w, b, 3, True),
        "act -1": (x, w, b, -1, True),
        "M = 0": (z(0, 64), w, b, 0, True),
        "N = 0": (x, z(0, 64), z(0, dtype=torch.float32), 0, True),
        "K = 0": (z(128, 0), z(128, 0), b, 0, True),
        "M % 128": (z(64, 64), w, b, 0, True),
        "N % 128": (x, z(64, 64), z(64, dtype=torch.float32), 0, True),
        "K % 64": (z(128, 32), z(128, 32), b, 0, True),
        "K mismatch": (x, z(128, 128), b, 0, True),
        "x fp32": (x.float(), w, b, 0, True),
        "w on CPU": (x, w.cpu(), b, 0, True),
    }
    for what, args in bad.items():
        with pytest.raises(RuntimeError):
            _C.fused_linear(*args)
            pytest.fail(f"fused_linear accepted: {what}")
    assert (_C.fused_linear(x, w, b, 0, True) == 0).all()
