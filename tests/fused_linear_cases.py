"""Hand-built operands for tests/test_fused_linear_branches.py (plain torch
on CPU).

Integer cases: every operand is an integer that bf16 holds exactly and every
product and partial sum stays below 2^24, so fp32 accumulation is exact in
any order and the kernel's output can be compared position by position.
Real cases: operands rounded to bf16 first, reference in fp64.
"""
import functools

import torch

BK = 64              # the kernel's K tile

# (M, K, N): one tile / both LDS buffers / odd tile count (buffer 0 reused) /
# two blocks along x / two blocks along y / everything at once
INT_SHAPES = [(128, 64, 128), (128, 128, 128), (128, 192, 128),
              (256, 64, 128), (128, 64, 256), (256, 320, 384)]
REAL_SHAPES = [(128, 192, 128), (256, 2048, 128)]


def column_scale(K):
    """Per-column factor (1 + 2 (k mod 64)) * 2^(k div 64): an odd number
    <= 127 times a power of two, so no two columns share it, and integers
    in [-2, 2] scaled by it (at most 8 significant bits) stay exact in
    bf16."""
    k = torch.arange(K)
    return (1 + 2 * (k % BK)) * 2 ** (k // BK)


@functools.lru_cache(maxsize=None)
def int_case(M, K, N, scaled=True):
    """A (M, K), W (N, K), bias (N,) as int64, and the exact result."""
    g = torch.Generator().manual_seed(M * 7 + K * 3 + N)
    A = torch.randint(-2, 3, (M, K), generator=g)
    W = torch.randint(-2, 3, (N, K), generator=g)
    b = torch.randint(-8, 9, (N,), generator=g)
    if scaled:
        A = A * column_scale(K)
    return A, W, b, A @ W.t()


@functools.lru_cache(maxsize=None)
def real_case(M, K, N):
    """bf16-rounded A, W (as fp32), fp32 bias, fp64 pre-activation and its
    per-element error bound (K + 2) * 2^-24 * (|A| |W|^T + |b|): the
    standard summation bound, valid for any accumulation order."""
    g = torch.Generator().manual_seed(M + K + N)
    A = torch.randn(M, K, generator=g).bfloat16().float()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16().float()
    b = torch.randn(N, generator=g)
    Ad, Wd, bd = A.double(), W.double(), b.double()
    ref = Ad @ Wd.t() + bd
    bound = (K + 2) * 2.0 ** -24 * (Ad.abs() @ Wd.abs().t() + bd.abs())
    return A, W, b, ref, bound
