"""The pruning lemma behind the dense plane's pruned top-k, pinned on
the CPU oracles alone (ops/reference.py block_max + topk_pruned), no
kernel involved: the top k of the k blocks with the largest maxima IS
the top k of the row — values under ==, indices wherever the row has no
tie at rank k."""
from __future__ import annotations

import pytest
import torch

from infomesh_amd.ops import reference as R

NEG_INF = float("-inf")


def _check(s: torch.Tensor, W: int, k: int, what: str = ""):
    B, N = s.shape
    vals, idx = R.topk_pruned(s, R.block_max(s, W), W, k)
    assert vals.shape == (B, k) and idx.shape == (B, k)
    n = min(k, N)
    rv, _ = torch.topk(s, n, dim=1)
    assert bool((vals[:, :n] == rv).all()), f"{what}: values"
    assert bool((vals[:, n:] == NEG_INF).all()) \
        and bool((idx[:, n:] == -1).all()), f"{what}: padding"
    sv, si = torch.sort(s, dim=1, descending=True, stable=True)
    for b in range(B):
        i = idx[b, :n]
        assert bool(((i >= 0) & (i < N)).all()), f"{what}: range"
        assert i.unique().numel() == n, f"{what}: duplicates"
        assert bool((s[b, i] == vals[b, :n]).all()), f"{what}: s[idx]"
        tied = vals[b, 1:n] == vals[b, :n - 1]
        assert bool((i[1:] > i[:-1])[tied].all()), f"{what}: tie order"
        if n == N or sv[b, n - 1] != sv[b, n]:
            assert torch.equal(i, si[b, :n]), f"{what}: indices"


@pytest.mark.parametrize("W", [32, 64])
@pytest.mark.parametrize("N", [64 * 5, 64 * 40 + 7, 3001])
@pytest.mark.parametrize("k", [1, 10, 100])
def test_random_rows(W, N, k):
    g = torch.Generator().manual_seed(N * 131 + k)
    _check(torch.randn(3, N, generator=g), W, k, f"W={W} N={N} k={k}")


def test_block_max_is_the_blockwise_max():
    g = torch.Generator().manual_seed(1)
    s = torch.randn(2, 64 * 3 + 9, generator=g)
    bm = R.block_max(s, 64)
    assert bm.shape == (2, 4)
    for j in range(4):
        assert torch.equal(bm[:, j], s[:, j * 64:(j + 1) * 64].max(1).values)
    # ordered-key order: +0.0 beats -0.0, bit for bit
    z = torch.tensor([[-0.0, 0.0, -0.0, -0.0], [-0.0, -0.0, -0.0, -0.0]])
    bz = R.block_max(z, 4)
    assert bz.view(torch.int32).tolist() == [[0], [-(1 << 31)]]


@pytest.mark.parametrize("k", [1, 7, 100])
def test_all_equal_rows(k):
    _check(torch.full((2, 64 * 9 + 3), 0.25), 64, k, f"const k={k}")


def test_more_than_k_blocks_at_the_threshold():
    # 30 blocks share the maximum 2.0 and k = 8: whichever 8 blocks are
    # kept, the values are right; a few larger values decide the rest
    W, NB, k = 32, 40, 8
    g = torch.Generator().manual_seed(2)
    s = torch.rand(2, NB * W, generator=g)
    s[:, (torch.arange(30) * W + torch.arange(30) % W)] = 2.0
    s[0, 5] = 3.0
    s[1, [7, 700]] = torch.tensor([4.0, 3.5])
    _check(s, W, k, "threshold ties")


@pytest.mark.parametrize("N,W,k", [
    (64 * 3 + 1, 64, 5),     # N % W != 0, last block one column wide
    (200, 64, 4),            # k == NB
    (200, 64, 50),           # k > NB: every block chosen
    (640, 64, 10),           # k * W == N
    (500, 64, 8),            # k * W > N
    (40, 64, 100),           # N < k: padding
    (70, 32, 1024),
])
def test_shape_edges(N, W, k):
    g = torch.Generator().manual_seed(N + k)
    _check(torch.randn(3, N, generator=g), W, k, f"N={N} W={W} k={k}")


def test_signed_zeros_and_neg_inf():
    g = torch.Generator().manual_seed(3)
    N, W = 64 * 6 + 5, 64
    z = torch.where(torch.rand(2, N, generator=g) < 0.5,
                    torch.tensor(0.0), torch.tensor(-0.0))
    z[0, ::7] = -1.0
    for k in (1, 10, 200):
        _check(z, W, k, f"zeros k={k}")
    s = torch.full((2, N), NEG_INF)
    s[0, [3, 100, 388]] = torch.tensor([1.0, -2.0, 0.5])
    s[1, 64:70] = 1.0
    for k in (1, 3, 50, 1024):
        _check(s, W, k, f"-inf heavy k={k}")
