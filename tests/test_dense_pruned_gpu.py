"""Dense plane from block maxima (MI355X only): the GEMM variant that
writes each row's block maxima beside the scores (`gemm.hip` BMAX
tiles), the pruned selector that reads them (`infomesh_topk_pruned` in
`topk.hip`), and `GpuShard.search_dense`, which pairs the two.

- GEMM: scores bit-equal to `gemm_nt(out_f32=True)`, maxima bit-equal to
  the block-wise maximum of those scores taken on the CPU.
- Selector: hand-built score matrices with CPU-derived maxima, so it is
  tested apart from the GEMM, under every rule of `_check_topk`
  (tests/test_select_plane_gpu.py).
- Plane: captured and uncaptured `search_dense` against the generic
  GEMM + streaming top-k; a masked batch keeps the old path.

Shapes are the smallest that reach each path: both widths (W = 64 on
the 128x128 tile, 32 on the 64x128 one), full and partial tiles, M off
the tile, NB below / above k, N < k, and gathered rows past the 4096
entries of the candidate buffer's tie region (32-bit refinement).
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from infomesh_amd.ops import _build
    _build.build()
from infomesh_amd.ops import kernels as K
from infomesh_amd.ops import reference as R
from test_select_plane_gpu import _check_topk

NEG_INF = float("-inf")


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.manual_seed(0)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------- GEMM

# (M, N) -> (W, tile of the plain gemm_nt at K % 64 == 0): the variant
# always runs a 128-column tile, the plain path steps down to the
# pipelined 64x64 tile on these small shapes at M > 64, so the first and
# third rows also show that the scores do not depend on the tile
GEMM_SHAPES = {
    (128, 128 * 3 + 40): (64, (64, 64, 64, True)),
    (64, 128 * 2 + 8): (32, (64, 128, 64, False)),
    (128, 128): (64, (64, 64, 64, True)),
    (100, 128 + 70): (64, (64, 64, 64, True)),   # M off the tile
    (40, 200): (32, (64, 128, 64, False)),
    (256, 128 * 2 + 1): (64, (64, 64, 64, True)),   # two m-tiles
}


@pytest.mark.parametrize("Kd", [64, 384])
@pytest.mark.parametrize("M,N", list(GEMM_SHAPES))
def test_gemm_bmax_scores_and_maxima(M, N, Kd):
    W, tile = GEMM_SHAPES[(M, N)]
    assert K.gemm_bmax_width(M, N, Kd) == W
    assert K.gemm_tile(M, N, Kd, 1) == tile
    g = torch.Generator().manual_seed(M * 1000 + N + Kd)
    a = torch.randn(M, Kd, generator=g).bfloat16().cuda()
    b = torch.randn(N, Kd, generator=g).bfloat16().cuda()
    a[1] = 0       # a row of +0.0 scores
    want = K.gemm_nt(a, b, out_f32=True)
    NB = (N + W - 1) // W
    # poisoned outputs: every element has to be written
    out = torch.full((M, N), float("nan"), device="cuda")
    bmax = torch.full((M, NB), float("nan"), device="cuda")
    got = K.gemm_nt_bmax(a, b, out=out, bmax=bmax)
    assert got is not None and got[2] == W
    assert got[0] is out and got[1] is bmax
    assert torch.equal(_bits(out), _bits(want)), "scores differ in bits"
    assert torch.equal(_bits(bmax), _bits(R.block_max(want.cpu(), W)))


def test_gemm_bmax_k32_tile_and_alpha():
    """K % 64 != 0 takes the BK = 32 instantiations; alpha is applied
    before the maximum. With BK = 32 a 128-column f32 tile does not fit
    the operand buffers, so full tiles must take the direct epilogue
    too (staging them used to drop rows: M = 48 runs the plain 64x128
    tile over two full tiles). The plain scores are checked against an
    f32 product: 96 exact bf16 products of magnitude below ~16 each,
    accumulated in f32, are within 96 * 16 * 2^-24 ~ 1e-4 of it."""
    for M, W in ((128, 64), (48, 32)):
        a = torch.randn(M, 96).bfloat16().cuda()
        b = torch.randn(300, 96).bfloat16().cuda()
        want = K.gemm_nt(a, b, out_f32=True, alpha=-0.5)
        ref = -0.5 * (a.cpu().double() @ b.cpu().double().T)
        assert float((want.cpu() - ref).abs().max()) < 1e-3
        out, bmax, w = K.gemm_nt_bmax(a, b, alpha=-0.5)
        assert w == W
        assert torch.equal(_bits(out), _bits(want))
        assert torch.equal(_bits(bmax), _bits(R.block_max(want.cpu(), W)))


def test_gemm_bmax_ineligible_shape_reports_so():
    """M <= 16 runs the GEMV route, which has no maxima: width 0, None,
    and nothing written."""
    a = torch.randn(16, 64).bfloat16().cuda()
    b = torch.randn(300, 64).bfloat16().cuda()
    assert K.gemm_bmax_width(16, 300, 64) == 0
    out = torch.full((16, 300), 7.0, device="cuda")
    assert K.gemm_nt_bmax(a, b, out=out) is None
    assert bool((out == 7.0).all())


# --------------------------------------------------------------- selector

def _cases(N: int, W: int, k: int):
    """name -> [3, N] f32 host scores."""
    g = torch.Generator().manual_seed(N * 7 + W + k)
    NB = (N + W - 1) // W
    out = {"random": torch.randn(3, N, generator=g),
           "constant": torch.full((3, N), 0.5)}
    # more than k blocks share the threshold maximum (as many as the row
    # has when NB <= k), a few larger values above it
    s = torch.rand(3, N, generator=g)
    nb = min(NB, k + 20)
    blocks = torch.randperm(NB, generator=g)[:nb]
    s[:, (blocks * W + blocks % W).clamp(max=N - 1)] = 2.0
    s[0, N // 2] = 3.0
    s[1, [0, N - 1]] = torch.tensor([4.0, 3.5])
    out["threshold blocks"] = s
    # eight distinct values, so duplicates everywhere; the largest on
    # both sides of block boundaries
    s = torch.randint(0, 8, (3, N), generator=g).float()
    edge = torch.tensor([W - 1, W, 2 * W - 1, 2 * W, 4 * W - 1, 4 * W])
    s[:, edge] = 9.0
    out["duplicates"] = s
    s = torch.where(torch.rand(3, N, generator=g) < 0.5,
                    torch.tensor(0.0), torch.tensor(-0.0))
    s[0, ::5] = -1.0
    s[1] = -0.0
    out["signed zeros"] = s
    s = torch.full((3, N), NEG_INF)
    s[0, [3, N // 3, N - 2]] = torch.tensor([1.0, -2.0, 0.5])
    s[1, W:W + 6] = 1.0
    out["-inf heavy"] = s
    # row 0 in [1, 1 + 2^-7): one 16-bit prefix for the whole row, so the
    # gathered blocks overflow the tie region wherever min(k, NB) * W
    # > 4096 and the threshold needs all 32 bits
    s = torch.randn(3, N, generator=g)
    s[0] = 1.0 + torch.rand(N, generator=g) * 2.0 ** -7
    out["near-tied row"] = s
    return out


@pytest.mark.parametrize("k", [1, 100, 1024])
@pytest.mark.parametrize("W,mult", [(32, 5), (32, 300), (32, 0),
                                    (64, 5), (64, 300), (64, 0)])
def test_topk_pruned(W, mult, k):
    N = W * mult + (7 if mult == 300 else 0) if mult else 20_000
    tk = K.TopKPruned("cuda")
    for name, host in _cases(N, W, k).items():
        bmax = R.block_max(host, W)
        vals, idx = tk(host.cuda(), bmax.cuda(), W, k)
        _check_topk(host, k, vals, idx, what=f"{name} N={N} W={W} k={k}")


def test_topk_pruned_matches_streaming_selector():
    """Same values as TopK, same indices on rows without a tie at rank
    k (random f32 rows have none)."""
    host = torch.randn(3, 20_000)
    dev = host.cuda()
    v0, i0 = K.topk(dev, 100)
    v1, i1 = K.TopKPruned("cuda")(dev, R.block_max(host, 64).cuda(), 64, 100)
    assert torch.equal(v0, v1) and torch.equal(i0, i1)


# ------------------------------------------------------------------ plane

N_DOCS, DIM, QB = 3000, 64, 24     # 17 <= QB <= 64: the 64x128 tile


@pytest.fixture(scope="module")
def shard():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infomesh_amd.index.gpu_index import GpuShard
    rng = np.random.default_rng(5)
    lens = rng.integers(3, 9, size=N_DOCS)
    emb = torch.nn.functional.normalize(
        torch.randn(N_DOCS, DIM, generator=torch.Generator().manual_seed(5)),
        dim=-1).bfloat16()
    s = GpuShard("cuda")
    s.build_from_arrays(
        rng.integers(0, 500, size=int(lens.sum())),
        np.repeat(np.arange(N_DOCS), lens), lens,
        np.arange(N_DOCS) + 100, emb)
    return s


def _queries(seed: int, B: int = QB) -> torch.Tensor:
    return torch.nn.functional.normalize(
        torch.randn(B, DIM, generator=torch.Generator().manual_seed(seed)),
        dim=-1).bfloat16().cuda()


def _generic(shard, q: torch.Tensor, k: int):
    scores = K.gemm_nt(q, shard.embeddings, out_f32=True)
    return scores, K.topk(scores, k)


@pytest.mark.parametrize("k", [10, 100])
def test_search_dense_uncaptured_takes_the_pruned_pair(shard, k):
    shard.graph_dense = False
    shard._dense_bmax.clear()
    q = _queries(1)
    vals, idx = shard.search_dense(q, k)
    assert QB in shard._dense_bmax, "block maxima were not produced"
    assert shard._dense_bmax[QB].shape == (QB, (N_DOCS + 31) // 32)
    scores, (gv, gi) = _generic(shard, q, k)
    assert torch.equal(vals, gv)
    _check_topk(scores.cpu(), k, vals, idx, what="uncaptured")


def test_search_dense_graph_replays_with_new_queries(shard):
    k = 50
    shard.graph_dense = True
    try:
        shard._dense_graphs.clear()
        for seed in (2, 3, 2):
            q = _queries(seed)
            vals, idx = shard.search_dense(q, k)
            scores, (gv, gi) = _generic(shard, q, k)
            assert torch.equal(vals, gv), f"seed {seed}"
            _check_topk(scores.cpu(), k, vals, idx, what=f"graph seed {seed}")
        g = shard._dense_graphs[(QB, k)]
        assert not g._failed and len(g._cache) == 1, "plane was not captured"
    finally:
        shard.graph_dense = False


def test_masked_batch_keeps_the_streaming_path(shard):
    """Runs last on the shared shard: it tombstones documents. The mask
    is then active, the maxima would count dead documents, and the
    plane must not use them."""
    k, B = 20, 20
    q = _queries(4, B)
    scores = K.gemm_nt(q, shard.embeddings, out_f32=True).cpu()
    best = scores.argmax(dim=1).unique()          # local rows
    assert shard.delete((best + 100).tolist()) == best.numel()
    shard._dense_bmax.clear()
    vals, idx = shard.search_dense(q, k)
    assert not shard._dense_bmax, "masked batch produced block maxima"
    dead = torch.zeros(N_DOCS, dtype=torch.bool)
    dead[best] = True
    want, _ = torch.topk(scores.masked_fill(dead, NEG_INF), k, dim=1)
    assert torch.equal(vals.cpu(), want)
    assert not bool(dead[idx.cpu().long()].any())
