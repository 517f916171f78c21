"""The one-kernel pruned selector (`row_select_kernel` behind
`infomesh_topk_pruned`, topk.hip), the BM25 block kernel's block-maxima
writeout (bm25.hip) and the BM25 plane that pairs the two (MI355X only).

The selector's contract is strict: for a row without NaN, `idx` is the
first k columns of a stable descending sort of the row with -0.0 counted
equal to +0.0, and `vals` the values there (zeros as +0.0), also where
several equal values meet at rank k. There is no tolerance anywhere in
this file: every comparison is on bits or on integers.

Shapes are the smallest that reach each path: both block widths, N below
k, N off the block, NB below / above k, a maxima row past the 24 576
keys the kernel stages in LDS (48 001 blocks, which takes the grouped
level), and chosen blocks past it
(k = 1024 at W = 64: 65 536 scores), with a staged and with an unstaged
maxima row.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from infomesh_amd.ops import _build
    _build.build()
from infomesh_amd.ops import kernels as K
from infomesh_amd.ops import reference as R
from test_dense_pruned_gpu import _cases
from test_select_plane_gpu import _check_topk

NEG_INF = float("-inf")


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.manual_seed(0)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.cpu().contiguous().view(torch.int32)


def _canon(host: torch.Tensor) -> torch.Tensor:
    """-0.0 -> +0.0, everything else untouched."""
    return torch.where(host == 0, torch.zeros_like(host), host)


def _stable_sort(host: torch.Tensor):
    return torch.sort(_canon(host), dim=1, descending=True, stable=True)


def _check_strict(host: torch.Tensor, k: int, vals: torch.Tensor,
                  idx: torch.Tensor, what: str = "", oracle=None):
    """The strict contract, against a stable sort of the CPU copy
    (oracle: that sort, where several checks share one matrix)."""
    B, N = host.shape
    vals, idx = vals.cpu(), idx.cpu().long()
    assert vals.shape == (B, k) and idx.shape == (B, k), what
    n = min(k, N)
    sv, si = oracle if oracle is not None else _stable_sort(host)
    assert torch.equal(idx[:, :n], si[:, :n]), \
        f"{what}: {int((idx[:, :n] != si[:, :n]).sum())} indices differ " \
        f"from the stable sort"
    assert torch.equal(_bits(vals[:, :n]), _bits(sv[:, :n])), \
        f"{what}: values"
    assert bool((vals[:, n:] == NEG_INF).all()) \
        and bool((idx[:, n:] == -1).all()), f"{what}: padding"


def _select(host: torch.Tensor, W: int, k: int):
    return K.TopKPruned("cuda")(host.cuda(), R.block_max(host, W).cuda(),
                                W, k)


# --------------------------------------------------------------- selector

def _N(W: int, mult: int) -> int:
    return W * mult + (7 if mult == 300 else 0) if mult else 20_000


@pytest.mark.parametrize("k", [1, 100, 1024])
@pytest.mark.parametrize("W,mult", [(32, 5), (32, 300), (32, 0),
                                    (64, 5), (64, 300), (64, 0)])
def test_strict_order(W, mult, k):
    """Every matrix of `_cases`; N = 5 W is below k = 1024 (and NB = 5
    below every k but 1). Both levels fit the LDS stage at every shape
    here (at most 625 maxima and 20 032 scores)."""
    N = _N(W, mult)
    for name, host in _cases(N, W, k).items():
        vals, idx = _select(host, W, k)
        what = f"{name} N={N} W={W} k={k}"
        _check_strict(host, k, vals, idx, what)
        _check_topk(host, k, vals, idx, what=what)


@functools.lru_cache(maxsize=None)
def _big():
    """3 x (64 * 48 001) scores, their maxima on the device and their
    stable sort: a random row, a row of 7 distinct values (ties
    everywhere, at the group, the block and the score level), a constant
    row."""
    W, NB = 64, 48_001
    g = torch.Generator().manual_seed(11)
    host = torch.randn(3, W * NB, generator=g)
    host[1] = torch.randint(0, 7, (W * NB,), generator=g).float()
    host[2] = 0.25
    return host, host.cuda(), R.block_max(host, W).cuda(), _stable_sort(host)


@pytest.mark.parametrize("k", [100, 1024])
def test_maxima_row_past_the_lds_stage(k):
    """48 001 blocks per row do not fit the stage: the maxima are
    grouped in pairs first (24 001 groups, the last of one block), the
    kernel chooses groups, then blocks among their children. At k = 1024
    the 65 536 scores of the chosen blocks are read from global memory
    as well."""
    host, dev, bmax, oracle = _big()
    vals, idx = K.TopKPruned("cuda")(dev, bmax, 64, k)
    _check_strict(host, k, vals, idx, f"48001 blocks k={k}", oracle)


def test_staged_maxima_with_scores_past_the_lds_stage():
    """NB = 2000 maxima fit the stage, the 1024 * 64 = 65 536 scores of
    the chosen blocks do not: the second level alone reads global
    memory. N ends inside the last block."""
    W, N, k = 64, 64 * 2000 - 9, 1024
    cases = _cases(N, W, k)
    for name in ("random", "duplicates", "threshold blocks"):
        vals, idx = _select(cases[name], W, k)
        _check_strict(cases[name], k, vals, idx, f"{name} N={N}")


def test_tie_blocks_lowest_ids_win():
    """More blocks share the threshold maximum t than there are slots
    left, and a block with a maximum above t and a HIGHER id also holds
    a score equal to t: the k = 100 results are the 30 scores above t and
    the 70 lowest columns among the 121 equal to t, none from the blocks
    left out and not the one in the last block."""
    W, NB, k, t = 64, 300, 100, 2.0
    g = torch.Generator().manual_seed(3)
    host = torch.rand(1, W * NB, generator=g)          # all below t
    blocks = torch.randperm(NB - 1, generator=g)       # block NB-1 is set below
    above, tie = blocks[:29], blocks[29:29 + 120]
    host[0, above * W + above % W] = 3.0 + torch.rand(29, generator=g)
    host[0, tie * W + (tie * 7) % W] = t
    host[0, (NB - 1) * W + 5] = 5.0                    # maximum above t ...
    host[0, (NB - 1) * W + 9] = t                      # ... and a score == t
    bm = R.block_max(host, W)[0]
    K1 = min(k, NB)
    kth = torch.sort(bm, descending=True).values[K1 - 1]
    n_above = int((bm > kth).sum())
    assert float(kth) == t and n_above == 30
    assert int((bm == kth).sum()) > K1 - n_above, "precondition: tie blocks"
    assert int((host[0] == t).sum()) == 121
    vals, idx = _select(host, W, k)
    _check_strict(host, k, vals, idx, "tie blocks")
    assert (NB - 1) * W + 9 not in idx.cpu().tolist()[0]


def test_near_tied_row_shares_one_16_bit_prefix():
    """Values in [1, 1 + 2^-7): the 6400 scores of the 100 chosen blocks
    share one 16-bit prefix (more than the 4096 a two-byte select could
    leave to a sort), so the threshold needs all 32 bits."""
    W, N, k = 64, 20_000, 100
    g = torch.Generator().manual_seed(5)
    host = 1.0 + torch.rand(3, N, generator=g) * 2.0 ** -7
    host[2, ::3] = host[2, 1]                           # and exact ties
    prefix = _bits(host) >> 16
    assert bool((prefix == prefix[0, 0]).all())
    assert min(k, (N + W - 1) // W) * W > 4096, "precondition: gathered"
    vals, idx = _select(host, W, k)
    _check_strict(host, k, vals, idx, "near-tied")


@pytest.mark.parametrize("W,k", [(64, 100), (32, 1024)])
def test_two_calls_agree(W, k):
    N = 300 * W + 7
    tk = K.TopKPruned("cuda")
    for name in ("constant", "duplicates", "random"):
        host = _cases(N, W, k)[name]
        dev, bmax = host.cuda(), R.block_max(host, W).cuda()
        v0, i0 = tk(dev, bmax, W, k)
        v1, i1 = tk(dev, bmax, W, k)
        assert torch.equal(_bits(v0), _bits(v1)) and torch.equal(i0, i1), name


# ------------------------------------------------------------ BM25 maxima

def _bm25_segments(segs, queries, n_terms: int, bd: int, with_bmax: bool,
                   seed: int):
    """Score `queries` (lists of term ids; terms >= n_terms have no
    postings) over `segs` [(doc_base, nseg), ...] with K.bm25_block into
    NaN-filled scores (and maxima). Returns (scores, bmax or None)."""
    dev = "cuda"
    N = sum(n for _, n in segs)
    rng = np.random.default_rng(seed)
    doc_lens = rng.integers(5, 200, size=N)
    postings = {t: sorted(rng.choice(N, size=int(rng.integers(1, N // 3)),
                                     replace=False).tolist())
                for t in range(n_terms)}
    tf = {t: rng.integers(1, 6, size=len(p)) for t, p in postings.items()}
    B = len(queries)
    tlist = [t for q in queries for t in sorted(set(q))]
    qt_off = np.cumsum([0] + [len(set(q)) for q in queries]).astype(np.int32)
    uterms, qt_ut = np.unique(np.array(tlist, dtype=np.int64),
                              return_inverse=True)
    df = [len(postings.get(t, ())) for t in tlist]
    idf = [math.log(1.0 + (N - d + 0.5) / (d + 0.5)) for d in df]
    scores = torch.full((B, N), float("nan"), device=dev)
    bmax = torch.full((B, (N + 63) // 64), float("nan"), device=dev) \
        if with_bmax else None
    for base, nseg in segs:
        doc_ids, packed, begin, end = [], [], [], []
        for t in uterms:
            begin.append(len(doc_ids))
            for d, f in zip(postings.get(int(t), ()), tf.get(int(t), ())):
                if base <= d < base + nseg:
                    doc_ids.append(d - base)
                    packed.append(int(f) | (int(doc_lens[d]) << 16))
            end.append(len(doc_ids))
        nblocks = (nseg + bd - 1) // bd
        bounds = torch.empty(max(1, len(uterms) * nblocks * 2),
                             dtype=torch.int32, device=dev)
        K.bm25_block(
            torch.from_numpy(np.array(doc_ids, dtype=np.int32)).to(dev),
            torch.from_numpy(np.array(packed, dtype=np.int32)).to(dev),
            torch.from_numpy(qt_off).to(dev),
            torch.from_numpy(qt_ut.astype(np.int32)).to(dev),
            torch.tensor(idf, dtype=torch.float32, device=dev),
            torch.from_numpy(np.array(begin, dtype=np.int64)).to(dev),
            torch.from_numpy(np.array(end, dtype=np.int64)).to(dev),
            bounds, scores, doc_base=base, nseg=nseg, bd=bd,
            avgdl=float(doc_lens.mean()), bmax=bmax)
    return scores, bmax


# B = 3: terms with postings, terms without any (an all-zero row), no terms
_BM_QUERIES = [[0, 3, 5, 7], [40, 41], []]


@pytest.mark.parametrize("segs", [
    [(0, 8192 + 4096 + 37)],      # full tiles, a partial tile and block
    [(0, 128), (128, 172)],       # a second segment at an aligned base
], ids=["one segment", "two aligned segments"])
def test_bm25_block_maxima(segs):
    plain, _ = _bm25_segments(segs, _BM_QUERIES, 8, 4096, False, seed=2)
    scores, bmax = _bm25_segments(segs, _BM_QUERIES, 8, 4096, True, seed=2)
    assert not bool(torch.isnan(scores).any()), "columns left unwritten"
    assert torch.equal(_bits(scores), _bits(plain)), "scores differ in bits"
    assert torch.equal(_bits(bmax), _bits(R.block_max(scores.cpu(), 64)))
    assert bool((scores[0] > 0).any())
    assert bool((scores[1:] == 0).all()) and bool((bmax[1:] == 0).all())
    vals, idx = K.TopKPruned("cuda")(scores, bmax, 64, 100)
    _check_strict(scores.cpu(), 100, vals, idx, "bm25 maxima")


def test_bm25_block_maxima_refuse_an_unaligned_base():
    with pytest.raises(AssertionError):
        _bm25_segments([(0, 45), (45, 65)], _BM_QUERIES, 8, 4096, True,
                       seed=2)


# ------------------------------------------------------------------ plane

def _shard_docs(n_docs: int, vocab: int, seed: int):
    rng = np.random.default_rng(seed)
    lens = rng.integers(3, 9, size=n_docs)
    return [rng.integers(0, vocab, size=int(n)) for n in lens]


def _shard(segments, vocab: int, seed: int):
    """GpuShard with one segment per (lo, hi) document range."""
    from infomesh_amd.index.gpu_index import GpuShard
    docs = _shard_docs(segments[-1][1], vocab, seed)
    s = GpuShard("cuda")
    for lo, hi in segments:
        for i in range(lo, hi):
            s.add_document(1000 + i, docs[i], None)
        s.build()
    assert [(g.doc_base, g.doc_base + g.n_docs) for g in s.segments] \
        == list(segments)
    return s


class _SpyTopK:
    def __init__(self, real):
        self.real, self.calls = real, []

    def __call__(self, scores, k, ext_hist1=None, mask=None, row_pred=None):
        self.calls.append({"ext_hist1": ext_hist1 is not None,
                           "masked": mask is not None})
        return self.real(scores, k, ext_hist1=ext_hist1, mask=mask,
                         row_pred=row_pred)


def _queries(vocab: int, seed: int, B: int = 6):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, vocab, size=int(rng.integers(1, 4)))
            for _ in range(B)]


def _search_strict(shard, terms, k: int, what: str):
    """search_bm25 against the strict oracle over the score matrix the
    plane wrote."""
    vals, idx = shard.search_bm25(terms, k)
    torch.cuda.synchronize()
    _check_strict(shard._bm25_scores_buf.cpu(), k, vals, idx, what)
    return vals, idx


@pytest.mark.parametrize("vocab", [8, 500])
def test_plane_single_segment_takes_the_pruned_pair(vocab):
    """vocab 8: exact ties everywhere; 500: rows with fewer than k
    positive scores (the rest are +0.0, lowest columns first)."""
    n_docs, k = 3000 + 37, 100
    s = _shard([(0, n_docs)], vocab, seed=vocab)
    s._topk = spy = _SpyTopK(s._get_topk())
    terms = _queries(vocab, seed=1)
    _search_strict(s, terms, k, f"vocab {vocab}")
    assert spy.calls == [], "the streaming selector ran"
    bmax = s._bm25_bmax[len(terms)]
    assert bmax.shape == (len(terms), (n_docs + 63) // 64)
    assert torch.equal(_bits(bmax),
                       _bits(R.block_max(s._bm25_scores_buf.cpu(), 64)))
    if vocab == 500:
        assert int((s._bm25_scores_buf > 0).sum(1).min()) < k


def test_plane_aligned_segments_take_the_pruned_pair():
    s = _shard([(0, 128), (128, 300)], 30, seed=7)
    s._topk = spy = _SpyTopK(s._get_topk())
    terms = _queries(30, seed=2)
    _search_strict(s, terms, 50, "segments 128 + 172")
    assert spy.calls == [] and len(terms) in s._bm25_bmax


def test_plane_unaligned_segments_keep_the_histogram():
    s = _shard([(0, 45), (45, 110)], 30, seed=8)
    s._topk = spy = _SpyTopK(s._get_topk())
    terms = _queries(30, seed=3)
    vals, idx = s.search_bm25(terms, 50)
    torch.cuda.synchronize()
    assert spy.calls == [{"ext_hist1": True, "masked": False}]
    assert not s._bm25_bmax, "an unaligned shard produced block maxima"
    # 110 columns: every tie fits the streaming selector's candidate
    # buffer, so its sort also settles rank k by column
    _check_strict(s._bm25_scores_buf.cpu(), 50, vals, idx,
                  "segments 45 + 65")


def test_plane_tombstoned_shard_keeps_the_masked_select():
    n_docs, k = 2000, 40
    s = _shard([(0, n_docs)], 500, seed=9)
    terms = _queries(500, seed=4)
    _, idx = s.search_bm25(terms, k)
    dead = idx[:, 0].unique().cpu()
    assert s.delete((dead + 1000).tolist()) == dead.numel()
    s._bm25_bmax.clear()
    s._topk = spy = _SpyTopK(s._get_topk())
    vals, idx = s.search_bm25(terms, k)
    torch.cuda.synchronize()
    assert spy.calls == [{"ext_hist1": False, "masked": True}]
    assert not s._bm25_bmax, "a masked batch produced block maxima"
    gone = torch.zeros(n_docs, dtype=torch.bool)
    gone[dead.long()] = True
    host = s._bm25_scores_buf.cpu()
    want, _ = torch.topk(host.masked_fill(gone, NEG_INF), k, dim=1)
    assert torch.equal(vals.cpu(), want)
    assert not bool(gone[idx.cpu().long()].any())
