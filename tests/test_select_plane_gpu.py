"""Selection plane against exact CPU oracles (MI355X only): `topk.hip`
(unmasked, producer histogram, masked) and the BM25 producer that feeds
it (`bm25.hip`, both instantiations of the block kernel).

Every top-k result goes through one checker, `_check_topk`:

- values equal `torch.topk` of the CPU copy under `==` (so +0.0 and
  -0.0 are one value, and there is no tolerance);
- indices are in range, distinct per row, pass the mask, and
  `scores[b, idx] == vals`;
- padding is exactly -inf / -1 and sits only past the number of
  available (passing) columns;
- inside the returned list equal values come in ascending index order
  (the sort key's "ties -> smaller idx first");
- where the row has no tie at rank k the indices equal the oracle's
  (value descending, index ascending among equals).

Which of several exactly equal values at rank k are returned is
arbitrary by design, so indices are not compared there. NaN scores are
outside the selector's contract and are not tested.

Shapes are the smallest that reach each path: one `hist1` grid chunk is
16 384 columns, the tie region of the candidate buffer holds 4096
entries, and B = 3 makes rows 1 and 2 start off a 16-byte boundary
whenever N % 4 != 0.
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

NEG_INF = float("-inf")


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.manual_seed(0)


# ---------------------------------------------------------------- checker

def _pass_matrix(bits: torch.Tensor, row_pred: torch.Tensor,
                 N: int) -> torch.Tensor:
    """[B, N] bool: column passes the mask row of its batch row."""
    words = bits.cpu().numpy().view(np.uint32)
    ok = np.unpackbits(words.view(np.uint8), axis=1,
                       bitorder="little")[:, :N].astype(bool)
    return torch.from_numpy(ok[row_pred.cpu().numpy().astype(np.int64)])


def _check_topk(host: torch.Tensor, k: int, vals: torch.Tensor,
                idx: torch.Tensor, bits: torch.Tensor | None = None,
                row_pred: torch.Tensor | None = None, what: str = ""):
    """host: the [B, N] f32 scores on the CPU; vals/idx: the selector's
    output; bits/row_pred: the mask of a masked call."""
    B, N = host.shape
    vals, idx = vals.cpu(), idx.cpu().long()
    assert vals.shape == (B, k) and idx.shape == (B, k), what
    assert vals.dtype == torch.float32
    kk = min(k, N)
    if bits is None:
        ok = torch.ones(B, N, dtype=torch.bool)
        s = host
        rv, _ = torch.topk(host, kk, dim=1)
    else:
        ok = _pass_matrix(bits, row_pred, N)
        s = host.masked_fill(~ok, NEG_INF)
        rv, _ = R.masked_topk(host, kk, bits, row_pred)
    # oracle order: value descending, index ascending among equals
    sv, si = torch.sort(s, dim=1, descending=True, stable=True)
    for b in range(B):
        w = f"{what} row {b}"
        n = min(k, int(ok[b].sum()))
        v, i = vals[b, :n], idx[b, :n]
        assert bool((v == rv[b, :n]).all()), \
            f"{w}: {int((v != rv[b, :n]).sum())} of {n} values differ " \
            f"from torch.topk"
        assert bool((vals[b, n:] == NEG_INF).all()) \
            and bool((idx[b, n:] == -1).all()), f"{w}: padding"
        assert bool(((i >= 0) & (i < N)).all()), f"{w}: index out of range"
        assert i.unique().numel() == n, f"{w}: duplicate indices"
        assert bool(ok[b, i].all()), f"{w}: masked-out column returned"
        assert bool((host[b, i] == v).all()), f"{w}: scores[idx] != vals"
        tied = v[1:] == v[:-1]
        assert bool((i[1:] > i[:-1])[tied].all()), \
            f"{w}: equal values out of index order"
        if n and (n == N or sv[b, n - 1] != sv[b, n]):
            assert torch.equal(i, si[b, :n]), f"{w}: indices"


def _ordered_top_hist(host: torch.Tensor) -> torch.Tensor:
    """[B, 256] counts of the ordered-float top byte, the mapping of
    float_to_ordered (common.h): negative -> ~bits, else bits | sign."""
    bits = host.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    ordered = torch.where(bits >= 0x80000000, bits ^ 0xFFFFFFFF,
                          bits | 0x80000000)
    return torch.stack([torch.bincount(r, minlength=256)
                        for r in ordered >> 24])


def _random_mask(P: int, N: int, frac: float,
                 g: torch.Generator) -> torch.Tensor:
    """[P, W] i32 pass bitmask in filter_bitmask's layout: W =
    ceil(N/64)*2, bit d&31 of word d>>5 is document d, bits >= N are 0."""
    W = (N + 63) // 64 * 2
    ok = np.zeros((P, W * 32), dtype=np.uint8)
    ok[:, :N] = (torch.rand(P, N, generator=g) < frac).numpy()
    words = np.packbits(ok, axis=1, bitorder="little").view(np.uint32)
    return torch.from_numpy(words.view(np.int32).copy())


def _run(host: torch.Tensor, k: int, what: str = "", sel=None):
    sel = sel or K.TopK()
    vals, idx = sel(host.cuda(), k)
    _check_topk(host, k, vals, idx, what=what)


# ------------------------------------------------------------ shape edges

_SHAPE_N = [1, 3, 4, 5, 63, 257, 1024, 1025, 4099, 16_384, 16_385]


@pytest.mark.parametrize("N,k", [(N, k) for N in _SHAPE_N
                                 for k in sorted({1, min(N, 100), 1024})])
def test_topk_shape_edges(N, k):
    """B = 3, unmasked: N below one float4, N % 4 != 0 (unaligned rows
    1 and 2, scalar tails), the 16 384-column chunk edge, k > N (padded
    tail) and k = N = 1024 (everything selected)."""
    g = torch.Generator().manual_seed(N * 1031 + k)
    host = torch.randn(3, N, generator=g)
    _run(host, k, what=f"N={N} k={k}")


# ------------------------------------------------------------ value edges

def _value_rows(name: str) -> torch.Tensor:
    g = torch.Generator().manual_seed(11)
    N = 5003
    if name == "inf":
        host = torch.randn(3, N, generator=g)
        for b in range(3):
            p = torch.randperm(N, generator=g)
            host[b, p[:3]] = float("inf")
            host[b, p[3:60]] = NEG_INF
        return host
    if name == "negative":
        host = -torch.rand(3, N, generator=g) - 5.0
        host[1] *= 1e20
        return host
    if name == "zeros_denormals":
        # 30 positive denormals, 20 +0.0 and 20 -0.0 interleaved, the
        # rest distinct negatives (denormal and normal): at k = 100 the
        # zeros sit inside the list and rank 100 is untied, so the
        # indices are checked, with +0.0 == -0.0 ordered by index
        host = torch.empty(3, N)
        for b in range(3):
            vals = torch.cat([
                torch.arange(1, 31, dtype=torch.float64) * 1e-41,
                torch.zeros(20, dtype=torch.float64),
                -torch.zeros(20, dtype=torch.float64),
                -torch.arange(1, 1001, dtype=torch.float64) * 1e-42,
                -torch.arange(1, N - 1069, dtype=torch.float64) * 1e-3,
            ]).float()
            host[b] = vals[torch.randperm(N, generator=g)]
        assert int((host == 0).sum()) == 120
        assert int((host.view(torch.int32) == -2**31).sum()) == 60
        return host
    if name == "wide_span":
        e = torch.rand(3, N, generator=g, dtype=torch.float64) * 60 - 30
        sign = torch.where(torch.rand(3, N, generator=g) < 0.5, -1.0, 1.0)
        return (10.0 ** e).float() * sign
    if name == "bin0":
        # the k-th value is -inf, whose ordered top byte is 0
        host = torch.full((3, N), NEG_INF)
        for b in range(3):
            p = torch.randperm(N, generator=g)
            host[b, p[:7]] = torch.randn(7, generator=g)
        return host
    raise KeyError(name)


@pytest.mark.parametrize("k", [1, 100])
@pytest.mark.parametrize("name", ["inf", "negative", "zeros_denormals",
                                  "wide_span", "bin0"])
def test_topk_value_edges(name, k):
    _run(_value_rows(name), k, what=f"{name} k={k}")


# -------------------------------------------------------------- near-ties

_BAND_N = 100_000


@functools.lru_cache(maxsize=None)
def _band(rows: int, seed: int = 3) -> torch.Tensor:
    """1 + u * 2^-7, u uniform in [0, 1): every value shares the top 16
    bits of its ordered form (sign, exponent, 7 mantissa bits), far more
    of them than the tie region holds, and about half are exact
    duplicates of another. Callers must not write into the result."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(rows, _BAND_N, generator=g, dtype=torch.float64)
    return (1.0 + u * 2.0 ** -7).float()


@pytest.mark.parametrize("k", [10, 1024])
def test_topk_near_tie_band(k):
    _run(_band(2), k, what=f"band k={k}")


@pytest.mark.parametrize("k", [10, 1024])
def test_topk_near_tie_band_negated(k):
    _run(-_band(2), k, what=f"-band k={k}")


@pytest.mark.parametrize("k", [10, 1024])
def test_topk_near_tie_band_with_outliers(k):
    """5 values above the band: the strictly-above region is in use
    while the threshold bin overflows."""
    host = _band(2).clone()
    g = torch.Generator().manual_seed(5)
    for b in range(2):
        p = torch.randperm(_BAND_N, generator=g)[:5]
        host[b, p] = torch.tensor([1.5, 2.0, 3.0, 1e10, 1.0 + 2.0 ** -6])
    _run(host, k, what=f"band+outliers k={k}")


@pytest.mark.parametrize("k", [10, 1024])
def test_topk_near_tie_band_ext_hist1(k):
    host = _band(2)
    hist = _ordered_top_hist(host)
    assert int(hist.sum()) == host.numel()
    vals, idx = K.TopK()(host.cuda(), k,
                         ext_hist1=hist.to(torch.int32).cuda())
    _check_topk(host, k, vals, idx, what=f"band ext_hist1 k={k}")


@pytest.mark.parametrize("k", [10, 1024])
def test_topk_near_tie_band_masked(k):
    host = _band(3)
    g = torch.Generator().manual_seed(9)
    bits = _random_mask(2, _BAND_N, 0.5, g)
    row_pred = torch.tensor([0, 1, 0], dtype=torch.int32)
    vals, idx = K.TopK()(host.cuda(), k, mask=bits.cuda(),
                         row_pred=row_pred.cuda())
    _check_topk(host, k, vals, idx, bits, row_pred,
                what=f"band masked k={k}")


def test_topk_plateau_24bit():
    """256 distinct values 1 + j * 2^-23, each about 400 times: over
    100 000 elements share the top 24 bits of the threshold, so a
    selector that refines one more byte and stops still has to drop
    candidates that differ."""
    g = torch.Generator().manual_seed(13)
    j = torch.arange(256, dtype=torch.float64).repeat(400)
    host = torch.stack([
        (1.0 + j * 2.0 ** -23).float()[torch.randperm(j.numel(), generator=g)]
        for _ in range(2)])
    assert host.unique().numel() == 256
    _run(host, 100, what="plateau")


def test_topk_mixed_batch():
    """Rows 0 and 2 banded, rows 1 and 3 randn: rows that need no
    refinement are unaffected by rows that do."""
    g = torch.Generator().manual_seed(17)
    host = torch.randn(4, _BAND_N, generator=g)
    host[0::2] = _band(2)
    _run(host, 100, what="mixed")


def test_topk_workspace_reuse():
    """One TopK object over band (B=4), randn (B=2), band again and a
    masked batch: no per-row state of a call survives the workspace's
    zeroed prefix into the next."""
    g = torch.Generator().manual_seed(19)
    band = _band(4, seed=4)
    rnd = torch.randn(2, 20_011, generator=g)
    sel = K.TopK()
    _run(band, 100, what="reuse band #1", sel=sel)
    _run(rnd, 100, what="reuse randn", sel=sel)
    _run(band, 100, what="reuse band #2", sel=sel)
    mhost = torch.cat([_band(1, seed=6), torch.randn(2, _BAND_N,
                                                     generator=g)])
    bits = _random_mask(2, _BAND_N, 0.5, g)
    row_pred = torch.tensor([1, 0, 1], dtype=torch.int32)
    vals, idx = sel(mhost.cuda(), 100, mask=bits.cuda(),
                    row_pred=row_pred.cuda())
    _check_topk(mhost, 100, vals, idx, bits, row_pred, what="reuse masked")
    _run(rnd, 100, what="reuse randn after masked", sel=sel)


# ------------------------------------------------------------------- BM25

_SEGS = [(0, 4097), (4097, 906)]   # (doc_base, nseg): N = 5003, N % 4 = 3
_N_DOCS = 5003
_QUERIES = [
    [1, 2, 3],
    [],                            # no terms: an all-zero row
    [40],                          # empty posting list in segment 1
    [41, 42],                      # 42 has no postings at all
    list(range(50, 62)),           # 12 terms all hitting doc 4096
    [70, 71],                      # pack limits
    [10, 25, 40, 7],
]


@functools.lru_cache(maxsize=None)
def _corpus():
    """{term: [(doc, tf)]} over global doc ids, doc lengths, and the
    oracle scores of _QUERIES. Doc lengths are independent of the tfs:
    kernel and oracle are fed the same (clamped) values."""
    rng = np.random.default_rng(0)
    doc_lens = torch.from_numpy(rng.integers(1, 400, size=_N_DOCS))
    postings: dict[int, list[tuple[int, int]]] = {}
    for t in range(40):
        docs = rng.choice(_N_DOCS, size=int(rng.integers(1, 300)),
                          replace=False)
        postings[t] = [(int(d), int(rng.integers(1, 5)))
                       for d in sorted(docs)]
    # doc ids at the loop bounds: bd-1, bd (= nseg-1 of segment 0, alone
    # in its block at bd=4096), and nseg-1 of segment 1
    postings[40] = [(5, 2), (4095, 1), (4096, 3)]
    postings[41] = [(0, 1), (4095, 2), (4096, 1), (4097, 1), (5002, 4)]
    postings[42] = []
    for t in range(50, 62):
        postings[t] = sorted({(4096, 1 + t % 3), (int(rng.integers(0, 4096)), 1),
                              (int(rng.integers(4097, _N_DOCS)), 2)})
    # tf in {1, 65535} x dl in {1, 32768, 65535}: dl >= 32768 sets the
    # sign bit of the packed i32 word
    lim_docs = {100: 1, 4096: 32768, 5000: 65535}
    for d, dl in lim_docs.items():
        doc_lens[d] = dl
    postings[70] = [(d, 1) for d in sorted(lim_docs)]
    postings[71] = [(d, 65535) for d in sorted(lim_docs)]
    ref = R.bm25_scores(postings, doc_lens,
                        [sorted(set(q)) for q in _QUERIES], _N_DOCS)
    return postings, doc_lens, ref


def _bm25_gpu(queries, bd: int, with_hist: bool):
    """Score `queries` over the two segments with K.bm25_block into one
    NaN-filled [B, N] matrix. Returns (scores, hist or None) on the
    device."""
    postings, doc_lens, _ = _corpus()
    dev = "cuda"
    B = len(queries)
    tlist = [t for q in queries for t in sorted(set(q))]
    qt_off = np.cumsum([0] + [len(set(q)) for q in queries]).astype(np.int32)
    uterms, qt_ut = np.unique(np.array(tlist, dtype=np.int64),
                              return_inverse=True)
    idf = [math.log(1.0 + (_N_DOCS - len(postings[t]) + 0.5)
                    / (len(postings[t]) + 0.5)) for t in tlist]
    avgdl = float(doc_lens.float().mean())
    scores = torch.full((B, _N_DOCS), float("nan"), device=dev)
    hist = torch.zeros(B, 256, dtype=torch.int32, device=dev) \
        if with_hist else None
    for base, nseg in _SEGS:
        doc_ids, packed, begin, end = [], [], [], []
        for t in uterms:
            begin.append(len(doc_ids))
            for d, tf in postings[int(t)]:
                if base <= d < base + nseg:
                    doc_ids.append(d - base)
                    packed.append(tf | (int(doc_lens[d]) << 16))
            end.append(len(doc_ids))
        nblocks = (nseg + bd - 1) // bd
        bounds = torch.empty(max(1, len(uterms) * nblocks * 2),
                             dtype=torch.int32, device=dev)
        # a packed word with bit 31 set does not fit torch.int32 as a
        # Python int: go through numpy's uint32
        tfdl = np.array(packed, dtype=np.uint32).view(np.int32)
        K.bm25_block(
            torch.from_numpy(np.array(doc_ids, dtype=np.int32)).to(dev),
            torch.from_numpy(tfdl).to(dev),
            torch.from_numpy(qt_off).to(dev),
            torch.from_numpy(qt_ut.astype(np.int32)).to(dev),
            torch.tensor(idf, dtype=torch.float32, device=dev),
            torch.from_numpy(np.array(begin, dtype=np.int64)).to(dev),
            torch.from_numpy(np.array(end, dtype=np.int64)).to(dev),
            bounds, scores, doc_base=base, nseg=nseg, bd=bd, avgdl=avgdl,
            hist1=hist)
    return scores, hist


@functools.lru_cache(maxsize=None)
def _bm25_run(bd: int, with_hist: bool):
    scores, hist = _bm25_gpu(_QUERIES, bd, with_hist)
    return scores.cpu(), None if hist is None else hist.cpu()


def _assert_close(gpu, ref, rtol, atol, what):
    err = (gpu - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    assert err <= atol + rtol * scale, f"{what}: max err {err} (scale {scale})"


@pytest.mark.parametrize("with_hist", [False, True])
@pytest.mark.parametrize("bd", [4096, 8192])
def test_bm25_two_segments(bd, with_hist):
    """Two segments (4097 + 906 docs) in one score matrix against the
    scalar oracle, per query row so that a small-score row (tf = 1 on a
    dl = 65535 doc) is not judged on another row's scale."""
    _, doc_lens, ref = _corpus()
    scores, _ = _bm25_run(bd, with_hist)
    assert not torch.isnan(scores).any(), "kernel left columns unwritten"
    for q in range(len(_QUERIES)):
        _assert_close(scores[q], ref[q], rtol=1e-3, atol=1e-3,
                      what=f"bm25 bd={bd} hist={with_hist} query {q}")
    assert bool((scores[1] == 0).all())
    assert int((scores[4] > 0).sum()) == len(
        {d for t in _QUERIES[4] for d, _ in _corpus()[0][t]})
    # the pack-limit postings, against the closed form in f64
    avgdl = float(doc_lens.float().mean())
    idf = math.log(1.0 + (_N_DOCS - 3 + 0.5) / 3.5)
    for d in (100, 4096, 5000):
        norm = 1.2 * (0.25 + 0.75 * float(doc_lens[d]) / avgdl)
        want = sum(idf * tf * 2.2 / (tf + norm) for tf in (1, 65535))
        assert abs(float(scores[5, d]) - want) <= 1e-3 + 1e-3 * want, \
            f"doc {d} dl {int(doc_lens[d])}: {float(scores[5, d])} vs {want}"


@pytest.mark.parametrize("bd", [4096, 8192])
def test_bm25_fused_histogram(bd):
    """hist1= changes no score bit, counts exactly the scores written,
    and drives the selector like its own pass 1."""
    plain, _ = _bm25_run(bd, False)
    scores, hist = _bm25_run(bd, True)
    assert torch.equal(plain.view(torch.int32), scores.view(torch.int32))
    assert torch.equal(hist.long(), _ordered_top_hist(scores))
    assert bool((hist.long().sum(1) == _N_DOCS).all())
    assert int(hist[1, 0x80]) == _N_DOCS      # the +0.0 bin
    for k in (10, 1024):
        vals, idx = K.TopK()(scores.cuda(), k, ext_hist1=hist.cuda())
        _check_topk(scores, k, vals, idx, what=f"bm25 ext_hist1 k={k}")


@pytest.mark.parametrize("with_hist", [False, True])
def test_bm25_batch_without_terms(with_hist):
    """U = 0: no query of the batch has a term."""
    scores, hist = _bm25_gpu([[], []], 4096, with_hist)
    assert bool((scores.cpu() == 0).all())
    assert not bool(torch.signbit(scores).any())
    if with_hist:
        want = torch.zeros(2, 256, dtype=torch.int32)
        want[:, 0x80] = _N_DOCS
        assert torch.equal(hist.cpu(), want)
