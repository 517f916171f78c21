"""GPU tests for the top domains of the whole match set: domtop.hip's
domain_count and domain_select against numpy, exact and bit for bit;
GpuShard against CpuShard; HybridEngine.search_with_facets with names
(MI355X only)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from infomesh_amd.ops import _build
    _build.build()
import term_ops_corpus as C
from facet_cases import corpus_spec
from infomesh_amd.index.doc_attrs import (TOP_FETCH, FacetSpec, domain_hash,
                                          domain_tables_np, pack_facets)
from infomesh_amd.ops import kernels as K
from infomesh_amd.ops import reference as R
from match_set_cases import B, GARBAGE, SCORES, _mask, _size, _u


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.manual_seed(0)


def _count(scores, rows, dom_id, D, mask=None, row_pred=None, out=None):
    """Kernel and oracle on the same arguments -> the tally, equal."""
    s = torch.from_numpy(scores)
    rows_t = torch.tensor(rows, dtype=torch.int32)
    ids = torch.from_numpy(np.asarray(dom_id, dtype=np.int32))
    want = R.domain_count(s, rows_t, ids, D, mask=mask, row_pred=row_pred)
    got = K.domain_count(
        s.cuda(), rows_t, ids.cuda(), D,
        mask=None if mask is None else mask.cuda(),
        row_pred=None if row_pred is None else row_pred.cuda(), out=out)
    torch.cuda.synchronize()
    assert got.dtype == torch.int32 and got.shape == (len(rows), D)
    assert torch.equal(got.cpu(), want)
    return want.numpy()


def test_exported_sizes():
    CH, S = K.domtop_chunk_docs(), K.domtop_lds_slots()
    assert CH == K.facet_chunk_docs()         # one queue, one chunk size
    assert S >= 64 and S & (S - 1) == 0 and S < CH
    assert K.domtop_k_max() == TOP_FETCH + 1 == 65


# ------------------------------------------------ domain_count vs numpy

@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("R_", [1, 3])
@pytest.mark.parametrize("size", ["1", "63", "64", "65", "257", "C-1", "C",
                                  "C+1", "2C+37"])
def test_domain_count_exact(size, R_, masked):
    CH = K.domtop_chunk_docs()
    N = _size(size, CH)
    rng = np.random.default_rng(N * 7 + R_ * 2 + masked)
    rows = [2] if R_ == 1 else [2, 0, 3]
    scores = rng.choice(SCORES, size=(B, N))
    for b in set(range(B)) - set(rows):
        scores[b] = GARBAGE
    # a few heavy domains and a long tail, as a Zipf draw gives them
    D = 300
    dom_id = np.minimum(rng.zipf(1.3, size=N) - 1, D - 1)
    mask = row_pred = None
    if masked:
        mask = _mask(N, CH, rng)
        row_pred = torch.tensor([0, 2, 0, 1], dtype=torch.int32)
    want = _count(scores, rows, dom_id, D, mask, row_pred)
    if masked and R_ == 3:
        assert not want[2].any(), "the all-zero mask row counted something"
        if N > 64:
            assert want[0].sum() > 0 and want[1].sum() > 0
    if not masked:
        for r, b in enumerate(rows):
            assert want[r].sum() == int((scores[b] > 0).sum())
        assert want.sum(1).max() < N or N < 8, "the garbage row leaked"


def test_every_document_its_own_domain_overflows_the_lds_table():
    CH = K.domtop_chunk_docs()
    N = CH + 1
    assert CH > K.domtop_lds_slots()
    scores = np.full((B, N), 1.0, dtype=np.float32)
    perm = np.random.default_rng(5).permutation(N)
    want = _count(scores, [1, 3], perm, N)
    assert (want == 1).all()


def test_one_domain_for_every_document():
    CH = K.domtop_chunk_docs()
    N = 2 * CH + 37
    scores = np.full((B, N), 1.0, dtype=np.float32)
    # among several ids, and with the workspace form of `out`
    ws = torch.full((3 * 7 + 5,), 77, dtype=torch.int32, device="cuda")
    want = _count(scores, [1, 3, 0], np.full(N, 4), 7,
                  out=ws[:21].view(3, 7))
    assert (want[:, 4] == N).all() and want.sum() == 3 * N
    assert (ws[21:] == 77).all()
    # D = 1
    want = _count(scores, [2], np.zeros(N), 1)
    assert want.tolist() == [[N]]


# ----------------------------------------------- domain_select vs lexsort

def _keys(D: int, rng) -> np.ndarray:
    """D distinct hashes, ascending as unsigned, on both sides of 2^31."""
    fixed = [0, 1, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFF]
    if D <= len(fixed):
        return np.asarray(sorted(fixed[-D:]), dtype=np.uint32)
    more = np.unique(rng.integers(2, (1 << 32) - 1, size=2 * D))
    more = more[~np.isin(more, fixed)]
    more = rng.permutation(more)[:D - len(fixed)]
    keys = np.sort(np.concatenate([np.asarray(fixed, dtype=np.int64), more]))
    assert len(keys) == D
    return keys.astype(np.uint32)


def _select(cnt: np.ndarray, keys: np.ndarray, K_: int) -> np.ndarray:
    c = torch.from_numpy(np.asarray(cnt, dtype=np.int32).reshape(-1, len(keys)))
    k = _u(keys)
    want = R.domain_select(c, k, K_)
    got = K.domain_select(c.cuda(), k.cuda(), K_)
    torch.cuda.synchronize()
    assert got.dtype == torch.int32 and got.shape == want.shape
    assert torch.equal(got.cpu(), want)                    # bit for bit
    return want.numpy()


@pytest.mark.parametrize("K_", [1, 8, 65])
def test_domain_select_exact(K_):
    rng = np.random.default_rng(K_)
    for D in sorted({1, K_ - 1, K_, K_ + 1, 5000} - {0}):
        keys = _keys(D, rng)
        assert D < 4 or (keys[0] < 1 << 31 <= keys[-1])
        rows = [
            np.minimum(rng.zipf(1.2, size=D), 1 << 20),    # ties at 1, 2, ..
            rng.integers(0, 3, size=D),                    # many zeros
            np.full(D, 5),                                 # all equal
            np.zeros(D),                                   # nothing matched
            rng.integers(0, 1 << 31, size=D),              # large counts
        ]
        rows[4][rng.integers(0, D)] = (1 << 31) - 1
        rows[4][rng.integers(0, D)] = (1 << 31) - 1
        want = _select(np.stack(rows), keys, K_)
        assert not want[3].any(), "padding is (0, 0)"
        n_eq = min(K_, D)                  # all equal: the smallest hashes
        assert want[2, :n_eq, 0].view(np.uint32).tolist() \
            == keys[:n_eq].tolist()
        assert (want[2, :n_eq, 1] == 5).all() and not want[2, n_eq:].any()
        assert want[4, 0, 1] == (1 << 31) - 1
        real = want[:, :, 1] > 0
        # real entries come first, counts descend
        assert (real[:, :-1] >= real[:, 1:]).all()
        assert (want[:, :-1, 1] >= want[:, 1:, 1]).all()


def _boundary_rows(D: int, rng) -> np.ndarray:
    """Every count non-zero, so the select sees exactly D keys."""
    return np.stack([np.full(D, 5),                        # all equal
                     np.arange(1, D + 1),                  # all distinct
                     rng.integers(1, 3, size=D)])          # two values


@pytest.mark.parametrize("K_", [1, 65])
@pytest.mark.parametrize("D", [2047, 2048, 2049, 4097])
def test_domain_select_at_the_candidate_boundary(D, K_):
    """D non-zero counts just below, at and above the 2048 candidate
    keys the select sorts in LDS: with one key more a radix pass runs
    first (4097: more than twice the buffer)."""
    rng = np.random.default_rng(D * 3 + K_)
    keys = _keys(D, rng)
    want = _select(_boundary_rows(D, rng), keys, K_)
    assert want[0, :, 0].view(np.uint32).tolist() == keys[:K_].tolist()
    assert (want[0, :, 1] == 5).all()
    assert want[1, :, 1].tolist() == list(range(D, D - K_, -1))
    assert (want[:, :, 1] > 0).all()
    assert (want[:, :-1, 1] >= want[:, 1:, 1]).all()


def test_domain_select_among_thousands_of_ties():
    """More tied domains than the candidate buffer holds: the ids decide,
    exactly, through every radix pass."""
    rng = np.random.default_rng(9)
    D = 200_003
    keys = _keys(D, rng)
    cnt = np.ones((2, D))
    cnt[0, rng.choice(D, size=40, replace=False)] = 2
    cnt[1, ::2] = 0
    want = _select(cnt, keys, 65)
    assert (want[0, :40, 1] == 2).all() and (want[0, 40:, 1] == 1).all()
    ones = keys[cnt[0] == 1][:25]
    assert want[0, 40:, 0].view(np.uint32).tolist() == ones.tolist()
    assert want[1, :, 0].view(np.uint32).tolist() == keys[1::2][:65].tolist()


def test_over_a_cap_is_a_value_error_before_the_launch():
    N = 64
    scores = torch.ones((B, N), device="cuda")
    ids = torch.zeros(N, dtype=torch.int32, device="cuda")
    rows = torch.tensor([0], dtype=torch.int32)
    cnt = K.domain_count(scores, rows, ids, 3)             # the good ones
    keys = _u([1, 2, 3]).cuda()
    K.domain_select(cnt, keys, 65)
    for bad in (0, 66, -1):
        with pytest.raises(ValueError, match="K ="):
            K.domain_select(cnt, keys, bad)
    with pytest.raises(ValueError, match="D ="):
        K.domain_count(scores, rows, ids, 0)
    # what would index outside an array is refused too
    for bad_rows in ([4], [-1]):
        with pytest.raises(AssertionError):
            K.domain_count(scores, torch.tensor(bad_rows, dtype=torch.int32),
                           ids, 3)
    with pytest.raises(AssertionError):
        K.domain_count(scores, rows, ids[:-1], 3)
    with pytest.raises(AssertionError):
        K.domain_select(cnt, keys[:2], 2)
    torch.cuda.synchronize()


# -------------------------------------------------- GpuShard vs CpuShard

@pytest.fixture(scope="module")
def shards():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infomesh_amd.index.gpu_index import CpuShard, GpuShard
    toks, meta, emb = C.corpus()
    return {"gpu": C.build_shard(GpuShard, toks, meta, emb, device="cuda"),
            "cpu": C.build_shard(CpuShard, toks, meta, emb)}


def _top_spec(n_rows: int) -> FacetSpec:
    base = corpus_spec(n_rows)
    return FacetSpec(date_edges=base.date_edges, languages=base.languages,
                     domains=base.domains,
                     top_domains=tuple(3 if i != 1 else 0
                                       for i in range(n_rows)))


def test_gpu_shard_top_domains_match_cpu_shard(shards):
    gpu, cpu = shards["gpu"], shards["cpu"]
    terms, q, filters, ops = C.queries()
    spec = _top_spec(len(terms))
    k = C.K_CMP
    before = gpu.hbm_bytes()
    plain = gpu.search(terms, q.cuda(), k=k, filters=filters, term_ops=ops)
    got = gpu.search(terms, q.cuda(), k=k, filters=filters, term_ops=ops,
                     facets=spec)
    torch.cuda.synchronize()
    assert plain.dom_top is None and plain.dom_tally is None
    for name in ("bm25_scores", "bm25_ids", "dense_scores", "dense_ids"):
        a, b = getattr(got, name), getattr(plain, name)
        assert a.dtype == b.dtype and torch.equal(
            a.view(torch.int32) if a.dtype == torch.float32 else a,
            b.view(torch.int32) if b.dtype == torch.float32 else b), name
    want = cpu.search(terms, q, k=k, filters=filters, term_ops=ops,
                      facets=spec)
    Rt = len(terms) - 1
    assert got.dom_top.dtype == torch.int32
    assert got.dom_top.shape == (Rt, TOP_FETCH + 1, 2)
    assert torch.equal(got.dom_top.cpu(), want.dom_top)
    assert torch.equal(got.facets.cpu(), want.facets)
    assert int((want.dom_top[:, 0, 1] > 0).sum()) == Rt
    # the tables, and the tally's lookup: every domain, one the shard
    # does not hold, and both ends of the key range
    keys, ids = domain_tables_np(cpu.attrs.numpy())
    assert torch.equal(gpu._domain_tables()[0].cpu(), torch.from_numpy(keys))
    assert torch.equal(gpu._domain_tables()[1].cpu(), torch.from_numpy(ids))
    ask = _u([domain_hash(d) for d in C.DOMAINS]
             + [0x55555555, 0, 0xFFFFFFFF]).repeat(Rt, 1)
    look = got.dom_tally.lookup(ask.cuda())
    assert torch.equal(look.cpu(), want.dom_tally.lookup(ask))
    assert int(look[:, :4].sum()) > 0 and not look[:, 4:].any()
    assert gpu.hbm_bytes() > before          # tables and workspace count
    # a delete keeps the tables, an append drops them
    tables = gpu._dom_tables
    assert gpu.delete([C.GID0 + 1]) == 1 and gpu._dom_tables is tables
    assert cpu.delete([C.GID0 + 1]) == 1
    got = gpu.search(terms, q.cuda(), k=k, facets=spec)
    want = cpu.search(terms, q, k=k, facets=spec)
    assert torch.equal(got.dom_top.cpu(), want.dom_top)


class _SpyTopK:
    """Records how the shard's BM25 selector is called."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __call__(self, scores, k, ext_hist1=None, mask=None, row_pred=None):
        self.calls.append({"ext_hist1": ext_hist1 is not None,
                           "masked": mask is not None})
        return self.real(scores, k, ext_hist1=ext_hist1, mask=mask,
                         row_pred=row_pred)


def test_unmasked_shard_with_top_domains_keeps_the_fused_histogram():
    from infomesh_amd.index.doc_attrs import pack_attrs
    from infomesh_amd.index.gpu_index import CpuShard, GpuShard
    toks, meta, emb = C.corpus()
    pair = []
    for cls, kw in ((GpuShard, {"device": "cuda"}), (CpuShard, {})):
        s = cls(**kw)
        for lo, hi in ((0, 45), (45, 110)):
            for i in range(lo, hi):
                s.add_document(C.GID0 + i, toks[i], emb[i],
                               attrs=pack_attrs(*meta[i]))
            s.build()
        pair.append(s)
    gpu, cpu = pair
    terms, q, _, _ = C.queries()
    spec = _top_spec(len(terms))
    plain = gpu.search(terms, q.cuda(), k=30)
    gpu._topk = spy = _SpyTopK(gpu._get_topk())
    got = gpu.search(terms, q.cuda(), k=30, facets=spec)
    torch.cuda.synchronize()
    assert spy.calls == [{"ext_hist1": True, "masked": False}]
    assert torch.equal(got.bm25_ids, plain.bm25_ids)
    assert torch.equal(got.bm25_scores.view(torch.int32),
                       plain.bm25_scores.view(torch.int32))
    want = cpu.search(terms, q, k=30, facets=spec)
    assert torch.equal(got.dom_top.cpu(), want.dom_top)
    # the four domains of the corpus, all counted, nothing behind them
    assert (want.dom_top[:, :4, 1] > 0).all() and not want.dom_top[:, 4:].any()


# ---------------------------------------------------------------- engine

def test_engine_top_domains_on_the_device():
    from infomesh_amd.engine import HybridEngine
    from infomesh_amd.index.local_store import Document
    eng = HybridEngine(device="cuda", use_encoder=True)
    sites = ["x.org", "y.net", "y.net", "z.io", "y.net", "x.org", "w.dev"]
    for i in range(42):
        words = ["rust"] + (["java"] if i % 2 == 0 else ["golang"]) \
            + [f"note{i}"] * i
        eng.add_document(Document(
            url=f"https://{sites[i % 7]}/{i}", title=f"t{i}",
            text=" ".join(words), doc_id=i, language="en",
            crawled_at=1000.0 + i))
    eng.flush()
    eng.delete_documents([41])                # a w.dev document
    spec = FacetSpec(domains=((), None, ("x.org",)), top_domains=(3, 0, 32))
    queries = ["rust", "rust", "java"]
    plain = eng.search_many(queries, limit=40)
    hits, counts = eng.search_with_facets(queries, limit=40, facets=spec)
    assert [[h.doc_id for h in row] for row in hits] \
        == [[h.doc_id for h in row] for row in plain]
    assert counts[1] is None
    live = [i for i in range(41)]
    def top(docs, T):
        tally = {}
        for i in docs:
            tally[sites[i % 7]] = tally.get(sites[i % 7], 0) + 1
        order = sorted(tally, key=lambda d: (-tally[d], domain_hash(d)))
        return [(d, tally[d]) for d in order[:T]]
    c = counts[0]
    assert c.total == 41 and c.top_domains_exact and c.top_domains_bound == 0
    assert [(eng.domain_name(h), n) for h, n in c.top_domains] \
        == top(live, 3)
    assert c.top_domains[0] == (domain_hash("y.net"), 18)
    c = counts[2]
    assert c.domains == {"x.org": 6}
    assert [(eng.domain_name(h), n) for h, n in c.top_domains] \
        == top([i for i in live if i % 2 == 0], 32)
    assert len(c.top_domains) == 4 and eng.domain_name(12345) is None
    # a spec without top rows answers as it always did
    _, counts = eng.search_with_facets(
        queries, limit=40, facets=FacetSpec(domains=((), None, None)))
    assert counts[0].top_domains is None and counts[0].total == 41
    assert pack_facets(FacetSpec(domains=((),)), 1).top == ()
