"""GPU tests for facet counts over the whole match set: facets.hip
against its numpy oracle, exact; GpuShard against CpuShard and brute
force with filters, tombstones and operands in one batch;
HybridEngine.search_with_facets (MI355X only)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from infomesh_amd.ops import _build
    _build.build()
import term_ops_corpus as C
from facet_cases import brute_counts, corpus_spec
from infomesh_amd.index import doc_attrs as A
from infomesh_amd.index.doc_attrs import (FacetSpec, facet_results, lang16,
                                          pack_facets)
from infomesh_amd.ops import kernels as K
from infomesh_amd.ops import reference as R
from match_set_cases import B, GARBAGE, SCORES, _mask, _size, _u


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.manual_seed(0)


# ------------------------------------------------- kernel vs the oracle

LANGS = sorted(lang16(c) for c in ("de", "en", "ja"))
EDGES = [1000, 2000, 0x80000000]
W0_POOL = [0, 1, 999, 1000, 1001, 2000, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
W1_POOL = [0, lang16("de"), lang16("en"), lang16("ja"), lang16("fr"),
           lang16("en") | (1 << 16)]          # the dead bit is not a language
HASHES = sorted([7, 0x1234, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xDEADBEEF,
                 0xFFFFFFFF])
NOWHERE = 0x55555555                          # a hash in no document


def _attrs(N: int, rng) -> np.ndarray:
    a = np.zeros((N, 4), dtype=np.uint32)
    a[:, 0] = rng.choice(np.asarray(W0_POOL, dtype=np.uint32), size=N)
    a[:, 1] = rng.choice(np.asarray(W1_POOL, dtype=np.uint32), size=N)
    a[:, 2] = rng.choice(np.asarray(HASHES, dtype=np.uint32), size=N)
    return a


def _invariants(counts: np.ndarray, E: int, L: int) -> None:
    sl = K.facet_slots(E, L)
    total = counts[:, sl["total"]]
    dates = counts[:, sl["date_zero"]] \
        + counts[:, sl["date0"]:sl["date0"] + E + 1].sum(1)
    assert np.array_equal(total, dates), "TOTAL != sum of the date slots"
    langs = counts[:, sl["lang_zero"]:sl["lang_other"] + 1].sum(1)
    assert np.array_equal(total, langs), "TOTAL != sum of the language slots"
    assert (counts[:, sl["dom0"]:] <= total[:, None]).all(), \
        "a domain slot above TOTAL"
    assert (counts >= 0).all()


def _run(scores, rows, attrs, edges, langs, desc, doms, mask=None,
         row_pred=None):
    """Kernel and oracle on the same arguments -> the counts, equal."""
    host = (torch.tensor(rows, dtype=torch.int32), _u(attrs).reshape(-1, 4),
            _u(edges), _u(langs),
            torch.tensor(desc, dtype=torch.int32).reshape(-1, 2), _u(doms))
    s = torch.from_numpy(scores)
    want = R.facet_counts(s, *host, mask=mask, row_pred=row_pred)
    got = K.facet_counts(
        s.cuda(), host[0], host[1].cuda(), *host[2:],
        mask=None if mask is None else mask.cuda(),
        row_pred=None if row_pred is None else row_pred.cuda())
    torch.cuda.synchronize()
    E, L = len(edges), len(langs)
    assert got.dtype == torch.int32
    assert got.shape == (len(rows), K.facet_width(E, L, max(
        n for _, n in desc)))
    assert torch.equal(got.cpu(), want)               # all R x F counters
    _invariants(want.numpy(), E, L)
    return want.numpy()


def test_layout_and_chunk_are_what_python_assumes():
    CH = K.facet_chunk_docs()
    assert CH % 1024 == 0 and CH >= 1024
    for E, L in ((0, 0), (3, 3), (7, 32), (5, 11)):
        assert K.facet_slots(E, L) == A.facet_slots(E, L)
        for Dw in (0, 1, 64):
            assert K.facet_width(E, L, Dw) == A.facet_width(E, L, Dw)
    assert (K.FACET_MAX_EDGES, K.FACET_MAX_LANGS, K.FACET_MAX_DOMS) \
        == (A.FACET_MAX_EDGES, A.FACET_MAX_LANGS, A.FACET_MAX_DOMS)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("R_", [1, 3])
@pytest.mark.parametrize("size", ["1", "63", "64", "65", "255", "256", "257",
                                  "C-1", "C", "C+1", "2C+37"])
def test_facet_counts_exact(size, R_, masked):
    CH = K.facet_chunk_docs()
    N = _size(size, CH)
    rng = np.random.default_rng(N * 7 + R_ * 2 + masked)
    rows = [2] if R_ == 1 else [2, 0, 3]
    scores = rng.choice(SCORES, size=(B, N))
    for b in set(range(B)) - set(rows):
        scores[b] = GARBAGE
    attrs = _attrs(N, rng)
    # rows of different widths in one call; a hash that is in no document
    lists = [HASHES[:1], HASHES[2:], sorted([NOWHERE] + HASHES[3:5])][:R_]
    doms, desc = [], []
    for lst in lists:
        desc.append((len(doms), len(lst)))
        doms += lst
    mask = row_pred = None
    if masked:
        mask = _mask(N, CH, rng)
        # rows 0 and 2 share mask row 0, row 3 has the all-zero one, the
        # skipped row 1 the all-ones one
        row_pred = torch.tensor([0, 2, 0, 1], dtype=torch.int32)
    want = _run(scores, rows, attrs, EDGES, LANGS, desc, doms, mask,
                row_pred)
    if masked and R_ == 3:
        assert not want[2].any(), "the all-zero mask row counted something"
        if N > 64:
            assert want[0, 0] > 0 and want[1, 0] > 0
    if not masked:
        # the oracle itself, where the answer is known without it
        for r, b in enumerate(rows):
            assert want[r, 0] == int((scores[b] > 0).sum())
        assert want[:, 0].max() < N or N < 8, "the garbage row leaked"


def test_every_document_in_one_slot():
    """All lanes of every wave add to the same three LDS counters."""
    CH = K.facet_chunk_docs()
    N = 2 * CH + 37
    scores = np.full((B, N), 1.0, dtype=np.float32)
    attrs = np.zeros((N, 4), dtype=np.uint32)
    attrs[:] = (1500, lang16("en"), 0x80000000, 0)
    want = _run(scores, [1, 3], attrs, EDGES, LANGS,
                [(0, len(HASHES)), (0, 1)], HASHES)
    sl = K.facet_slots(3, 3)
    assert want[0, sl["total"]] == N
    assert want[0, sl["date0"] + 1] == N
    assert want[0, sl["lang0"] + LANGS.index(lang16("en"))] == N
    assert want[0, sl["dom0"] + HASHES.index(0x80000000)] == N
    assert want[0].sum() == 4 * N and want[1].sum() == 3 * N


@pytest.mark.parametrize("E,L", [(0, 0), (7, 32), (0, 32), (7, 0)])
def test_edge_and_language_extremes(E, L):
    N = 300
    rng = np.random.default_rng(E * 40 + L)
    edges = [10, 20, 20, 1000, 2000, 0x80000000, 0xFFFFFFFF][:E]
    langs = sorted({lang16(a + b) for a in "de" for b in "abcdefghijklmnop"}
                   | {lang16("de"), lang16("en")})[:L]
    assert len(langs) == L
    scores = rng.choice(SCORES, size=(B, N))
    attrs = _attrs(N, rng)
    attrs[:8, 0] = [0, 10, 20, 1000, 2000, 0x80000000, 0xFFFFFFFF, 9]
    scores[:, :8] = 0.75
    want = _run(scores, [0, 1, 2, 3], attrs, edges, langs,
                [(0, 0), (0, 0), (0, 0), (0, 0)], [])
    sl = K.facet_slots(E, L)
    assert want.shape[1] == 5 + E + L
    assert (want[:, sl["date_zero"]] >= 1).all()          # w0 == 0
    if E == 7:
        # w0 == 0xFFFFFFFF passes all seven edges, 9 passes none
        assert (want[:, sl["date0"] + 7] >= 1).all()
        assert (want[:, sl["date0"]] >= 1).all()
        assert (want[:, sl["date0"] + 2] == 0).all()      # the repeated edge
    if L == 0:
        assert (want[:, sl["lang_other"]] > 0).all()      # nothing is listed
        assert (want[:, sl["lang_zero"]] > 0).all()       # and code 0 is 0


def test_domain_lists_of_0_1_63_and_64_hashes():
    N = 700
    rng = np.random.default_rng(11)
    pool = np.unique(np.concatenate([
        rng.integers(0, 1 << 32, size=80, dtype=np.uint64),
        np.asarray(HASHES, dtype=np.uint64)])).astype(np.uint32)
    assert (pool >= 1 << 31).sum() > 10
    attrs = _attrs(N, rng)
    attrs[:, 2] = rng.choice(pool, size=N)
    scores = rng.choice(SCORES, size=(B, N))
    l63 = sorted(set(pool[:62].tolist()) | {NOWHERE})
    l64 = sorted(pool[-64:].tolist())
    assert len(l63) == 63 and len(l64) == 64
    lists = [[], [int(pool[-1])], l63, l64]
    doms, desc = [], []
    for lst in lists:
        desc.append((len(doms), len(lst)))
        doms += lst
    want = _run(scores, [3, 2, 1, 0], attrs, EDGES, LANGS, desc, doms)
    sl = K.facet_slots(3, 3)
    assert want.shape[1] == sl["dom0"] + 64
    assert not want[0, sl["dom0"]:].any()
    assert want[1, sl["dom0"]] > 0 and not want[1, sl["dom0"] + 1:].any()
    assert want[2, sl["dom0"] + l63.index(NOWHERE)] == 0
    assert want[3, sl["dom0"]:].sum() > 64


def test_over_a_cap_is_a_value_error_before_the_launch():
    N = 64
    scores = torch.ones((B, N), device="cuda")
    attrs = torch.zeros((N, 4), dtype=torch.int32, device="cuda")
    rows = torch.tensor([0], dtype=torch.int32)
    one = torch.tensor([[0, 0]], dtype=torch.int32)
    none = _u([])
    K.facet_counts(scores, rows, attrs, none, none, one, none)   # the good one
    with pytest.raises(ValueError, match="caps"):
        K.facet_counts(scores, rows, attrs, _u(range(1, 9)), none, one, none)
    with pytest.raises(ValueError, match="caps"):
        K.facet_counts(scores, rows, attrs, none, _u(range(1, 34)), one, none)
    with pytest.raises(ValueError, match="caps"):
        K.facet_counts(scores, rows, attrs, none, none,
                       torch.tensor([[0, 65]], dtype=torch.int32),
                       _u(range(65)))
    # what would index outside an array is refused too
    for bad_rows, bad_desc, doms in (([4], [[0, 0]], []), ([-1], [[0, 0]], []),
                                     ([0], [[0, 2]], [5]),
                                     ([0], [[1, 1]], [5]),
                                     ([0], [[0, 2]], [9, 5])):
        with pytest.raises(AssertionError):
            K.facet_counts(scores, torch.tensor(bad_rows, dtype=torch.int32),
                           attrs, none, none,
                           torch.tensor(bad_desc, dtype=torch.int32),
                           _u(doms))
    with pytest.raises(AssertionError):                 # descending edges
        K.facet_counts(scores, rows, attrs, _u([5, 4]), none, one, none)
    with pytest.raises(AssertionError):                 # a repeated language
        K.facet_counts(scores, rows, attrs, none, _u([4, 4]), one, none)
    torch.cuda.synchronize()


# -------------------------------------------------- GpuShard vs CpuShard

@pytest.fixture(scope="module")
def shards():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infomesh_amd.index.gpu_index import CpuShard, GpuShard
    toks, meta, emb = C.corpus()
    return {"gpu": C.build_shard(GpuShard, toks, meta, emb, device="cuda"),
            "cpu": C.build_shard(CpuShard, toks, meta, emb), "meta": meta,
            "sets": [set(t.tolist()) for t in toks]}


def test_gpu_shard_counts_match_cpu_shard_and_brute_force(shards):
    gpu, cpu = shards["gpu"], shards["cpu"]
    terms, q, filters, ops = C.queries()
    spec = corpus_spec(len(terms))
    k = C.K_CMP
    plain = gpu.search(terms, q.cuda(), k=k, filters=filters, term_ops=ops)
    got = gpu.search(terms, q.cuda(), k=k, filters=filters, term_ops=ops,
                     facets=spec)
    torch.cuda.synchronize()
    assert plain.facets is None
    # the hits of the same call with and without facets: bit for bit
    for name in ("bm25_scores", "bm25_ids", "dense_scores", "dense_ids"):
        a, b = getattr(got, name), getattr(plain, name)
        assert a.dtype == b.dtype and torch.equal(
            a.view(torch.int32) if a.dtype == torch.float32 else a,
            b.view(torch.int32) if b.dtype == torch.float32 else b), name
    want = cpu.search(terms, q, k=k, filters=filters, term_ops=ops,
                      facets=spec)
    assert got.facets.dtype == torch.int32
    assert torch.equal(got.facets.cpu(), want.facets)
    packed = pack_facets(spec, len(terms))
    res = facet_results(spec, packed, got.facets.cpu().numpy())
    for qi in range(len(terms)):
        assert res[qi] == brute_counts(terms, filters, ops, shards["meta"],
                                       shards["sets"], spec, qi), qi
    assert min(r.total for r in res) > 0
    # the tombstones alone (no filter, no operand) mask the batch too
    got = gpu.search(terms, q.cuda(), k=k, facets=spec)
    want = cpu.search(terms, q, k=k, facets=spec)
    assert torch.equal(got.facets.cpu(), want.facets)
    none = [None] * len(terms)
    res = facet_results(spec, packed, got.facets.cpu().numpy())
    for qi in range(len(terms)):
        assert res[qi] == brute_counts(terms, none, none, shards["meta"],
                                       shards["sets"], spec, qi), qi


class _SpyTopK:
    """Records how the shard's BM25 selector is called."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __call__(self, scores, k, ext_hist1=None, mask=None, row_pred=None):
        self.calls.append({"ext_hist1": ext_hist1 is not None,
                           "masked": mask is not None})
        return self.real(scores, k, ext_hist1=ext_hist1, mask=mask,
                         row_pred=row_pred)


def test_unmasked_shard_with_facets_keeps_the_fused_histogram():
    """No filter and no tombstone: facets must not mask the batch."""
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
    spec = corpus_spec(len(terms))
    plain = gpu.search(terms, q.cuda(), k=30)
    gpu._topk = spy = _SpyTopK(gpu._get_topk())
    got = gpu.search(terms, q.cuda(), k=30, facets=spec)
    torch.cuda.synchronize()
    assert spy.calls == [{"ext_hist1": True, "masked": False}]
    assert gpu._mask_for(None, len(terms)) is None
    assert torch.equal(got.bm25_ids, plain.bm25_ids)
    assert torch.equal(got.bm25_scores.view(torch.int32),
                       plain.bm25_scores.view(torch.int32))
    want = cpu.search(terms, q, k=30, facets=spec)
    assert torch.equal(got.facets.cpu(), want.facets)
    sets = [set(t.tolist()) for t in toks[:110]]
    sl = K.facet_slots(3, 3)
    for qi, t in enumerate(terms):
        assert int(got.facets[qi, sl["total"]]) == sum(
            1 for d in sets if set(t.tolist()) & d)


# ---------------------------------------------------------------- engine

def test_engine_search_with_facets_on_the_device():
    from infomesh_amd.engine import HybridEngine
    from infomesh_amd.index.local_store import Document
    eng = HybridEngine(device="cuda", use_encoder=True)
    for i in range(40):
        words = ["rust"] + (["java"] if i % 2 == 0 else ["golang"]) \
            + [f"note{i}"] * i
        eng.add_document(Document(
            url=f"https://{'x.org' if i % 4 == 0 else 'y.net'}/{i}",
            title=f"t{i}", text=" ".join(words), doc_id=i,
            language="en" if i % 5 else "de", crawled_at=1000.0 + i))
    eng.flush()
    eng.delete_documents([39])
    spec = FacetSpec(date_edges=(1020,), languages=("en", "de"),
                     domains=(("x.org", "y.net", "z.io"), None, ("x.org",)))
    queries = ["rust", "rust", "java"]
    plain = eng.search_many(queries, limit=40)
    hits, counts = eng.search_with_facets(
        queries, limit=40, facets=spec, exclude=[None, None, ("note4",)])
    assert counts[1] is None
    assert [[h.doc_id for h in row] for row in hits[:2]] \
        == [[h.doc_id for h in row] for row in plain[:2]]
    c = counts[0]                     # documents 0..38 hold "rust"
    assert c.total == 39 and c.date_zero == 0 and c.dates == (20, 19)
    assert c.languages == {"en": 31, "de": 8}
    assert c.language_zero == 0 and c.language_other == 0
    assert c.domains == {"x.org": 10, "y.net": 29, "z.io": 0}
    c = counts[2]                     # even documents but 4 hold "java"
    assert c.total == 19 and c.domains == {"x.org": 9}
    # the dense plane returns every passing document, with or without
    # the word; those take no part in the counts
    assert 4 not in [h.doc_id for h in hits[2]] and len(hits[2]) == 38
    # no spec: nothing is counted, and the hits are search_many's
    hits, counts = eng.search_with_facets(queries, limit=40)
    assert counts == [None, None, None]
    assert [[h.doc_id for h in row] for row in hits] \
        == [[h.doc_id for h in row] for row in plain]
