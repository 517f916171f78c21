"""Required / excluded query terms (+word / -word), everything that runs
without a GPU: the parser, TermOps, the numpy oracle of termmask.hip
against brute force, CpuShard on a three-segment corpus, the query
plane's packing and a 2-rank gloo run, and the FTS5 path."""
from __future__ import annotations

import dataclasses
import os

import numpy as np
import pytest
import torch

import term_ops_corpus as C
from infomesh_amd.config import Config, GpuConfig
from infomesh_amd.index.doc_attrs import (TERM_OPS_MAX, DocFilter, TermOps,
                                          pack_attrs, pack_pred, words_i32)
from infomesh_amd.index.gpu_index import CpuShard, bm25_term_ids
from infomesh_amd.index.local_store import Document, LocalStore
from infomesh_amd.ops import reference as R
from infomesh_amd.parallel.fabric import Fabric
from infomesh_amd.parallel.query_plane import (MAX_QUERY_TERMS,
                                               DistributedQueryPlane,
                                               pack_term_row,
                                               unpack_term_row)
from infomesh_amd.search.nlp import parse_query_filters, parse_term_operators
from infomesh_amd.services import AppContext


# ---------------------------------------------------------------- parser

def test_parser_splits_operators_off():
    assert parse_term_operators("rust +async -java") == (
        "rust async", ("async",), ("java",))
    assert parse_term_operators("-Java rust +Async +async -java") == (
        "rust Async async", ("async",), ("java",))


@pytest.mark.parametrize("text", ["well-known - x", "a-b", "-site:a.org",
                                  "plain words", "", "x - +", "a+b c-"])
def test_parser_leaves_everything_else_alone(text):
    assert parse_term_operators(text) == (text, (), ())


def test_parse_query_filters_is_unchanged():
    # the strings tests/test_domain_sets_cpu.py pins, with their results
    pq = parse_query_filters("rust site:A.org,b.org async")
    assert (pq.text, pq.sites) == ("rust async", ("a.org", "b.org"))
    pq = parse_query_filters("rust -site:a.org")
    assert (pq.text, pq.exclude_sites) == ("rust", ("a.org",))
    pq = parse_query_filters("-site:a.org,B.org rust lang:de")
    assert (pq.text, pq.exclude_sites, pq.language) == (
        "rust", ("a.org", "b.org"), "de")
    pq = parse_query_filters("rust site:kernel.org")
    assert (pq.text, pq.site, pq.sites) == ("rust", "kernel.org", ())
    assert parse_query_filters("well-known -lang:de").text == "well-known -"
    # operators pass through it untouched and are read from what it leaves
    pq = parse_query_filters("rust -java -site:a.org +async lang:de")
    assert pq.text == "rust -java +async"
    assert parse_term_operators(pq.text) == ("rust async", ("async",),
                                             ("java",))


# --------------------------------------------------------------- TermOps

def test_term_ops_dedupes_and_caps():
    t = TermOps.of(require=[5, 3, 5, 3], exclude=[9, 9, 5])
    assert t.require == (5, 3) and t.exclude == (9, 5)
    assert not TermOps.of() and TermOps.of(exclude=[1])
    TermOps.of(range(10), range(10, 16))                  # 16: the cap
    assert TERM_OPS_MAX == 16
    with pytest.raises(ValueError):
        TermOps.of(range(10), range(10, 17))              # 17
    with pytest.raises(ValueError):
        TermOps(require=tuple(range(17)))
    with pytest.raises(dataclasses.FrozenInstanceError):
        t.require = ()


# ---------------------------------------------------------------- oracle

def _csr(token_sets, lo, hi, vocab):
    """Postings of documents lo..hi-1 as (doc_ids, offsets): ids
    segment-local, ascending per term."""
    per_term = [[] for _ in range(vocab)]
    for d in range(lo, hi):
        for t in sorted(token_sets[d]):
            per_term[t].append(d - lo)
    offs = np.zeros(vocab + 1, dtype=np.int64)
    np.cumsum([len(p) for p in per_term], out=offs[1:])
    ids = np.asarray([d for p in per_term for d in p], dtype=np.int32)
    return torch.from_numpy(ids), offs


def test_oracle_matches_brute_force_over_token_sets():
    rng = np.random.default_rng(5)
    N, V = 203, 12
    token_sets = [set(rng.integers(0, V - 1, size=rng.integers(0, 5)).tolist())
                  for _ in range(N)]                     # term V-1: nowhere
    a = words_i32([pack_attrs("en", "a.org", C.T0 + i) for i in range(N)])
    preds = words_i32([pack_pred(None),
                       pack_pred(DocFilter(after=C.T0 + 40))])
    base = R.filter_bitmask(torch.from_numpy(a), torch.from_numpy(preds))
    rows = [(0, [3], [1]), (1, [], [0, 2]), (0, [V - 1], []),
            (1, [4, 5], [4]), (0, [2], [])]
    ids = np.asarray([t for _, rq, ex in rows for t in rq + ex])
    op_off = np.zeros(len(rows) + 1, dtype=np.int32)
    np.cumsum([len(rq) + len(ex) for _, rq, ex in rows], out=op_off[1:])
    kind = np.asarray([k for _, rq, ex in rows
                       for k in [0] * len(rq) + [1] * len(ex)], dtype=np.int32)
    segs = []
    for lo, hi in ((0, 45), (45, 110), (110, N)):        # bases 0, 45, 110
        doc_ids, offs = _csr(token_sets, lo, hi, V)
        segs.append((doc_ids, lo, hi - lo, torch.from_numpy(offs[ids]),
                     torch.from_numpy(offs[ids + 1])))
    before = base.clone()
    got = R.term_bitmask(base, torch.tensor([r[0] for r in rows]), segs,
                         torch.from_numpy(op_off), torch.from_numpy(kind), N)
    assert torch.equal(base, before)
    W = (N + 63) // 64 * 2
    assert got.shape == (len(rows), W) and got.dtype == torch.int32
    bits = np.unpackbits(got.numpy().view(np.uint8), axis=1,
                         bitorder="little").astype(bool)
    assert not bits[:, N:].any()
    for r, (p, rq, ex) in enumerate(rows):
        for d in range(N):
            want = ((p == 0 or d >= 40) and set(rq) <= token_sets[d]
                    and not set(ex) & token_sets[d])
            assert bits[r, d] == want, (r, d)
    assert not bits[2].any() and not bits[3].any()       # nowhere; both lists


# -------------------------------------------------------------- CpuShard

@pytest.fixture(scope="module")
def corpus():
    toks, meta, emb = C.corpus()
    return {"toks": toks, "meta": meta, "emb": emb,
            "sets": [set(t.tolist()) for t in toks],
            "shard": C.build_shard(CpuShard, toks, meta, emb)}


def test_cpu_shard_operators_filters_and_tombstones(corpus):
    shard, meta, sets = corpus["shard"], corpus["meta"], corpus["sets"]
    terms, q, filters, ops = C.queries()
    k = 60
    got = shard.search(terms, q, k=k, filters=filters, term_ops=ops)
    plain = shard.search(terms, q, k=k, filters=filters)
    for ids in (got.bm25_ids, got.dense_ids):
        for qi, (f, t) in enumerate(zip(filters, ops)):
            row = ids[qi][ids[qi] >= 0].tolist()
            n_pass = sum(C.passes(C.GID0 + i, meta, f, t, sets)
                         for i in range(C.N_DOCS))
            assert len(row) == len(set(row)) == min(k, n_pass), (qi, n_pass)
            assert all(C.passes(g, meta, f, t, sets) for g in row), qi
    assert (got.bm25_ids[5] >= 0).sum() == 6              # the segment edges
    for qi, t in enumerate(ops):
        if t is None:      # a row without operators is the search without
            for name in ("bm25_ids", "bm25_scores", "dense_ids",
                         "dense_scores"):
                assert torch.equal(getattr(got, name)[qi],
                                   getattr(plain, name)[qi]), (qi, name)


def test_oracle_scores_are_untied_enough_to_compare_ids(corpus):
    """The GPU test compares ids with this shard's wherever its scores
    are not tied and may skip at most MAX_TIED of the positions: the
    oracle alone must stay inside that on the committed corpus."""
    terms, q, filters, ops = C.queries()
    want = corpus["shard"].search(terms, q, k=C.K_CMP + 1, filters=filters,
                                  term_ops=ops)
    for scores in (want.bm25_scores, want.dense_scores):
        must, tied = C.untied(scores, C.K_CMP)
        print(f"tied share {tied:.3f}, compared positions {int(must.sum())}")
        assert tied <= C.MAX_TIED


def test_cpu_shard_operators_without_filter_or_tombstone(corpus):
    toks, meta, emb = corpus["toks"], corpus["meta"], corpus["emb"]
    shard = CpuShard()
    for i in range(50):
        shard.add_document(C.GID0 + i, toks[i], emb[i])
    shard.build()
    terms, q, _, _ = C.queries()
    ops = [TermOps.of(exclude=[C.EVERY3]), None,
           TermOps.of(require=[C.NOWHERE]),
           TermOps.of(require=[C.EVERY5], exclude=[C.EVERY5])]
    got = shard.search(terms[:4], q[:4], k=50, term_ops=ops)
    row = got.dense_ids[0][got.dense_ids[0] >= 0].tolist()
    assert sorted(row) == [C.GID0 + i for i in range(50) if i % 3]
    assert (got.dense_ids[1] >= 0).all()
    for qi in (2, 3):      # nowhere in the shard; the same id in both lists
        assert (got.bm25_ids[qi] == -1).all()
        assert torch.isinf(got.dense_scores[qi]).all()


# ------------------------------------------------- query plane: packing

def test_packed_row_round_trips_and_keeps_operands_in_a_long_query():
    terms = np.arange(100, 132, dtype=np.int64)            # 32 scoring terms
    ops = TermOps.of(require=[101, 130, 7], exclude=[900, 131])
    row = pack_term_row(terms, ops)
    assert len(row) == MAX_QUERY_TERMS
    back, got = unpack_term_row(np.concatenate([row, [-1, -1]]))
    assert got == ops                        # all five survive the cut
    # scoring terms: the required ones that were scored, then the others
    # up to the cut; 7 (never a scoring term) and the exclusions are not
    assert 7 not in back and 900 not in back and 131 not in back
    assert set(back) <= set(terms.tolist()) and {101, 130} <= set(back)
    assert len(back) == MAX_QUERY_TERMS - 3
    # a short row, and one without operands
    back, got = unpack_term_row(pack_term_row(np.array([4, 5, 6]), TermOps.of(
        require=[5], exclude=[6])))
    assert sorted(back.tolist()) == [4, 5, 6]  # 6 is scored AND excluded
    assert got == TermOps.of(require=[5], exclude=[6])
    # a repeated required word keeps its repeats: the same multiset of
    # scoring terms as at world 1, where the row is not packed at all
    back, got = unpack_term_row(pack_term_row(
        np.array([5, 4, 5, 6, 5, 4]), TermOps.of(require=[5, 9])))
    assert sorted(back.tolist()) == [4, 4, 5, 5, 5, 6]
    assert got == TermOps.of(require=[5, 9])
    back, got = unpack_term_row(pack_term_row(np.array([4, 5]), None))
    assert back.tolist() == [4, 5] and got is None
    # ids reach up to 2^17 - 1 and stay clear of the flag bits
    back, got = unpack_term_row(pack_term_row(
        np.array([131071]), TermOps.of(exclude=[131071])))
    assert back.tolist() == [131071] and got.exclude == (131071,)


# ---------------------------------------------- query plane: two ranks

_K2 = 25
_N2 = 2 * _K2      # every candidate of a row: its BM25 and its dense list


def _two_rank_shards():
    """Rank 0: the corpus. Rank 1: documents that hold the scoring terms
    of both queries many times (they would win every list), each with
    EVERY3 and none with EVERY5, so the operands below fail them all."""
    toks, meta, emb = C.corpus()
    s0 = CpuShard()
    for i in range(C.N_DOCS):
        s0.add_document(C.GID0 + i, toks[i], emb[i])
    s0.build()
    terms, q, _, _ = C.queries()
    s1 = CpuShard()
    for i in range(40):
        body = np.concatenate([terms[0], terms[1]] * 3 + [[C.EVERY3]]
                              + [[C.FILLER] * i])
        s1.add_document(90_000 + i, body.astype(np.int64), q[i % 2].bfloat16())
    s1.build()
    ops = [TermOps.of(exclude=[C.EVERY3]), TermOps.of(require=[C.EVERY5])]
    return s0, s1, terms[:2], q[:2], ops


def _gloo_worker(rank: int, port: int, out_file: str):
    os.environ["HIP_VISIBLE_DEVICES"] = "-1"
    os.environ["CUDA_VISIBLE_DEVICES"] = "-1"
    assert not torch.cuda.is_available(), "GPUs still visible to the worker"
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": "2",
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    fabric = Fabric(backend="gloo")
    s0, s1, terms, q, ops = _two_rank_shards()
    plane = DistributedQueryPlane(s1 if rank else s0, fabric, k_per_shard=_K2)
    fused = plane.search_batch(None if rank else terms, None if rank else q,
                               B=2, dim=C.DIM, n_results=_N2,
                               term_ops=None if rank else ops)
    # one list only: nothing can tie across lists, the ids are exact
    bm = plane.search_batch(None if rank else terms, None, B=2, dim=C.DIM,
                            n_results=10, use_dense=False,
                            term_ops=None if rank else ops)
    if rank == 0:
        torch.save({"ids": fused.ids, "scores": fused.scores,
                    "bm_ids": bm.ids, "bm_scores": bm.scores}, out_file)
    fabric.destroy()


def test_plane_gloo_rank1_honours_rank0_operands(tmp_path):
    import torch.multiprocessing as mp
    out_file = str(tmp_path / "fused")
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_gloo_worker, args=(r, 29547, out_file))
             for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    two = torch.load(out_file, weights_only=True)
    s0, s1, terms, q, ops = _two_rank_shards()
    plane1 = DistributedQueryPlane(s0, Fabric(), k_per_shard=_K2)
    # BM25 alone: documents differ in length, so no two scores tie, and
    # the fused ids equal the 1-rank result position by position
    bm1 = plane1.search_batch(terms, None, B=2, dim=C.DIM, n_results=10,
                              use_dense=False, term_ops=ops)
    assert (bm1.ids >= 0).all() and (bm1.scores[:, :-1]
                                     > bm1.scores[:, 1:]).all()
    assert torch.equal(two["bm_ids"], bm1.ids)
    assert torch.equal(two["bm_scores"], bm1.scores)
    one = plane1.search_batch(
        terms, q, B=2, dim=C.DIM, n_results=_N2, term_ops=ops)
    # With both lists, n_results covers every candidate, so no tie is cut in two. RRF
    # gives the document at rank r of one list and the one at rank r of
    # the other the same fused score, and the sort orders such a pair as
    # it likes: ids are compared as (id, score) sets per row, and in
    # place wherever the fused score differs from both neighbours'.
    assert torch.allclose(two["scores"], one.scores, atol=1e-7)
    for qi in range(2):
        ids1, sc1 = one.ids[qi], one.scores[qi]
        assert (ids1 >= 0).sum() >= _K2
        pairs = [sorted(zip(i[i >= 0].tolist(),
                            s[i >= 0].round(decimals=6).tolist()))
                 for i, s in ((ids1, sc1), (two["ids"][qi], two["scores"][qi]))]
        assert pairs[0] == pairs[1]
        gap = (sc1[:-1] - sc1[1:]) > 1e-7
        untied = torch.ones_like(ids1, dtype=torch.bool)
        untied[:-1] &= gap
        untied[1:] &= gap
        assert untied.sum() >= 5
        assert torch.equal(two["ids"][qi][untied], ids1[untied])
    # and without the operands rank 1's documents do win
    lost = DistributedQueryPlane(s1, Fabric(), k_per_shard=_K2).search_batch(
        terms, q, B=2, dim=C.DIM, n_results=10)
    assert (lost.ids >= 90_000).all()


# ------------------------------------------------------------- FTS path

def _docs():
    return [Document(url="https://a.org/1", title="rust async",
                     text="rust async runtime with tokio and futures"),
            Document(url="https://a.org/2", title="rust and java",
                     text="rust compared with java for backend services"),
            Document(url="https://a.org/3", title="rust basics",
                     text="rust ownership and borrowing for beginners")]


def test_local_store_excludes_terms():
    store = LocalStore()
    for d in _docs():
        store.add_document(d)
    # today the minus is dropped and java is REQUIRED
    assert [h.url for h in store.search("rust -java")] == ["https://a.org/2"]
    got = store.search("rust", exclude_terms=("java",))
    assert sorted(h.url for h in got) == ["https://a.org/1", "https://a.org/3"]
    got = store.search("rust", exclude_terms=("java", "tokio"))
    assert [h.url for h in got] == ["https://a.org/3"]
    got = store.search("rust tokio", match_any=True, exclude_terms=("java",))
    assert sorted(h.url for h in got) == ["https://a.org/1", "https://a.org/3"]
    assert store.search("", exclude_terms=("java",)) == []   # no positive term
    store.close()


def _ctx(flag: bool, with_engine: bool):
    cfg = dataclasses.replace(Config(), gpu=GpuConfig(term_operators=flag))
    c = AppContext.create(config=cfg, with_engine=with_engine,
                          with_worker=False, in_memory=True)
    for d in _docs():
        c.index_document(d, attest=False, credit=False)
    c.flush_engine()
    return c


@pytest.mark.parametrize("with_engine", [False, True], ids=["fts", "engine"])
def test_app_context_flag_off_is_unchanged_and_on_excludes(with_engine):
    assert Config().gpu.term_operators is False
    off = _ctx(False, with_engine)
    try:
        resp = off.search("rust -java", use_cache=False, deduct=False)
        # the Java document is in the result, as it always was
        assert "https://a.org/2" in [h.url for h in resp.results]
    finally:
        off.close()
    on = _ctx(True, with_engine)
    try:
        resp = on.search("rust -java", use_cache=False, deduct=False)
        assert sorted(h.url for h in resp.results) == [
            "https://a.org/1", "https://a.org/3"]
        resp = on.search("rust +tokio", use_cache=False, deduct=False)
        assert [h.url for h in resp.results] == ["https://a.org/1"]
        resp = on.search("rust", use_cache=False, deduct=False)
        assert len(resp.results) == 3
        resp = on.search("-java", use_cache=False, deduct=False)
        assert resp.results == []            # no positive term
        if with_engine:
            too_many = "rust " + " ".join(f"-w{i}" for i in range(17))
            with pytest.raises(ValueError):
                on.search(too_many, use_cache=False, deduct=False)
    finally:
        on.close()


def test_cjk_operator_words_reach_the_engine_whole():
    """The CJK splitter of preprocess_query must not part a sign from
    its word: `-東京都` excludes and `+東京都` requires the run and its
    bigrams, as bm25_term_ids indexes them."""
    from infomesh_amd.search.query import preprocess_query
    assert preprocess_query("rust -東京都", term_operators=True) \
        == "rust -東京都"
    assert preprocess_query("+東京都 the rust -java", term_operators=True) \
        == "rust +東京都 -java"
    assert preprocess_query("-java", term_operators=True) == "-java"
    assert preprocess_query("rust -東京都") \
        == preprocess_query("rust -東京都", term_operators=False)
    cfg = dataclasses.replace(Config(), gpu=GpuConfig(term_operators=True))
    c = AppContext.create(config=cfg, with_engine=True, with_worker=False,
                          in_memory=True)
    try:
        for i, body in enumerate(["rust 東京都 の案内 guide",
                                  "rust 大阪府 の案内 guide",
                                  "rust plain notes guide"], 1):
            c.index_document(Document(url=f"https://a.org/{i}",
                                      title=f"page {i}", text=body),
                             attest=False, credit=False)
        c.flush_engine()
        kw = dict(use_cache=False, deduct=False, mode="hybrid")
        assert len(c.search("rust", **kw).results) == 3
        resp = c.search("rust -東京都", **kw)
        assert sorted(h.url for h in resp.results) == [
            "https://a.org/2", "https://a.org/3"]
        resp = c.search("rust +東京都", **kw)
        assert [h.url for h in resp.results] == ["https://a.org/1"]
        resp = c.search("rust +案内 -大阪府", **kw)
        assert [h.url for h in resp.results] == ["https://a.org/1"]
    finally:
        c.close()


def test_operand_cap_is_the_engine_s_alone():
    """A query that the FTS path serves (a site: filter with gpu.filters
    off) has no operand cap, engine or not."""
    on = _ctx(True, True)
    try:
        many = "rust site:a.org " + " ".join(f"-w{i}" for i in range(17))
        resp = on.search(many, use_cache=False, deduct=False)
        assert len(resp.results) == 3
        with pytest.raises(ValueError):
            on.search(many.replace("site:a.org ", ""), use_cache=False,
                      deduct=False)
    finally:
        on.close()


def test_required_word_collision_is_dropped_at_hydration(monkeypatch):
    """A document that holds only a word colliding with the required one
    in the 2^17-bucket vocabulary passes the shard and is dropped when
    its stored text is read."""
    on = _ctx(True, True)
    try:
        import infomesh_amd.engine as E
        import infomesh_amd.index.gpu_index as G
        real = G.bm25_term_ids
        tokio = int(real("tokio")[0])

        def colliding(text, vocab=G.BM25_VOCAB):
            ids = real(text, vocab)
            if vocab == G.BM25_VOCAB:     # "java" lands in tokio's bucket
                ids = np.where(ids == int(real("java")[0]), tokio, ids)
            return ids
        monkeypatch.setattr(E, "bm25_term_ids", colliding)
        on.engine.add_document(Document(
            url="https://a.org/2", title="rust and java", doc_id=2,
            text="rust compared with java for backend services"))
        on.flush_engine()
        raw = on.engine.search("rust", require=("tokio",))
        assert sorted(h.doc_id for h in raw) == [1, 2]      # the shard's view
        resp = on.search("rust +tokio", use_cache=False, deduct=False)
        assert [h.url for h in resp.results] == ["https://a.org/1"]
    finally:
        on.close()
