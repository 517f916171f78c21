"""Facet counts over the whole match set, without a GPU: the numpy
oracle against a plain loop, the FacetSpec packer, CpuShard against brute
force, the query plane's packing and a 2-rank gloo run, AppContext with
and without an engine, and the /search, MCP and SDK pass-through."""
from __future__ import annotations

import dataclasses
import os

import numpy as np
import pytest
import torch

import term_ops_corpus as C
from facet_cases import brute_counts, corpus_spec
from infomesh_amd.config import Config, GpuConfig
from infomesh_amd.index.doc_attrs import (FACET_MAX_DOMS, FACET_MAX_EDGES,
                                          FACET_MAX_LANGS, DocFilter,
                                          FacetCounts, FacetSpec,
                                          PackedFacets, domain_hash,
                                          facet_results, facet_slots,
                                          facet_width, lang16, pack_attrs,
                                          pack_facets)
from infomesh_amd.index.gpu_index import CpuShard
from infomesh_amd.index.local_store import Document
from infomesh_amd.mcp.handlers import Handlers
from infomesh_amd.ops import reference as R
from infomesh_amd.parallel.fabric import Fabric
from infomesh_amd.parallel.query_plane import DistributedQueryPlane
from infomesh_amd.search.nlp import (parse_facet_token, parse_query_filters,
                                     with_facet_token)
from infomesh_amd.services import AppContext, FacetedHits


def _i32(values) -> torch.Tensor:
    return torch.from_numpy(np.asarray(values, dtype=np.uint32).view(np.int32))


# ------------------------------------------------- oracle vs a plain loop

def _loop_counts(scores, rows, attrs, edges, langs, desc, doms, ok):
    """The rules of the issue, one document at a time."""
    E, L = len(edges), len(langs)
    F = 5 + E + L + max(n for _, n in desc)
    out = np.zeros((len(rows), F), dtype=np.int64)
    for r, b in enumerate(rows):
        off, n = desc[r]
        mine = doms[off:off + n]
        for d in range(scores.shape[1]):
            if not (ok is None or ok[b][d]) or not scores[b, d] > 0:
                continue
            w0, w1, w2 = (int(v) for v in attrs[d][:3])
            out[r, 0] += 1
            if w0 == 0:
                out[r, 1] += 1
            else:
                out[r, 2 + sum(1 for e in edges if e <= w0)] += 1
            c = w1 & 0xFFFF
            if c == 0:
                out[r, 3 + E] += 1
            elif c in langs:
                out[r, 4 + E + langs.index(c)] += 1
            else:
                out[r, 4 + E + L] += 1
            if w2 in mine:
                out[r, 5 + E + L + mine.index(w2)] += 1
    return out


def test_oracle_equals_a_plain_loop_and_the_layout_is_the_documented_one():
    assert facet_slots(3, 2) == {"total": 0, "date_zero": 1, "date0": 2,
                                 "lang_zero": 6, "lang0": 7, "lang_other": 9,
                                 "dom0": 10}
    assert facet_width(3, 2, 4) == 14 and facet_width(0, 0, 0) == 5
    rng = np.random.default_rng(3)
    B, N = 4, 333
    scores = rng.choice(np.asarray([0.0, -0.0, -1.0, 1e-3, 2.5, 1e30],
                                   dtype=np.float32), size=(B, N))
    edges = [100, 200, 200, 0x90000000]
    langs = sorted(lang16(c) for c in ("en", "de", "zh"))
    a = np.zeros((N, 4), dtype=np.uint32)
    a[:, 0] = rng.choice([0, 1, 99, 100, 150, 200, 0x90000000, 0xFFFFFFFF],
                         size=N)
    a[:, 1] = rng.choice([0, lang16("en"), lang16("de"), lang16("fr"),
                          lang16("zh") | (1 << 16)], size=N)
    pool = sorted([5, 77, 0x80000001, 0xFFFFFFF0, 1 << 20])
    a[:, 2] = rng.choice(pool + [123456], size=N)
    doms = pool[:2] + pool + [424242]          # lists of 2, 5 and 1 hashes
    desc = [(0, 2), (2, 5), (7, 1)]
    rows = [3, 0, 3]
    bits = rng.integers(0, 2, size=(2, N)).astype(bool)
    pred = [1, 0, 0, 1]
    W = (N + 63) // 64 * 2
    words = np.zeros((2, W * 32), dtype=bool)
    words[:, :N] = bits
    mask = torch.from_numpy(np.packbits(words, axis=1, bitorder="little")
                            .view(np.uint32).view(np.int32).reshape(2, W))
    args = (torch.from_numpy(scores), torch.tensor(rows, dtype=torch.int32),
            _i32(a), _i32(edges), _i32(langs),
            torch.tensor(desc, dtype=torch.int32), _i32(doms))
    for m, rp, ok in ((None, None, None),
                      (mask, torch.tensor(pred, dtype=torch.int32),
                       [bits[p] for p in pred])):
        got = R.facet_counts(*args, mask=m, row_pred=rp)
        want = _loop_counts(scores, rows, a.tolist(), edges, langs, desc,
                            doms, ok)
        assert got.dtype == torch.int32 and got.shape == want.shape
        assert np.array_equal(got.numpy(), want)
        assert want[:, 0].min() > 0
    # -0.0 and -1.0 never match
    only = torch.tensor([[-0.0, -1.0, 0.0]])
    z = R.facet_counts(only, torch.tensor([0], dtype=torch.int32),
                       _i32(np.ones((3, 4))), _i32([]), _i32([]),
                       torch.zeros((1, 2), dtype=torch.int32), _i32([]))
    assert z.tolist() == [[0, 0, 0, 0, 0]]


# ----------------------------------------------------------------- packer

def test_packer_sorts_dedupes_and_maps_back():
    spec = FacetSpec(date_edges=(300, 100, 300),
                     languages=("fr", "EN", "en"),
                     domains=(("b.org", "A.org", "b.org "), None, ()))
    p = pack_facets(spec, 4)
    assert p.edges == (100, 300)
    assert p.langs == tuple(sorted({lang16("fr"), lang16("en")}))
    assert p.rows == (0, 2)
    assert p.lists == (tuple(sorted({domain_hash("a.org"),
                                     domain_hash("b.org")})), ())
    assert all(0 <= h <= 0xFFFFFFFF for h in p.lists[0])
    assert p.width == facet_width(2, 2, 2)
    rows, edges, langs, desc, doms = p.tables()
    assert rows.tolist() == [0, 2] and desc.tolist() == [[0, 2], [2, 0]]
    assert all(t.dtype == np.int32 for t in (rows, edges, langs, desc, doms))
    assert pack_facets(p, 4) is p                       # passes through
    # counts by slot -> the caller's names and order
    sl = facet_slots(2, 2)
    c = np.zeros((2, p.width), dtype=np.int32)
    c[0, sl["total"]] = 9
    c[0, sl["date_zero"]] = 1
    c[0, sl["date0"]:sl["date0"] + 3] = (2, 3, 3)
    c[0, sl["lang0"] + p.langs.index(lang16("fr"))] = 4
    c[0, sl["lang0"] + p.langs.index(lang16("en"))] = 2
    c[0, sl["lang_zero"]], c[0, sl["lang_other"]] = 1, 2
    c[0, sl["dom0"] + p.lists[0].index(domain_hash("b.org"))] = 5
    c[0, sl["dom0"] + p.lists[0].index(domain_hash("a.org"))] = 3
    got = facet_results(spec, p, c, n_rows=4)
    assert got[1] is None and got[3] is None
    assert got[0] == FacetCounts(
        total=9, date_zero=1, dates=(2, 3, 3),
        languages={"fr": 4, "EN": 2, "en": 2}, language_zero=1,
        language_other=2, domains={"b.org": 5, "A.org": 3, "b.org ": 5})
    assert list(got[0].domains) == ["b.org", "A.org", "b.org "]
    assert got[2].total == 0 and got[2].domains == {}
    # nothing to count
    assert pack_facets(None, 2) is None
    assert pack_facets(FacetSpec(domains=(None, None)), 2) is None


def test_packer_caps_are_value_errors():
    ok = FacetSpec(date_edges=tuple(range(1, FACET_MAX_EDGES + 1)),
                   languages=tuple(f"{a}{b}" for a in "ab"
                                   for b in "abcdefghijklmnop"),
                   domains=(tuple(f"h{i}.org" for i in range(FACET_MAX_DOMS)),))
    p = pack_facets(ok, 1)
    assert (len(p.edges), len(p.langs), len(p.lists[0])) == (7, 32, 64)
    assert (FACET_MAX_EDGES, FACET_MAX_LANGS, FACET_MAX_DOMS) == (7, 32, 64)
    for bad in (dataclasses.replace(ok, date_edges=tuple(range(1, 9))),
                dataclasses.replace(ok, languages=ok.languages + ("zz",)),
                dataclasses.replace(ok, domains=(ok.domains[0] + ("x.org",),))):
        with pytest.raises(ValueError, match="caps"):
            pack_facets(bad, 1)
    with pytest.raises(ValueError):
        pack_facets(FacetSpec(languages=("eng", "e"), domains=((),)), 1)
    with pytest.raises(ValueError):
        pack_facets(FacetSpec(domains=((), ())), 1)     # more lists than rows
    with pytest.raises(ValueError, match="caps"):
        PackedFacets(edges=(), langs=(), rows=(0,),
                     lists=(tuple(range(65)),))


# --------------------------------------------- CpuShard against brute force

@pytest.fixture(scope="module")
def corpus_shard():
    toks, meta, emb = C.corpus()
    return (C.build_shard(CpuShard, toks, meta, emb), meta,
            [set(t.tolist()) for t in toks])


def test_cpu_shard_counts_equal_brute_force(corpus_shard):
    cpu, meta, sets = corpus_shard
    terms, q, filters, ops = C.queries()
    spec = corpus_spec(len(terms))
    plain = cpu.search(terms, q, k=C.K_CMP, filters=filters, term_ops=ops)
    assert plain.facets is None
    got = cpu.search(terms, q, k=C.K_CMP, filters=filters, term_ops=ops,
                     facets=spec)
    for name in ("bm25_scores", "bm25_ids", "dense_scores", "dense_ids"):
        assert torch.equal(getattr(got, name), getattr(plain, name)), name
    p = pack_facets(spec, len(terms))
    assert got.facets.shape == (len(terms), p.width)
    assert got.facets.dtype == torch.int32
    res = facet_results(spec, p, got.facets.numpy())
    for qi in range(len(terms)):
        want = brute_counts(terms, filters, ops, meta, sets, spec, qi)
        assert res[qi] == want, qi
        assert want.domains["absent.example"] == 0
    assert min(r.total for r in res) > 0
    assert any(r.total > C.K_CMP for r in res), "counts go past the hits"
    # only the rows the spec names are counted
    some = dataclasses.replace(spec, domains=(None, spec.domains[1], None))
    part = cpu.search(terms, q, k=C.K_CMP, filters=filters, term_ops=ops,
                      facets=some)
    assert part.facets.shape[0] == 1
    assert facet_results(some, pack_facets(some, 6), part.facets.numpy(),
                         n_rows=6)[1] == res[1]


def test_unmasked_cpu_shard_counts(corpus_shard):
    """No filter, no tombstone, no operand: nothing but score > 0."""
    toks, meta, emb = C.corpus()
    s = CpuShard()
    for i in range(C.N_DOCS):
        s.add_document(C.GID0 + i, toks[i], emb[i],
                       attrs=pack_attrs(*meta[i]))
    s.build()
    terms, q, _, _ = C.queries()
    spec = corpus_spec(len(terms))
    got = s.search(terms, q, k=5, facets=spec)
    res = facet_results(spec, pack_facets(spec, 6), got.facets.numpy())
    sets = [set(t.tolist()) for t in toks]
    for qi, t in enumerate(terms):
        assert res[qi].total == sum(1 for d in sets if set(t.tolist()) & d)
        assert res[qi].total == sum(res[qi].dates) + res[qi].date_zero


# ------------------------------------------------- query plane: two ranks

_HALF = 300


def _half_shard(lo: int, hi: int) -> CpuShard:
    toks, meta, emb = C.corpus()
    s = CpuShard()
    for i in range(lo, hi):
        s.add_document(C.GID0 + i, toks[i], emb[i],
                       attrs=pack_attrs(*meta[i]))
    s.build()
    s.delete([g for g in C.DEAD if lo <= g - C.GID0 < hi])
    return s


class _CountingFabric:
    """Forwards to a Fabric and counts its broadcasts."""

    def __init__(self, fabric):
        self._fabric = fabric
        self.broadcasts = 0

    def broadcast(self, t, src=0):
        self.broadcasts += 1
        return self._fabric.broadcast(t, src)

    def __getattr__(self, name):
        return getattr(self._fabric, name)


def _facet_worker(rank: int, port: int, out_dir: str):
    os.environ["HIP_VISIBLE_DEVICES"] = "-1"
    os.environ["CUDA_VISIBLE_DEVICES"] = "-1"
    assert not torch.cuda.is_available(), "GPUs still visible to the worker"
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": "2",
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    fabric = _CountingFabric(Fabric(backend="gloo"))
    shard = _half_shard(_HALF, C.N_DOCS) if rank else _half_shard(0, _HALF)
    plane = DistributedQueryPlane(shard, fabric, k_per_shard=20)
    terms, q, filters, ops = C.queries()
    filters = [DocFilter(language="de", after=C.T0 + 7)] + filters[1:]
    spec = corpus_spec(len(terms))
    lead = rank == 0
    # the packing alone: what every rank holds after the broadcasts
    seen = plane._broadcast_query(terms if lead else None, 6,
                                  filters if lead else None,
                                  ops if lead else None,
                                  spec if lead else None)
    with_facets = fabric.broadcasts
    fabric.broadcasts = 0
    plain = plane._broadcast_query(terms if lead else None, 6,
                                   filters if lead else None,
                                   ops if lead else None)
    without = fabric.broadcasts
    fused = plane.search_batch(terms if lead else None, q if lead else None,
                               B=6, dim=C.DIM, n_results=10,
                               filters=filters if lead else None,
                               term_ops=ops if lead else None,
                               facets=spec if lead else None)
    none = plane.search_batch(terms if lead else None, q if lead else None,
                              B=6, dim=C.DIM, n_results=10,
                              filters=filters if lead else None,
                              term_ops=ops if lead else None)
    assert (fused is not None) == lead
    torch.save({"filters": seen[1], "facets": seen[3],
                "plain_filters": plain[1], "plain_facets": plain[3],
                "broadcasts": (with_facets, without),
                "counts": fused.facets if lead else None,
                "ids": fused.ids if lead else None,
                "plain_ids": none.ids if lead else None,
                "plain_counts": none.facets if lead else "n/a"},
               os.path.join(out_dir, f"r{rank}"))
    fabric.destroy()


def test_plane_gloo_counts_equal_one_shard_holding_both_halves(tmp_path):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_facet_worker, args=(r, 29553, str(tmp_path)))
             for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    r0, r1 = (torch.load(str(tmp_path / f"r{r}"), weights_only=False)
              for r in range(2))
    terms, q, filters, ops = C.queries()
    filters = [DocFilter(language="de", after=C.T0 + 7)] + filters[1:]
    spec = corpus_spec(len(terms))
    want = pack_facets(spec, 6)
    # every rank holds rank 0's spec, and row 0 keeps its predicate words
    # with and without the facet mark
    assert r0["facets"] == want and r1["facets"] == want
    assert r0["filters"] == r1["filters"] == r0["plain_filters"] \
        == r1["plain_filters"]
    x, y, z, w = r1["filters"][0]
    assert (x, y, w) == (C.T0 + 7, 0xFFFFFFFF, 0) and z == lang16("de")
    assert r0["plain_facets"] is None and r1["plain_facets"] is None
    # the spec costs two broadcasts, and only a batch that has one
    assert r0["broadcasts"] == r1["broadcasts"]
    assert r0["broadcasts"][0] == r0["broadcasts"][1] + 2
    assert r0["plain_counts"] is None
    assert torch.equal(r0["ids"], r0["plain_ids"])
    # counts: the two halves sum to what one shard holding both counts
    whole = _half_shard(0, C.N_DOCS)
    one = DistributedQueryPlane(whole, Fabric(), k_per_shard=20).search_batch(
        terms, q, B=6, dim=C.DIM, n_results=10, filters=filters,
        term_ops=ops, facets=spec)
    assert one.facets.dtype == torch.int32
    assert torch.equal(r0["counts"], one.facets.cpu())
    assert int(one.facets[:, 0].min()) > 0
    halves = [_half_shard(0, _HALF).search(terms, q, k=20, filters=filters,
                                           term_ops=ops, facets=spec).facets,
              _half_shard(_HALF, C.N_DOCS).search(
                  terms, q, k=20, filters=filters, term_ops=ops,
                  facets=spec).facets]
    assert all(int(h[:, 0].sum()) > 0 for h in halves), "both halves count"
    assert torch.equal(halves[0] + halves[1], one.facets.cpu())


# ---------------------------------------------------------------- serving

def test_facet_token_round_trip():
    q = with_facet_token("rust async", ["B.org", "a.org", "b.org", " "])
    assert q == "rust async facets:@b.org,a.org"
    assert parse_facet_token(q) == ("rust async", ("b.org", "a.org"))
    assert parse_facet_token(with_facet_token("rust")) == ("rust", ())
    assert parse_facet_token("rust async") == ("rust async", None)
    assert parse_facet_token("about facets: and x:facets:@y") == (
        "about facets: and x:facets:@y", None)
    # it rides beside the filter tokens and leaves them alone
    both = with_facet_token("rust site:a.org,b.org after:@5", ["c.org"])
    text, doms = parse_facet_token(both)
    assert doms == ("c.org",)
    pq = parse_query_filters(text)
    assert pq.text == "rust" and pq.sites == ("a.org", "b.org")
    assert parse_query_filters(both).sites == ("a.org", "b.org")


def _ctx(engine: bool, filters: bool = True):
    cfg = dataclasses.replace(Config(), gpu=GpuConfig(filters=filters))
    c = AppContext.create(config=cfg, with_engine=engine, with_worker=False,
                          in_memory=True)
    import time
    now = time.time()
    ages = {"today": 0.2, "this_week": 3, "this_month": 20, "this_year": 200,
            "older": 500}
    labels = list(ages)
    for i in range(40):
        c.index_document(Document(
            url=f"https://{'big.com' if i % 4 else 'rare.org'}/p{i}",
            title=f"zebra page {i}",
            text="zebra stripes " + " ".join(f"w{i}x{j}" for j in range(i)),
            language=("en", "de", "")[i % 3],
            crawled_at=now - ages[labels[i % 5]] * 86400),
            attest=False, credit=False)
    for i in range(5):
        c.index_document(Document(
            url=f"https://other.net/p{i}", title=f"lion page {i}",
            text=f"lion mane savanna n{i}", language="en"),
            attest=False, credit=False)
    if engine:
        c.flush_engine()
    return c


def test_app_context_engine_counts_every_match():
    c = _ctx(True)
    try:
        plain = c.search("zebra", limit=5, deduct=False)
        assert plain.total_matches is None and plain.facets is None
        resp = c.search("zebra", limit=5, deduct=False, facets=True,
                        facet_domains=["rare.org", "big.com", "nowhere.io"])
        assert resp is not plain, "the cache must keep the two apart"
        assert [h.doc_id for h in resp.results] \
            == [h.doc_id for h in plain.results]
        assert resp.total_candidates == 5 and resp.total_matches == 40
        f = resp.facets
        assert set(f) == {"scope", "domains", "languages", "date_ranges"}
        assert f["scope"] == "matches"
        assert f["domains"] == {"rare.org": 10, "big.com": 30,
                                "nowhere.io": 0}
        assert list(f["domains"]) == ["rare.org", "big.com", "nowhere.io"]
        assert f["date_ranges"] == {"older": 8, "this_year": 8,
                                    "this_month": 8, "this_week": 8,
                                    "today": 8, "unknown": 0}
        assert f["languages"]["en"] == 14 and f["languages"]["de"] == 13
        assert f["languages"]["unknown"] == 13 and f["languages"]["other"] == 0
        assert sum(f["languages"].values()) == 40
        # both are cached, each under its own key
        assert c.search("zebra", limit=5, deduct=False) is plain
        assert c.search("zebra", limit=5, deduct=False, facets=True,
                        facet_domains=["rare.org", "big.com",
                                       "nowhere.io"]) is resp
        other = c.search("zebra", limit=5, deduct=False, facets=True)
        assert other is not resp and other.facets["domains"] == {}
        assert other.total_matches == 40
        # a filter narrows the match set, on the engine (gpu.filters)
        de = c.search("zebra lang:de", limit=5, deduct=False, facets=True,
                      facet_domains=["rare.org"])
        assert de.total_matches == 13 and de.facets["scope"] == "matches"
        assert de.facets["languages"]["de"] == 13
        assert de.facets["languages"]["en"] == 0
        assert de.facets["domains"] == {"rare.org": 3}     # i in 4, 16, 28
        with pytest.raises(ValueError, match="64"):
            c.search("zebra", deduct=False, facets=True,
                     facet_domains=[f"h{i}.org" for i in range(65)])
    finally:
        c.close()


def test_plain_request_is_unchanged_in_a_batch_with_a_facet_request():
    c = _ctx(True)
    try:
        def key(hits):
            return [(h.doc_id, h.url, h.title, h.snippet) for h in hits]
        alone = c._batch_execute(["zebra", "lion"], 10)
        assert all(type(r) is list for r in alone)
        mixed = c._batch_execute(
            ["zebra", with_facet_token("zebra", ["rare.org"]), "lion",
             with_facet_token("lion")], 10)
        assert type(mixed[0]) is list and type(mixed[2]) is list
        assert key(mixed[0]) == key(alone[0])
        assert key(mixed[2]) == key(alone[1])
        assert [h.score for h in mixed[0]] == pytest.approx(
            [h.score for h in alone[0]], abs=5e-6, rel=0)
        assert isinstance(mixed[1], FacetedHits)
        assert key(mixed[1].hits) == key(alone[0])
        assert mixed[1].counts.total == 40
        assert mixed[1].counts.domains == {"rare.org": 10}
        assert mixed[3].counts.total == 5 and mixed[3].counts.domains == {}
        # through the batcher as well: the facet and the plain request of
        # one batch each get their own kind of result
        out = _in_one_batch(c, {
            "plain": lambda: c.search("zebra", limit=5, deduct=False,
                                      use_cache=False),
            "facets": lambda: c.search("zebra", limit=5, deduct=False,
                                       use_cache=False, facets=True,
                                       facet_domains=["rare.org"])})
        assert out["plain"].facets is None
        assert out["plain"].total_matches is None
        assert out["facets"].total_matches == 40
        assert key(out["plain"].results) == key(out["facets"].results) \
            == key(alone[0][:5])
    finally:
        c.close()


def _in_one_batch(c, calls: dict) -> dict:
    """Run the calls on a thread each so that they share ONE batch: the
    batcher is told to fire when all of them have arrived (max_batch),
    not after a wait, so no timing decides what the batch holds. A
    call's exception is its result."""
    import threading
    c.ensure_batcher()
    saved = c.batcher.max_batch, c.batcher.max_wait_s
    c.batcher.max_batch = len(calls)
    c.batcher.max_wait_s = 60.0          # never reached: the batch fills
    out = {}

    def run(name, fn):
        try:
            out[name] = fn()
        except BaseException as e:       # noqa: BLE001 (handed to the test)
            out[name] = e
    ts = [threading.Thread(target=run, args=item) for item in calls.items()]
    before = c.batcher.stats()["batches"]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    c.batcher.max_batch, c.batcher.max_wait_s = saved
    assert c.batcher.stats()["batches"] == before + 1, "one batch"
    assert c.batcher.stats()["max_batch_seen"] >= len(calls)
    return out


def test_a_typed_facet_token_cannot_fail_or_burden_its_batch():
    """The token is the serving path's own syntax. Typed into a query it
    must not raise for anybody, must not run the count kernel, and must
    not stay in the effective query."""
    c = _ctx(True)
    try:
        def key(hits):
            return [(h.doc_id, h.url, h.title) for h in hits]
        over = "zebra facets:@" + ",".join(f"h{i}.org" for i in range(70))
        under = "zebra facets:@rare.org"
        alone = c._batch_execute(["zebra"], 5)[0]
        assert len(alone) == 5
        calls = []
        real = c.engine.search_with_facets
        c.engine.search_with_facets = lambda *a, **kw: (
            calls.append(1), real(*a, **kw))[1]
        # AppContext.search drops a typed token on the caller's thread
        out = _in_one_batch(c, {
            "plain": lambda: c.search("zebra", limit=5, deduct=False,
                                      use_cache=False),
            "over": lambda: c.search(over, limit=5, deduct=False,
                                     use_cache=False),
            "under": lambda: c.search(under, limit=5, deduct=False,
                                      use_cache=False)})
        for name, resp in out.items():
            assert not isinstance(resp, BaseException), (name, resp)
            assert resp.facets is None and resp.total_matches is None
            assert "facets:" not in resp.effective_query
            assert key(resp.results) == key(alone), name
        assert calls == [], "a typed token launched the count kernel"
        # the cap still holds for the parameter, on the caller alone
        out = _in_one_batch(c, {
            "plain": lambda: c.search("zebra", limit=5, deduct=False,
                                      use_cache=False),
            "asks": lambda: c.search("zebra", limit=5, deduct=False,
                                     use_cache=False, facets=True,
                                     facet_domains=["rare.org"])})
        assert key(out["plain"].results) == key(alone)
        assert out["asks"].facets["domains"] == {"rare.org": 10}
        with pytest.raises(ValueError, match="64"):
            c.search("zebra", deduct=False, facets=True,
                     facet_domains=[f"h{i}.org" for i in range(65)])
        # past AppContext.search (a direct submit): the executor cuts an
        # over-cap list, it never raises into the shared batch
        calls.clear()
        out = _in_one_batch(c, {
            "plain": lambda: c.batcher.submit("zebra", 5),
            "over": lambda: c.batcher.submit(over, 5)})
        assert type(out["plain"]) is list and key(out["plain"]) == key(alone)
        assert isinstance(out["over"], FacetedHits)
        assert key(out["over"].hits[:5]) == key(alone)
        assert list(out["over"].counts.domains) == [
            f"h{i}.org" for i in range(64)]
        assert out["over"].counts.total == 40
        both = c._batch_execute(["zebra", over], 5)
        assert key(both[0]) == key(alone) and both[1].counts.total == 40
        # and _engine_search itself writes only its own token
        resp = c._engine_search(over, 5, "auto")
        assert resp.facets is None and "facets:" not in resp.effective_query
        assert key(resp.results) == key(alone)
    finally:
        c.close()


def test_web_search_over_the_list_cap_answers_no_facets():
    """Past the cap the handler searches without the lists and filters
    the hits: counts over the unfiltered match set are not theirs."""
    c = _ctx(True)
    try:
        many = [f"host{i}.example" for i in range(2100)]
        c.store.domains_matching = lambda names: list(names)
        out = Handlers(c).web_search(query="zebra", limit=5,
                                     domain_blocklist=many, facets=True,
                                     facet_domains=["rare.org"])
        assert len(out["results"]) == 5
        assert out["total_matches"] is None and out["facets"] is None
    finally:
        c.close()


def test_app_context_without_engine_counts_the_results():
    c = _ctx(False)
    try:
        plain = c.search("zebra", limit=5, deduct=False)
        assert plain.facets is None and plain.total_matches is None
        resp = c.search("zebra", limit=5, deduct=False, facets=True,
                        facet_domains=["rare.org"])
        assert resp is not plain
        assert resp.total_matches is None
        assert set(resp.facets) == {"scope", "domains", "languages",
                                    "date_ranges"}
        assert resp.facets["scope"] == "results"
        assert sum(resp.facets["domains"].values()) == len(resp.results) == 5
    finally:
        c.close()
    c = _ctx(True)
    try:                        # mode="local" is FTS even with an engine
        resp = c.search("zebra", limit=5, mode="local", deduct=False,
                        facets=True)
        assert resp.facets["scope"] == "results"
        assert resp.total_matches is None
    finally:
        c.close()


def test_http_route_mcp_tool_and_sdk_pass_the_parameters_through():
    import asyncio

    import httpx
    from fastapi.testclient import TestClient

    from infomesh_amd.api.local_api import create_app
    from infomesh_amd.mcp.tools import TOOLS
    from infomesh_amd.sdk.client import AsyncInfoMeshClient, InfoMeshClient
    c = _ctx(True)
    try:
        http = TestClient(create_app(c))
        plain = http.get("/search", params={"q": "zebra", "limit": 5}).json()
        assert "facets" not in plain and "total_matches" not in plain
        body = http.get("/search", params={
            "q": "zebra", "limit": 5, "facets": 1,
            "facet_domains": "rare.org,big.com"}).json()
        assert body["results"] == plain["results"]
        assert body["total_matches"] == 40
        assert body["facets"]["scope"] == "matches"
        assert body["facets"]["domains"] == {"rare.org": 10, "big.com": 30}
        r = http.get("/search", params={
            "q": "zebra", "facets": 1,
            "facet_domains": ",".join(f"h{i}.org" for i in range(65))})
        assert r.status_code == 400
        # MCP tool
        props = next(t for t in TOOLS if t["name"] == "web_search")[
            "inputSchema"]["properties"]
        assert props["facets"]["type"] == "boolean"
        assert props["facet_domains"]["type"] == "array"
        h = Handlers(c)
        out = h.web_search(query="zebra", limit=5)
        assert "facets" not in out and "total_matches" not in out
        out = h.web_search(query="zebra", limit=5, facets=True,
                           facet_domains=["rare.org"])
        assert out["total_matches"] == 40
        assert out["facets"]["domains"] == {"rare.org": 10}
        # both SDK clients, against the same app
        seen = []

        def handler(request: httpx.Request) -> httpx.Response:
            seen.append(dict(request.url.params))
            r = http.get("/search", params=dict(request.url.params))
            return httpx.Response(r.status_code, json=r.json())
        sdk = InfoMeshClient(transport=httpx.MockTransport(handler))
        assert sdk.search("zebra", limit=5) == plain["results"]
        assert "facets" not in seen[-1]
        got = sdk.search("zebra", limit=5, facets=True,
                         facet_domains=["rare.org", "big.com"])
        assert seen[-1]["facets"] == "1"
        assert seen[-1]["facet_domains"] == "rare.org,big.com"
        assert got["total_matches"] == 40
        assert got["results"] == plain["results"]
        assert got["facets"]["domains"] == {"rare.org": 10, "big.com": 30}
        sdk.close()

        async def _async():
            a = AsyncInfoMeshClient(transport=httpx.MockTransport(handler))
            try:
                return await a.search("zebra", limit=5, facets=True,
                                      facet_domains=["rare.org"])
            finally:
                await a.close()
        got = asyncio.run(_async())
        assert got["total_matches"] == 40
        assert got["facets"]["domains"] == {"rare.org": 10}
    finally:
        c.close()
