"""CPU tests for the top domains of the whole match set: the numpy
oracle against a plain loop, the packer, CpuShard against brute force, a
2-rank gloo run of the query plane's two rounds (exact, inexact and a
mixed batch), AppContext with and without an engine, and the entry
points."""
from __future__ import annotations

import dataclasses
import os
from collections import Counter

import numpy as np
import pytest
import torch

import term_ops_corpus as C
from facet_cases import corpus_spec
from infomesh_amd.config import Config, GpuConfig
from infomesh_amd.index.doc_attrs import (TOP_DOMAINS_MAX, TOP_FETCH,
                                          FacetCounts, FacetSpec,
                                          PackedFacets, domain_hash,
                                          domain_tables_np, domain_top_np,
                                          facet_results, pack_attrs,
                                          pack_facets)
from infomesh_amd.index.gpu_index import CpuShard
from infomesh_amd.index.local_store import Document
from infomesh_amd.mcp.handlers import Handlers
from infomesh_amd.ops import reference as R
from infomesh_amd.parallel.fabric import Fabric
from infomesh_amd.parallel.query_plane import (DistributedQueryPlane,
                                               rank_top_domains)
from infomesh_amd.search.cache import QueryCache
from infomesh_amd.search.nlp import (parse_facet_request, parse_facet_token,
                                     with_facet_request, with_facet_token)
from infomesh_amd.services import AppContext, FacetedHits


# ------------------------------------------------------------ the oracle

def _loop_top(scores, fail, w2, b, K):
    """Row b, document by document, with a Counter."""
    tally = Counter()
    for d in range(scores.shape[1]):
        if scores[b, d] > 0 and not (fail is not None and fail[b, d]):
            tally[int(w2[d])] += 1
    order = sorted(tally, key=lambda h: (-tally[h], h))[:K]
    return [(h, tally[h]) for h in order]


def test_oracle_equals_a_plain_loop():
    rng = np.random.default_rng(3)
    N, B = 900, 3
    pool = np.asarray([0, 5, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE,
                       0xFFFFFFFF, 77, 78, 79], dtype=np.uint32)
    attrs = np.zeros((N, 4), dtype=np.uint32)
    attrs[:, 2] = rng.choice(pool, size=N)
    # 77, 78, 79 and two hashes above 2^31 tie: the hash decides
    attrs[:40, 2] = np.repeat(pool[[7, 8, 9, 3, 6]], 8)
    scores = rng.choice(np.asarray([0.0, -0.0, -1.0, 0.5], dtype=np.float32),
                        size=(B, N))
    scores[:, :40] = 1.0
    scores[1, 40:] = 0.0                      # row 1: the five tied alone
    fail = rng.random((B, N)) < 0.3
    fail[:, :40] = False
    for f in (None, fail):
        for K in (1, 4, 10, 65):
            got = domain_top_np(scores, f, attrs.view(np.int32), [2, 1], K)
            assert got.dtype == np.int32 and got.shape == (2, K, 2)
            for r, b in enumerate([2, 1]):
                want = _loop_top(scores, f, attrs[:, 2], b, K)
                pairs = got[r].view(np.uint32)[:len(want)]
                assert [tuple(int(v) for v in p) for p in pairs] == want
                assert not got[r, len(want):].any()
    five = domain_top_np(scores, None, attrs.view(np.int32), [1], 5)[0]
    assert five.view(np.uint32)[:, 0].tolist() \
        == [77, 78, 79, 0x80000000, 0xFFFFFFFF]
    assert (five[:, 1] == 8).all()
    # the tables: keys ascending as unsigned, ids index them
    keys, ids = domain_tables_np(attrs.view(np.int32))
    assert keys.dtype == np.int32 and ids.dtype == np.int32
    assert keys.view(np.uint32).tolist() == sorted(pool.tolist())
    assert np.array_equal(keys.view(np.uint32)[ids], attrs[:, 2])
    # the kernels' oracles agree with it: count, then select
    s, a = torch.from_numpy(scores), torch.from_numpy(attrs.view(np.int32))
    rows = torch.tensor([2, 1], dtype=torch.int32)
    cnt = R.domain_count(s, rows, torch.from_numpy(ids), len(keys))
    assert cnt.sum(1).tolist() == [int((scores[b] > 0).sum()) for b in (2, 1)]
    sel = R.domain_select(cnt, torch.from_numpy(keys), 65)
    assert torch.equal(sel, R.domain_top(s, rows, a, 65))
    assert np.array_equal(sel.numpy(), domain_top_np(
        scores, None, attrs.view(np.int32), [2, 1], 65))


# ------------------------------------------------------------ the packer

def test_packer_maps_top_rows_back():
    spec = FacetSpec(domains=(None, ("b.org", "a.org"), (), None, ()),
                     top_domains=(0, 5, 0, 0, 32))
    p = pack_facets(spec, 8)
    assert p.rows == (1, 2, 4) and p.top == (5, 0, 32)
    assert p.top_rows == (1, 4)
    assert pack_facets(p, 8) is p
    # a spec without top rows packs as it always did
    plain = pack_facets(FacetSpec(domains=spec.domains), 8)
    assert plain.top == () and plain.top_rows == ()
    assert plain == PackedFacets(edges=(), langs=(), rows=p.rows,
                                 lists=p.lists)
    assert pack_facets(FacetSpec(domains=((),), top_domains=(0,)), 1).top == ()
    # back to the caller's rows, cut to each row's T
    ha, hb, hc = (domain_hash(d) for d in ("a.org", "b.org", "c.org"))
    counts = np.zeros((3, p.width), dtype=np.int32)
    counts[:, 0] = (9, 4, 7)
    long = tuple((h, 40 - h) for h in range(40))
    res = facet_results(spec, p, counts, top=[
        (((hc, 5), (ha, 3), (hb, 1)), False, 4), (long, True, 0)])
    assert res[0] is None and res[3] is None
    assert res[1].total == 9 and res[1].top_domains == ((hc, 5), (ha, 3),
                                                        (hb, 1))
    assert (res[1].top_domains_exact, res[1].top_domains_bound) == (False, 4)
    assert res[2].top_domains is None and res[2].top_domains_exact
    assert res[4].top_domains == long[:32] and res[4].top_domains_bound == 0
    # the new fields have defaults: old constructors and == keep working
    old = FacetCounts(total=4, date_zero=0, dates=(0,), languages={},
                      language_zero=0, language_other=0, domains={})
    assert res[2] == old and old.top_domains is None


def test_packer_refuses_what_it_cannot_count():
    with pytest.raises(ValueError, match=str(TOP_DOMAINS_MAX)):
        pack_facets(FacetSpec(domains=((),), top_domains=(33,)), 2)
    with pytest.raises(ValueError, match="top domains"):
        pack_facets(FacetSpec(domains=((),), top_domains=(-1,)), 2)
    with pytest.raises(ValueError, match="not a counted row"):
        pack_facets(FacetSpec(domains=((), None), top_domains=(1, 1)), 2)
    with pytest.raises(ValueError, match="not a counted row"):
        pack_facets(FacetSpec(domains=((),), top_domains=(1, 1)), 2)
    with pytest.raises(ValueError, match="more top-domain"):
        pack_facets(FacetSpec(domains=((),), top_domains=(1, 0, 0)), 2)
    with pytest.raises(ValueError):
        PackedFacets(edges=(), langs=(), rows=(0,), lists=((),), top=(33,))
    assert pack_facets(FacetSpec(domains=((),), top_domains=(32,)),
                       1).top == (32,)
    # a T behind the last counted row that asks for nothing is fine
    assert pack_facets(FacetSpec(domains=((),), top_domains=(1, 0)), 2).top \
        == (1,)


# --------------------------------------------------------------- CpuShard

@pytest.fixture(scope="module")
def corpus_shard():
    toks, meta, emb = C.corpus()
    return (C.build_shard(CpuShard, toks, meta, emb), meta,
            [set(t.tolist()) for t in toks])


def _top_spec(n_rows: int, T: int = 3) -> FacetSpec:
    base = corpus_spec(n_rows)
    return FacetSpec(date_edges=base.date_edges, languages=base.languages,
                     domains=base.domains,
                     top_domains=tuple(T if i != 1 else 0
                                       for i in range(n_rows)))


def _brute_top(terms, filters, ops, meta, sets, qi, K):
    tally = Counter()
    for i in range(C.N_DOCS):
        if C.passes(C.GID0 + i, meta, filters[qi], ops[qi], sets) \
                and set(terms[qi].tolist()) & sets[i]:
            tally[domain_hash(meta[i][1])] += 1
    order = sorted(tally, key=lambda h: (-tally[h], h))[:K]
    return [(h, tally[h]) for h in order]


def test_cpu_shard_top_domains_equal_brute_force(corpus_shard):
    shard, meta, sets = corpus_shard
    terms, q, filters, ops = C.queries()
    spec = _top_spec(len(terms))
    k = C.K_CMP
    plain = shard.search(terms, q, k=k, filters=filters, term_ops=ops)
    listed = shard.search(terms, q, k=k, filters=filters, term_ops=ops,
                          facets=corpus_spec(len(terms)))
    got = shard.search(terms, q, k=k, filters=filters, term_ops=ops,
                       facets=spec)
    assert plain.dom_top is None and listed.dom_top is None
    assert listed.dom_tally is None
    assert torch.equal(got.facets, listed.facets)
    assert torch.equal(got.bm25_ids, plain.bm25_ids)
    top_rows = [0, 2, 3, 4, 5]
    assert got.dom_top.shape == (5, TOP_FETCH + 1, 2)
    some = 0
    for r, qi in enumerate(top_rows):
        want = _brute_top(terms, filters, ops, meta, sets, qi, TOP_FETCH + 1)
        pairs = got.dom_top[r].numpy().view(np.uint32)
        assert [tuple(int(v) for v in p) for p in pairs[:len(want)]] == want
        assert not got.dom_top[r, len(want):].any()
        some += len(want)
        # the tally answers for every hash, held or not
        ask = torch.tensor([[h for h, _ in want] + [0x55555555]],
                           dtype=torch.int64).repeat(5, 1)
        look = got.dom_tally.lookup(ask)
        assert look[r].tolist() == [n for _, n in want] + [0]
    assert some >= 10
    # through the plane (one rank): FacetCounts with the three fields
    fused = DistributedQueryPlane(shard, Fabric(), k_per_shard=k).search_batch(
        terms, q, B=len(terms), dim=C.DIM, filters=filters, term_ops=ops,
        facets=spec)
    res = facet_results(spec, pack_facets(spec, len(terms)),
                        fused.facets.cpu().numpy(), top=fused.top_domains)
    assert res[1].top_domains is None
    for qi in top_rows:
        want = _brute_top(terms, filters, ops, meta, sets, qi, 3)
        assert list(res[qi].top_domains) == want
        assert res[qi].top_domains_exact and res[qi].top_domains_bound == 0
    # a delete keeps the per-epoch tables, an append builds new ones
    tables = shard._dom_tables
    assert tables is not None
    extra = shard.merged_with([np.asarray([1, 2])], [99],
                              torch.ones(1, C.DIM).bfloat16(),
                              attrs=[pack_attrs("en", "new.example", 5.0)])
    assert extra._dom_tables is None and shard._dom_tables is tables
    assert len(extra._domain_tables()[0]) == len(tables[0]) + 1
    assert extra.hbm_bytes() > 0


def test_rank_top_domains_says_when_it_cannot_know():
    pad = 1 << 32
    union = torch.tensor([[5, 9, 11, pad]])
    total = torch.tensor([[7, 7, 3, 0]])
    for W, cut, T, exact, pairs in (
            (2, 0, 2, True, ((5, 7), (9, 7))),      # everything reported
            (2, 6, 2, True, ((5, 7), (9, 7))),      # 7 > 6
            (2, 7, 2, False, ((5, 7), (9, 7))),     # a hidden 7 could tie
            (2, 3, 3, False, ((5, 7), (9, 7), (11, 3))),
            (1, 9, 3, True, ((5, 7), (9, 7), (11, 3))),   # one shard
            (2, 1, 4, False, ((5, 7), (9, 7), (11, 3))),  # fewer than T
            (2, 0, 4, True, ((5, 7), (9, 7), (11, 3)))):
        got = rank_top_domains(union, total, torch.tensor([cut]), W, [T])
        assert got == [(pairs, exact, cut)], (W, cut, T)


# ------------------------------------------------------------ 2-rank gloo

_HALF = 300
_ADV_TERM = 7
_ADV_T = 3


def _half_shard(lo: int, hi: int) -> CpuShard:
    toks, meta, emb = C.corpus()
    s = CpuShard()
    for i in range(lo, hi):
        s.add_document(C.GID0 + i, toks[i], emb[i],
                       attrs=pack_attrs(*meta[i]))
    s.build()
    s.delete([g for g in C.DEAD if lo <= g - C.GID0 < hi])
    return s


def _adversarial_docs(rank: int) -> list[str]:
    """One domain per document, 66 domains per shard: 64 of the shard's
    own with 10 documents each, "both.example" with 9 (rank 65 on either
    shard, 18 = the global maximum) and a straggler with 1."""
    own = [f"s{rank}d{j}.example" for j in range(64)]
    return [d for d in own for _ in range(10)] + ["both.example"] * 9 \
        + [f"last{rank}.example"]


def _adversarial_shard(ranks) -> CpuShard:
    s = CpuShard()
    gid = 0
    for rank in ranks:
        for j, dom in enumerate(_adversarial_docs(rank)):
            # every document holds the term; lengths differ
            s.add_document(rank * 10_000 + j,
                           np.asarray([_ADV_TERM] + [900 + j % 7] * (j % 5)),
                           None, attrs=pack_attrs("en", dom, 100.0))
            gid += 1
    s.build()
    return s


class _CountingFabric:
    """Forwards to a Fabric and counts its collectives."""

    def __init__(self, fabric):
        self._fabric = fabric
        self.broadcasts = self.gathers = 0

    def broadcast(self, t, src=0):
        self.broadcasts += 1
        return self._fabric.broadcast(t, src)

    def all_gather(self, t):
        self.gathers += 1
        return self._fabric.all_gather(t)

    def __getattr__(self, name):
        return getattr(self._fabric, name)


def _mixed_spec() -> FacetSpec:
    """Row 0 asks for top domains, row 1 for listed ones only, the rest
    for nothing."""
    return FacetSpec(languages=("de",), domains=((), ("a.org", "c.org")),
                     top_domains=(3,))


def _worker(rank: int, port: int, out_dir: str):
    os.environ["HIP_VISIBLE_DEVICES"] = "-1"
    os.environ["CUDA_VISIBLE_DEVICES"] = "-1"
    assert not torch.cuda.is_available(), "GPUs still visible to the worker"
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": "2",
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    fabric = _CountingFabric(Fabric(backend="gloo"))
    lead = rank == 0
    terms, q, filters, ops = C.queries()
    shard = _half_shard(_HALF, C.N_DOCS) if rank else _half_shard(0, _HALF)
    plane = DistributedQueryPlane(shard, fabric, k_per_shard=20)

    def run(spec):
        fabric.broadcasts = fabric.gathers = 0
        fused = plane.search_batch(
            terms if lead else None, q if lead else None, B=6, dim=C.DIM,
            n_results=10, filters=filters if lead else None,
            term_ops=ops if lead else None, facets=spec if lead else None)
        assert (fused is not None) == lead
        return fused, (fabric.broadcasts, fabric.gathers)
    seen = plane._broadcast_query(terms if lead else None, 6,
                                  filters if lead else None,
                                  ops if lead else None,
                                  _top_spec(6) if lead else None)[3]
    top, n_top = run(_top_spec(6))
    listed, n_listed = run(corpus_spec(6))
    mixed, n_mixed = run(_mixed_spec())
    plain, n_plain = run(None)
    # (b) the adversarial corpus, one more plane over the same fabric
    adv_plane = DistributedQueryPlane(_adversarial_shard([rank]), fabric,
                                      k_per_shard=10)
    adv = adv_plane.search_batch(
        [np.asarray([_ADV_TERM])] if lead else None, None, B=1, dim=C.DIM,
        n_results=5, use_dense=False,
        facets=FacetSpec(domains=((),), top_domains=(_ADV_T,))
        if lead else None)

    def pick(f):
        return None if f is None else {
            "ids": f.ids, "scores": f.scores, "facets": f.facets,
            "top": f.top_domains}
    torch.save({"seen": seen, "top": pick(top), "listed": pick(listed),
                "mixed": pick(mixed), "plain": pick(plain), "adv": pick(adv),
                "collectives": (n_top, n_listed, n_mixed, n_plain)},
               os.path.join(out_dir, f"r{rank}"))
    fabric.destroy()


@pytest.fixture(scope="module")
def gloo_run(tmp_path_factory):
    import torch.multiprocessing as mp
    out = tmp_path_factory.mktemp("topdom")
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, 29567, str(out)))
             for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return [torch.load(str(out / f"r{r}"), weights_only=False)
            for r in range(2)]


def test_gloo_top_domains_equal_one_shard_holding_both_halves(gloo_run):
    r0, r1 = gloo_run
    terms, q, filters, ops = C.queries()
    spec = _top_spec(6)
    # every rank holds rank 0's spec, the T of every counted row included
    assert r0["seen"] == r1["seen"] == pack_facets(spec, 6)
    assert r1["seen"].top == (3, 0, 3, 3, 3, 3)
    whole = _half_shard(0, C.N_DOCS)
    one = DistributedQueryPlane(whole, Fabric(), k_per_shard=20).search_batch(
        terms, q, B=6, dim=C.DIM, n_results=10, filters=filters,
        term_ops=ops, facets=spec)
    # the single-shard oracle: the whole corpus' own first domains
    single = whole.search(terms, q, k=20, filters=filters, term_ops=ops,
                          facets=spec).dom_top.numpy().view(np.uint32)
    assert len(r0["top"]["top"]) == 5
    for r, (pairs, exact, bound) in enumerate(r0["top"]["top"]):
        n = int((single[r, :, 1] > 0).sum())
        want = tuple((int(h), int(c)) for h, c in single[r, :min(n, 3)])
        assert pairs == want and exact is True and bound == 0
        assert one.top_domains[r] == (want, True, 0)
    assert sum(len(p) for p, _, _ in r0["top"]["top"]) >= 12
    assert torch.equal(r0["top"]["facets"], one.facets.cpu())
    assert torch.equal(r0["top"]["facets"], r0["listed"]["facets"])
    # the spec's broadcasts stay two; the top rows cost two more gathers,
    # and only a batch that has one
    (b_top, g_top), (b_listed, g_listed), (b_mixed, g_mixed), \
        (b_plain, g_plain) = r0["collectives"]
    assert r0["collectives"] == r1["collectives"]
    assert b_top == b_listed == b_mixed == b_plain + 2
    assert g_listed == g_plain + 1
    assert g_top == g_mixed == g_listed + 2
    assert r0["listed"]["top"] is None and r0["plain"]["top"] is None


def test_gloo_adversarial_corpus_is_reported_inexact(gloo_run):
    r0, _ = gloo_run
    (pairs, exact, bound), = r0["adv"]["top"]
    # each shard's cut-off is both.example's 9 documents
    assert exact is False and bound == 18
    # what is returned is counted exactly: 10 documents each, the three
    # smallest hashes of the 128 reported domains
    tens = sorted(domain_hash(f"s{r}d{j}.example")
                  for r in range(2) for j in range(64))
    assert pairs == tuple((h, 10) for h in tens[:_ADV_T])
    # and one shard holding both halves knows better
    whole = _adversarial_shard([0, 1])
    one = DistributedQueryPlane(whole, Fabric(), k_per_shard=10).search_batch(
        [np.asarray([_ADV_TERM])], None, B=1, dim=C.DIM, n_results=5,
        use_dense=False,
        facets=FacetSpec(domains=((),), top_domains=(_ADV_T,)))
    (truth, exact, bound), = one.top_domains
    assert exact is True
    assert truth[0] == (domain_hash("both.example"), 18)
    assert truth[1:] == pairs[:_ADV_T - 1]
    assert int(r0["adv"]["facets"][0, 0]) == 2 * 650 == int(one.facets[0, 0])


def test_gloo_mixed_batch_leaves_the_plain_rows_alone(gloo_run):
    r0, _ = gloo_run
    mixed, plain, top = r0["mixed"], r0["plain"], r0["top"]
    assert plain["facets"] is None
    # bit for bit, every row: the top row, the listed row, the plain rows
    assert torch.equal(mixed["ids"], plain["ids"])
    assert torch.equal(mixed["scores"].view(torch.int32),
                       plain["scores"].view(torch.int32))
    assert torch.equal(top["ids"], plain["ids"])
    assert mixed["facets"].shape[0] == 2
    assert len(mixed["top"]) == 1 and mixed["top"][0] == top["top"][0]
    res = facet_results(_mixed_spec(), pack_facets(_mixed_spec(), 6),
                        mixed["facets"].numpy(), n_rows=6, top=mixed["top"])
    assert res[0].top_domains == top["top"][0][0] and res[0].domains == {}
    assert res[1].top_domains is None
    assert set(res[1].domains) == {"a.org", "c.org"}
    assert res[2:] == [None] * 4


# ---------------------------------------------------------------- serving

def test_facet_request_token_round_trip():
    q = with_facet_request("rust async", ["B.org", "a.org"], 20)
    assert q == "rust async facets:20@b.org,a.org"
    assert parse_facet_request(q) == ("rust async", ("b.org", "a.org"), 20)
    assert parse_facet_token(q) == ("rust async", ("b.org", "a.org"))
    assert with_facet_request("rust", (), 5) == "rust facets:5@"
    assert parse_facet_request("rust facets:5@") == ("rust", (), 5)
    # today's tokens read and write as they did
    assert with_facet_request("rust", ["a.org"], 0) \
        == with_facet_token("rust", ["a.org"]) == "rust facets:@a.org"
    assert parse_facet_request("rust facets:@a.org") == ("rust", ("a.org",), 0)
    assert parse_facet_request("rust async") == ("rust async", None, 0)
    assert parse_facet_request("about facets:x@y and facets:-3@z") == (
        "about facets:x@y and facets:-3@z", None, 0)
    assert parse_facet_request("rust facets:" + "9" * 30 + "@")[2] == int(
        "9" * 30)


# few.net and rare.org tie at 5 matches of "zebra": the hash decides
_TIE = sorted(["few.net", "rare.org"], key=domain_hash)


def _ctx(engine: bool):
    cfg = dataclasses.replace(Config(), gpu=GpuConfig(filters=True))
    c = AppContext.create(config=cfg, with_engine=engine, with_worker=False,
                          in_memory=True)
    for i in range(40):
        site = "big.com" if i % 4 else ("rare.org" if i % 8 else "few.net")
        c.index_document(Document(
            url=f"https://{site}/p{i}", title=f"zebra page {i}",
            text="zebra stripes " + " ".join(f"w{i}x{j}" for j in range(i)),
            language=("en", "de", "")[i % 3], crawled_at=1000.0 + i),
            attest=False, credit=False)
    for i in range(5):
        c.index_document(Document(
            url=f"https://other.net/p{i}", title=f"lion page {i}",
            text=f"lion mane savanna n{i}", language="en"),
            attest=False, credit=False)
    if engine:
        c.flush_engine()
    return c


def test_app_context_names_the_top_domains_in_order():
    c = _ctx(True)
    try:
        listed = c.search("zebra", limit=5, deduct=False, facets=True,
                          facet_domains=["rare.org", "nowhere.io"])
        assert "top_domains" not in listed.facets
        resp = c.search("zebra", limit=5, deduct=False, facets=True,
                        facet_domains=["rare.org", "nowhere.io"],
                        top_domains=2)
        assert resp is not listed, "T joins the cache key"
        f = resp.facets
        assert list(f["top_domains"].items()) == [("big.com", 30),
                                                  (_TIE[0], 5)]
        assert f["top_domains_exact"] is True and f["top_domains_bound"] == 0
        # everything else is what the request without T answers
        assert {k: v for k, v in f.items() if not k.startswith("top_")} \
            == listed.facets
        assert f["domains"] == {"rare.org": 5, "nowhere.io": 0}
        assert resp.total_matches == listed.total_matches == 40
        assert [h.doc_id for h in resp.results] \
            == [h.doc_id for h in listed.results]
        # the tie between few.net and rare.org goes by hash
        three = c.search("zebra", limit=5, deduct=False, facets=True,
                         top_domains=32).facets["top_domains"]
        assert list(three.items()) == [("big.com", 30), (_TIE[0], 5),
                                       (_TIE[1], 5)]
        # the cache: T = 0 shares the key a facet request always had
        assert c.search("zebra", limit=5, deduct=False, facets=True,
                        facet_domains=["rare.org", "nowhere.io"],
                        top_domains=0) is listed
        assert c.search("zebra", limit=5, deduct=False, facets=True,
                        facet_domains=["rare.org", "nowhere.io"],
                        top_domains=2) is resp
        assert QueryCache.make_key("q", limit=5, mode="auto", facets=[],
                                   top_domains=None) \
            == QueryCache.make_key("q", limit=5, mode="auto", facets=[])
        # without facets the parameter asks for nothing
        plain = c.search("zebra", limit=5, deduct=False)
        assert c.search("zebra", limit=5, deduct=False,
                        top_domains=2) is plain and plain.facets is None
        with pytest.raises(ValueError, match="32"):
            c.search("zebra", deduct=False, facets=True, top_domains=33)
        with pytest.raises(ValueError):
            c.search("zebra", deduct=False, facets=True, top_domains=-1)
        # a warm start knows no names: they come from the store, once
        c.engine._domain_names.clear()
        warm = c.search("zebra", limit=5, deduct=False, facets=True,
                        top_domains=2, use_cache=False)
        assert list(warm.facets["top_domains"]) == ["big.com", _TIE[0]]
        # and a hash nobody can name is shown as one
        c.engine._domain_names.clear()
        anon = c.search("zebra", limit=5, deduct=False, facets=True,
                        top_domains=1, use_cache=False)
        assert anon.facets["top_domains"] \
            == {"#%08x" % domain_hash("big.com"): 30}
    finally:
        c.close()


def test_a_typed_top_request_cannot_fail_its_batch():
    c = _ctx(True)
    try:
        def key(hits):
            return [(h.doc_id, h.url, h.title) for h in hits]
        alone = c._batch_execute(["zebra"], 5)[0]
        huge = "zebra facets:" + "9" * 25 + "@"
        # typed into a query: dropped on the caller's thread
        resp = c.search(huge, limit=5, deduct=False, use_cache=False)
        assert resp.facets is None and "facets:" not in resp.effective_query
        assert key(resp.results) == key(alone)
        # past AppContext.search: clamped to the cap, never raised
        both = c._batch_execute(["zebra", huge, "lion facets:2@",
                                 with_facet_token("lion")], 5)
        assert type(both[0]) is list and key(both[0]) == key(alone)
        assert isinstance(both[1], FacetedHits)
        assert [n for _, n in both[1].counts.top_domains] == [30, 5, 5]
        assert both[2].counts.top_domains == ((domain_hash("other.net"), 5),)
        assert both[3].counts.top_domains is None
        assert both[3].counts.total == 5
    finally:
        c.close()


def test_app_context_without_engine_counts_the_results():
    c = _ctx(False)
    try:
        resp = c.search("zebra", limit=8, deduct=False, facets=True,
                        top_domains=2)
        f = resp.facets
        assert f["scope"] == "results" and resp.total_matches is None
        assert set(f) == {"scope", "domains", "languages", "date_ranges",
                          "top_domains"}
        want = Counter(r.domain for r in resp.results).most_common(2)
        assert list(f["top_domains"].items()) == want and len(want) == 2
        assert "top_domains" not in c.search(
            "zebra", limit=8, deduct=False, facets=True).facets
    finally:
        c.close()


def test_http_route_mcp_tool_and_sdk_pass_the_parameter_through():
    import httpx
    from fastapi.testclient import TestClient

    from infomesh_amd.api.local_api import create_app
    from infomesh_amd.mcp.tools import TOOLS
    from infomesh_amd.sdk.client import InfoMeshClient
    c = _ctx(True)
    try:
        http = TestClient(create_app(c))
        plain = http.get("/search", params={"q": "zebra", "limit": 5,
                                            "facets": 1}).json()
        assert "top_domains" not in plain["facets"]
        body = http.get("/search", params={
            "q": "zebra", "limit": 5, "facets": 1, "top_domains": 2}).json()
        assert body["results"] == plain["results"]
        assert list(body["facets"]["top_domains"].items()) \
            == [("big.com", 30), (_TIE[0], 5)]
        assert body["facets"]["top_domains_exact"] is True
        assert body["facets"]["top_domains_bound"] == 0
        assert http.get("/search", params={
            "q": "zebra", "facets": 1, "top_domains": 33}).status_code == 400
        # without facets=1 the parameter asks for nothing
        assert "facets" not in http.get("/search", params={
            "q": "zebra", "limit": 5, "top_domains": 2}).json()
        # MCP tool
        props = next(t for t in TOOLS if t["name"] == "web_search")[
            "inputSchema"]["properties"]
        assert props["top_domains"]["type"] == "integer"
        h = Handlers(c)
        out = h.web_search(query="zebra", limit=5, facets=True)
        assert "top_domains" not in out["facets"]
        out = h.web_search(query="zebra", limit=5, facets=True,
                           top_domains=2)
        assert list(out["facets"]["top_domains"]) == ["big.com", _TIE[0]]
        # SDK
        seen = []

        def handler(request: httpx.Request) -> httpx.Response:
            seen.append(dict(request.url.params))
            r = http.get("/search", params=dict(request.url.params))
            return httpx.Response(r.status_code, json=r.json())
        sdk = InfoMeshClient(transport=httpx.MockTransport(handler))
        sdk.search("zebra", limit=5, facets=True)
        assert "top_domains" not in seen[-1]
        got = sdk.search("zebra", limit=5, facets=True, top_domains=2)
        assert seen[-1]["top_domains"] == "2"
        assert got["facets"]["top_domains"] == {"big.com": 30, _TIE[0]: 5}
        sdk.close()
    finally:
        c.close()
