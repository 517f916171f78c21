"""Domain allow/block lists without a GPU: the list packer, the bitmask
oracle, CpuShard, the parser, the store, the services and MCP handler
(the recall the over-fetch lost), the 2-rank query plane and the
hash-collision guard."""
from __future__ import annotations

import dataclasses
import os

import numpy as np
import pytest
import torch

from infomesh_amd.config import Config, GpuConfig
from infomesh_amd.index.doc_attrs import (DEAD_BIT, HAS_ALLOW_BIT,
                                          HAS_BLOCK_BIT, MAX_LIST_HASHES,
                                          DocFilter, domain_hash, pack_attrs,
                                          pack_pred, pack_pred_sets, passes,
                                          words_i32)
from infomesh_amd.index.gpu_index import CpuShard
from infomesh_amd.index.local_store import Document, LocalStore
from infomesh_amd.mcp.handlers import Handlers
from infomesh_amd.ops import reference as R
from infomesh_amd.parallel.fabric import Fabric
from infomesh_amd.parallel.query_plane import DistributedQueryPlane
from infomesh_amd.search.nlp import parse_query_filters, with_filter_tokens
from infomesh_amd.services import AppContext

LANGS = ["en", "de", "fr"]
DOMAINS = ["a.org", "b.org", "c.org", "d.org", "e.org", "f.org"]
T0 = 1_700_000_000


# --------------------------------------------------------------- packing

def test_lists_are_deduped_sorted_unsigned_and_flagged():
    names = ["B.org", "a.org", "b.org", "zz.example", "c.org", "a.org "]
    words, allow, block = pack_pred_sets(
        DocFilter(language="de", sites=tuple(names),
                  exclude_sites=("x.org", "X.ORG")))
    want = sorted({domain_hash(n) for n in names})
    assert len(want) == 4 and list(allow) == want
    assert all(0 <= h <= 0xFFFFFFFF for h in allow)
    assert block == (domain_hash("x.org"),)
    assert HAS_ALLOW_BIT == 1 << 18 and HAS_BLOCK_BIT == 1 << 19
    assert words[2] == ((ord("d") << 8) | ord("e")) | (1 << 18) | (1 << 19)
    # one flag each, and none without a list
    assert pack_pred_sets(DocFilter(sites=("a.org",)))[0][2] == 1 << 18
    assert pack_pred_sets(DocFilter(exclude_sites=("a.org",)))[0][2] == 1 << 19
    # unsigned order: a hash with the top bit set sorts last, not first
    packed = pack_pred_sets(((0, 0xFFFFFFFF, 0, 0),
                             (0x80000000, 5), (0xFFFFFFFF,)))
    assert packed == ((0, 0xFFFFFFFF, (1 << 18) | (1 << 19), 0),
                      (0x80000000, 5), (0xFFFFFFFF,))   # passes through
    some = sorted({domain_hash(f"d{i}.org") for i in range(64)})
    assert some[-1] >= 0x80000000 > some[0], "sample too small to show order"
    assert list(pack_pred_sets(DocFilter(sites=tuple(
        f"d{i}.org" for i in range(64))))[1]) == some


def test_pack_pred_is_unchanged_for_filters_without_lists():
    # the filters of test_pack_attrs_and_pred_round_trip, and their words
    # as the parent commit packed them
    f = DocFilter(language="de", site="Kernel.org", after=T0 + 0.25,
                  before=T0 + 9.75)
    want = (T0 + 1, T0 + 9, ((ord("d") << 8) | ord("e")) | (1 << 16),
            domain_hash("kernel.org"))
    assert pack_pred(f) == want
    assert pack_pred(None) == (0, 0xFFFFFFFF, 0, 0)
    assert pack_pred(want) == want
    for g in (None, f, want, DocFilter(), DocFilter(site="b.org")):
        assert pack_pred_sets(g) == (pack_pred(g), (), ())
    # a filter with lists has no 4-word form
    with pytest.raises(ValueError):
        pack_pred(DocFilter(sites=("a.org",)))


def test_more_than_the_cap_raises():
    names = tuple(f"host{i}.example" for i in range(MAX_LIST_HASHES + 1))
    assert len({domain_hash(n) for n in names}) == 2049
    assert MAX_LIST_HASHES == 2048
    with pytest.raises(ValueError, match="2048"):
        pack_pred_sets(DocFilter(sites=names))
    with pytest.raises(ValueError, match="2048"):      # the two together
        pack_pred_sets(DocFilter(sites=names[:2000],
                                 exclude_sites=names[2000:]))
    words, allow, block = pack_pred_sets(
        DocFilter(sites=names[:2000], exclude_sites=names[2000:2048]))
    assert len(allow) + len(block) == 2048


# ------------------------------------------------- oracle vs brute force

def _brute_pass(attr, f: DocFilter | None) -> bool:
    """The predicate spelled out on unpacked fields and domain STRINGS."""
    crawled, lang, domain, dead = attr
    if dead:
        return False
    if f is None:
        return True
    sec = int(crawled)
    if f.after is not None and sec < int(np.ceil(f.after)):
        return False
    if f.before is not None and sec > int(np.floor(f.before)):
        return False
    if f.language and (lang or "").lower() != f.language.lower():
        return False
    if f.site and domain != f.site.lower():
        return False
    if f.sites and domain not in [s.lower() for s in f.sites]:
        return False
    if domain in [s.lower() for s in f.exclude_sites]:
        return False
    return True


LIST_FILTERS = [
    DocFilter(sites=("a.org", "c.org")),                        # allow only
    DocFilter(exclude_sites=("b.org",)),                        # block only
    DocFilter(sites=("a.org", "b.org", "c.org"),
              exclude_sites=("b.org", "d.org")),                # overlap
    DocFilter(site="a.org", sites=("a.org", "b.org")),          # both hold
    DocFilter(site="e.org", sites=("a.org", "b.org")),          # nothing can
    DocFilter(language="de", sites=("c.org", "d.org", "e.org"),
              after=T0 + 20, before=T0 + 80.5,
              exclude_sites=("d.org",)),
    DocFilter(sites=("nowhere.example",)),
    None,
]


def _unpack(bits: torch.Tensor, n: int) -> np.ndarray:
    w = bits.numpy().view(np.uint32)
    return np.unpackbits(w.view(np.uint8), axis=1,
                         bitorder="little")[:, :n].astype(bool)


def _tables(packed):
    """[(words, allow, block)] -> preds, desc, doms as the kernel and its
    oracle read them."""
    desc, flat = [], []
    for _, allow, block in packed:
        desc.append((len(flat), len(allow), len(flat) + len(allow),
                     len(block)))
        flat += list(allow) + list(block)
    return (torch.from_numpy(words_i32([w for w, _, _ in packed])),
            torch.tensor(desc, dtype=torch.int32).reshape(-1, 4),
            torch.from_numpy(np.asarray(flat, dtype=np.uint32).view(np.int32)))


def test_set_oracle_matches_brute_force_over_domain_strings():
    rng = np.random.default_rng(1)
    n = 200
    docs = [(T0 + int(rng.integers(0, 100)),
             [None, "en", "de", "fr"][int(rng.integers(0, 4))],
             DOMAINS[int(rng.integers(0, 6))], bool(rng.integers(0, 8) == 0))
            for _ in range(n)]
    docs[0] = (T0 + 50, "de", "c.org", True)       # dead in an allowed domain
    docs[1] = (T0 + 50, "de", "c.org", False)
    attrs = words_i32([pack_attrs(l, d, c) for c, l, d, _ in docs])
    attrs[:, 1] |= np.array([DEAD_BIT if dead else 0 for *_, dead in docs],
                            dtype=np.int32)
    preds, desc, doms = _tables([pack_pred_sets(f) for f in LIST_FILTERS])
    bits = R.filter_bitmask_sets(torch.from_numpy(attrs), preds, desc, doms)
    W = (n + 63) // 64 * 2
    assert bits.shape == (len(LIST_FILTERS), W) and bits.dtype == torch.int32
    got = _unpack(bits, W * 32)
    assert not got[:, n:].any(), "bits past N must be zero"
    for p, f in enumerate(LIST_FILTERS):
        assert got[p, :n].tolist() == [_brute_pass(d, f) for d in docs], f
    assert not got[0, 0] and got[0, 1]
    assert not got[4].any() and not got[6].any() and got[3].any()
    # without the arrays passes() is what it was: the flag bits alone
    # restrict nothing
    w = pack_pred_sets(LIST_FILTERS[0])[0]
    assert passes(attrs, w).tolist() == passes(attrs, pack_pred(None)).tolist()


# -------------------------------------------------------------- CpuShard

N_DOCS = 300


def _corpus(seed=3):
    rng = np.random.default_rng(seed)
    toks = [rng.integers(0, 60, size=rng.integers(5, 25)).astype(np.int64)
            for _ in range(N_DOCS)]
    meta = [(LANGS[i % 3], DOMAINS[(i // 3) % 6], T0 + i)
            for i in range(N_DOCS)]
    emb = torch.nn.functional.normalize(
        torch.randn(N_DOCS, 16, generator=torch.Generator().manual_seed(seed)),
        dim=-1).bfloat16()
    return toks, meta, emb


def _shard(rank=0, world=1, seed=3):
    toks, meta, emb = _corpus(seed)
    shard = CpuShard()
    shard.build_from_arrays(
        np.concatenate(toks), np.repeat(np.arange(N_DOCS),
                                        [len(t) for t in toks]),
        np.array([len(t) for t in toks]),
        np.arange(N_DOCS, dtype=np.int64) * world + rank, emb,
        attrs=[pack_attrs(l, d, c) for l, d, c in meta])
    return shard, meta


QUERIES = [np.array([1, 2, 3]), np.array([7, 11]), np.array([20]),
           np.array([5, 6])]


def test_cpu_shard_list_search_equals_brute_force_on_both_planes():
    shard, meta = _shard()
    k = 15
    filters = [DocFilter(sites=("a.org", "f.org")),
               DocFilter(exclude_sites=("b.org", "c.org", "d.org")),
               DocFilter(language="fr", sites=("a.org", "b.org"),
                         exclude_sites=("b.org",)),
               # 4 documents pass: fewer than k
               DocFilter(language="de", sites=("e.org", "zz.example"),
                         after=T0, before=T0 + 71)]
    qemb = torch.nn.functional.normalize(
        torch.randn(4, 16, generator=torch.Generator().manual_seed(9)), dim=-1)
    full = shard.search(QUERIES, qemb, k=N_DOCS)          # unfiltered scores
    hits = shard.search(QUERIES, qemb, k=k, filters=filters)
    # the forwarded packed form is accepted wherever a DocFilter is
    again = shard.search(QUERIES, qemb, k=k,
                         filters=[pack_pred_sets(f) for f in filters])
    assert torch.equal(hits.bm25_ids, again.bm25_ids)
    assert torch.equal(hits.dense_ids, again.dense_ids)
    short = 0
    for qi, f in enumerate(filters):
        ok = np.array([_brute_pass((c, l, d, False), f) for l, d, c in meta])
        for ids, scores, fids, fscores in (
                (full.bm25_ids, full.bm25_scores, hits.bm25_ids,
                 hits.bm25_scores),
                (full.dense_ids, full.dense_scores, hits.dense_ids,
                 hits.dense_scores)):
            by_row = np.zeros(N_DOCS, dtype=np.float32)
            by_row[ids[qi].numpy()] = scores[qi].numpy()
            want = [i for i in np.argsort(-by_row, kind="stable") if ok[i]][:k]
            n_ok = len(want)
            got = fids[qi].tolist()
            # scores equal exactly; ids equal up to ties; -inf / -1 pads
            assert fscores[qi, :n_ok].tolist() == [by_row[i] for i in want]
            assert got[n_ok:] == [-1] * (k - n_ok)
            assert (fscores[qi, n_ok:] == -float("inf")).all()
            for g, w in zip(got[:n_ok], want):
                assert ok[g] and (g == w or by_row[g] == by_row[w])
            assert len(set(got[:n_ok])) == n_ok
            short += n_ok < k
    assert short == 2, "the last row must come up short on both planes"


# ---------------------------------------------------------------- parser

def test_parser_reads_every_list_form():
    pq = parse_query_filters("rust site:A.org,b.org async")
    assert (pq.text, pq.site, pq.sites) == ("rust async", None,
                                            ("a.org", "b.org"))
    assert pq.exclude_sites == ()
    pq = parse_query_filters("rust -site:a.org")
    assert (pq.text, pq.site, pq.sites, pq.exclude_sites) == (
        "rust", None, (), ("a.org",))
    assert "-" not in pq.text
    pq = parse_query_filters("-site:a.org,B.org rust lang:de")
    assert (pq.text, pq.exclude_sites, pq.language) == (
        "rust", ("a.org", "b.org"), "de")
    pq = parse_query_filters("rust site:kernel.org")          # as it was
    assert (pq.text, pq.site, pq.sites, pq.exclude_sites) == (
        "rust", "kernel.org", (), ())
    pq = parse_query_filters("x site:a.org,b.org -site:c.org site:d.org")
    assert (pq.site, pq.sites, pq.exclude_sites) == (
        "d.org", ("a.org", "b.org"), ("c.org",))
    pq = parse_query_filters(f"x after:@{T0} before:@{T0 + 90}.5")
    assert (pq.text, pq.after, pq.before) == ("x", float(T0), T0 + 90.5)
    assert parse_query_filters("x after:2024-01-02").after is not None
    # a minus that is not in front of site: stays text
    assert parse_query_filters("well-known -lang:de").text == "well-known -"


def test_with_filter_tokens_round_trips_through_the_parser():
    q = with_filter_tokens("rust async", ["B.org", "a.org"], ["c.org"],
                           T0 + 0.25)
    pq = parse_query_filters(q)
    assert (pq.text, pq.sites, pq.exclude_sites, pq.after, pq.site) == (
        "rust async", ("b.org", "a.org"), ("c.org",), T0 + 1.0, None)
    # one allowed name is still a list, and keeps its www.
    pq = parse_query_filters(with_filter_tokens("q", ["www.a.org"]))
    assert (pq.text, pq.site, pq.sites) == ("q", None, ("www.a.org",))
    assert with_filter_tokens("q") == "q"
    # a name no host can have stays in the list and cannot split it
    pq = parse_query_filters(with_filter_tokens("q", ["a b,c.org"]))
    assert pq.text == "q" and pq.sites == ("a_b_c.org",)


# ----------------------------------------------------------------- store

def _store():
    store = LocalStore()
    rows = [("https://python.org/a", "python.org"),
            ("https://docs.python.org/b", "docs.python.org"),
            ("https://notpython.org/c", "notpython.org"),
            ("https://rust-lang.org/d", "rust-lang.org"),
            ("https://python.org/e", "python.org")]
    for i, (url, _) in enumerate(rows):
        store.add_document(Document(
            url=url, title=f"guide {i}",
            text=f"language guide number{i} " + "filler " * i))
    return store, rows


def test_store_search_with_domain_lists():
    store, rows = _store()
    everything = store.search("guide", limit=10)
    assert len(everything) == 5
    for inc, exc in ((["python.org", "RUST-lang.org"], None),
                     (None, ["python.org"]),
                     (["python.org", "docs.python.org"], ["python.org"]),
                     (["absent.example"], None)):
        got = store.search("guide", limit=10, include_domains=inc,
                           exclude_domains=exc)
        want = [h for h in everything
                if (not inc or h.domain in [d.lower() for d in inc])
                and h.domain not in (exc or [])]
        assert [h.url for h in got] == [h.url for h in want], (inc, exc)
    assert [h.domain for h in store.search(
        "guide", limit=10, include_domains=["python.org", "docs.python.org"],
        exclude_domains=["python.org"])] == ["docs.python.org"]
    store.close()


def test_domains_matching_is_a_suffix_on_a_label_boundary():
    store, _ = _store()
    assert store.domains_matching(["python.org"]) == [
        "docs.python.org", "python.org"]                 # not notpython.org
    assert store.domains_matching(["Python.ORG", "rust-lang.org"]) == [
        "docs.python.org", "python.org", "rust-lang.org"]
    assert store.domains_matching(["org", "%", "_ython.org"]) == [
        "docs.python.org", "notpython.org", "python.org", "rust-lang.org"]
    assert store.domains_matching(["%", "_ython.org", "ython.org"]) == []
    assert store.domains_matching([]) == []
    store.close()


# ------------------------------------------- the recall the over-fetch lost

def _recall_ctx(gpu_filters: bool):
    cfg = dataclasses.replace(Config(), gpu=GpuConfig(filters=gpu_filters))
    c = AppContext.create(config=cfg, with_engine=gpu_filters,
                          with_worker=False, in_memory=True)
    assert (c.engine is not None) == gpu_filters
    # 30 short documents full of the term outrank 3 long ones that
    # mention it once
    for i in range(30):
        c.index_document(Document(
            url=f"https://big.com/p{i}", title=f"zebra zebra {i}",
            text=f"zebra zebra zebra stripes zebra number{i}"),
            attest=False, credit=False)
    for i in range(3):
        c.index_document(Document(
            url=f"https://rare.org/p{i}", title=f"savanna notes {i}",
            text=f"a zebra was seen once near the river crossing{i} "
                 + " ".join(f"padding{i}x{j}" for j in range(60))),
            attest=False, credit=False)
    c.flush_engine()
    return c


RARE = [f"https://rare.org/p{i}" for i in range(3)]


@pytest.mark.parametrize("gpu_filters", [False, True],
                         ids=["fts", "engine"])
def test_domain_lists_return_the_true_top_of_the_passing_documents(
        gpu_filters):
    c = _recall_ctx(gpu_filters)
    try:
        plain = c.search("zebra", limit=10, use_cache=False, deduct=False)
        assert len(plain.results) == 10
        assert all("big.com" in h.url for h in plain.results), \
            "rare.org must rank below the over-fetch window"
        queries = c.batcher.stats()["queries"] if gpu_filters else 0
        h = Handlers(c)
        out = h.web_search(query="zebra", limit=5,
                           domain_allowlist=["rare.org"])
        assert sorted(r["url"] for r in out["results"]) == RARE
        out = h.web_search(query="zebra", limit=5,
                           domain_blocklist=["big.com"])
        assert sorted(r["url"] for r in out["results"]) == RARE
        resp = c.search("zebra", limit=5, include_domains=["rare.org"],
                        use_cache=False, deduct=False)
        assert sorted(r.url for r in resp.results) == RARE
        resp = c.search("zebra", limit=5, exclude_domains=["big.com"],
                        use_cache=False, deduct=False)
        assert sorted(r.url for r in resp.results) == RARE
        # a page of the blocked domain's size is not cut short either
        resp = c.search("zebra", limit=5, exclude_domains=["rare.org"],
                        use_cache=False, deduct=False)
        assert len(resp.results) == 5
        if gpu_filters:     # all five ran on the engine, not on FTS
            assert c.batcher.stats()["queries"] == queries + 5
    finally:
        c.close()


def test_http_route_and_sdk_clients_carry_the_lists():
    import asyncio

    import httpx
    from fastapi.testclient import TestClient

    from infomesh_amd.api.local_api import create_app
    from infomesh_amd.sdk.client import AsyncInfoMeshClient, InfoMeshClient
    c = _recall_ctx(False)
    try:
        http = TestClient(create_app(c))
        r = http.get("/search", params={"q": "zebra", "limit": 5,
                                        "include_domains": "rare.org,x.org"})
        assert sorted(h["url"] for h in r.json()["results"]) == RARE
        r = http.get("/search", params={"q": "zebra", "limit": 5,
                                        "exclude_domains": "big.com"})
        assert sorted(h["url"] for h in r.json()["results"]) == RARE
        r = http.get("/search", params={"q": "zebra", "limit": 5})
        assert all("big.com" in h["url"] for h in r.json()["results"])

        # both clients put the same parameters on the wire; the route
        # above is what answers them
        def handler(request: httpx.Request) -> httpx.Response:
            return httpx.Response(200, json=http.get(
                "/search", params=dict(request.url.params)).json())
        with InfoMeshClient(transport=httpx.MockTransport(handler)) as sdk:
            hits = sdk.search("zebra", limit=5, exclude_domains=["big.com"],
                              recency_days=30)
            assert sorted(h["url"] for h in hits) == RARE
            assert len(sdk.search("zebra", limit=5)) == 5

        async def run():
            async with AsyncInfoMeshClient(
                    transport=httpx.MockTransport(handler)) as sdk:
                return await sdk.search("zebra", limit=5,
                                        include_domains=["rare.org"])
        assert sorted(h["url"] for h in asyncio.run(run())) == RARE
    finally:
        c.close()


def test_web_search_over_the_cap_falls_back_to_the_over_fetch(caplog):
    c = _recall_ctx(False)
    try:
        many = [f"host{i}.example" for i in range(2100)]
        c.store.domains_matching = lambda names: list(names)
        with caplog.at_level("WARNING", logger="infomesh.mcp"):
            out = Handlers(c).web_search(query="zebra", limit=5,
                                         domain_blocklist=many)
        assert "over the cap" in caplog.text
        assert len(out["results"]) == 5
        with pytest.raises(ValueError, match="2048"):
            pack_pred_sets(DocFilter(exclude_sites=tuple(many)))
    finally:
        c.close()


def test_recency_days_travels_as_a_filter_token():
    c = _recall_ctx(False)
    try:
        old = Document(url="https://old.net/p", title="zebra archive",
                       text="zebra zebra zebra from the archive",
                       crawled_at=T0)
        c.index_document(old, attest=False, credit=False)
        urls = [h.url for h in c.search("zebra", limit=50, use_cache=False,
                                        deduct=False).results]
        assert "https://old.net/p" in urls
        urls = [h.url for h in c.search("zebra", limit=50, recency_days=30,
                                        use_cache=False, deduct=False).results]
        assert len(urls) == 33 and "https://old.net/p" not in urls
    finally:
        c.close()


# ------------------------------------------------------- collision guard

def test_hash_collision_on_an_allowed_domain_is_dropped_at_hydration():
    cfg = dataclasses.replace(Config(), gpu=GpuConfig(filters=True))
    c = AppContext.create(config=cfg, with_engine=True, with_worker=False,
                          in_memory=True)
    try:
        ids = {}
        for url in ("https://kernel.org/sched", "https://kernel.org/rt",
                    "https://lwn.net/sched", "https://rocm.docs/queues"):
            ids[url] = c.index_document(
                Document(url=url, title="scheduler",
                         text=f"the scheduler of {url} maps tasks"),
                attest=False, credit=False)
        c.flush_engine()
        # lwn.net's record now carries kernel.org's hash: a collision
        shard = c.engine.shard
        row = int((shard.global_ids == ids["https://lwn.net/sched"])
                  .nonzero()[0])
        shard._attr_buf[row, 2] = int(np.uint32(
            domain_hash("kernel.org")).view(np.int32))
        f = DocFilter(sites=("kernel.org", "other.example"))
        raw = c.engine.search_many(["scheduler"], limit=10, filters=[f])[0]
        assert sorted(h.doc_id for h in raw) == sorted(
            ids[u] for u in ids if "rocm" not in u), "no collision staged"
        resp = c.search("scheduler", limit=10, use_cache=False, deduct=False,
                        include_domains=["kernel.org", "other.example"])
        assert sorted(h.url for h in resp.results) == [
            "https://kernel.org/rt", "https://kernel.org/sched"]
    finally:
        c.close()


# ------------------------------------------------- 2-process gloo plane

PLANE_FILTERS = [
    DocFilter(language="de", sites=("c.org", "d.org", "zz.example"),
              exclude_sites=("d.org",)),
    None,
    DocFilter(exclude_sites=("a.org", "b.org")),
    DocFilter(site="e.org"),
]


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


def _list_worker(rank: int, world: int, port: int, out_dir: str):
    os.environ["HIP_VISIBLE_DEVICES"] = "-1"
    os.environ["CUDA_VISIBLE_DEVICES"] = "-1"
    assert not torch.cuda.is_available(), "GPUs still visible to the worker"
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    real = Fabric(backend="gloo")
    fabric = _CountingFabric(real)
    shard, _ = _shard(rank, world, seed=5 + rank)
    plane = DistributedQueryPlane(shard, fabric, k_per_shard=40)
    terms = [np.array([1, 2, 3]), np.array([4, 5]), np.array([7]),
             np.array([9])]
    lead = rank == 0
    # what every rank sees after the broadcast, and at what cost
    _, seen = plane._broadcast_terms(terms if lead else None, 4,
                                     PLANE_FILTERS if lead else None)
    with_lists = fabric.broadcasts
    _, plain = plane._broadcast_terms(
        terms if lead else None, 4,
        [DocFilter(site="e.org"), None, None, None] if lead else None)
    without_lists = fabric.broadcasts - with_lists
    fabric.broadcasts = 0
    _, none = plane._broadcast_terms(terms if lead else None, 4, None)
    unfiltered = fabric.broadcasts
    emb = torch.nn.functional.normalize(
        torch.randn(4, 16, generator=torch.Generator().manual_seed(2)), dim=-1)
    fused = plane.search_batch(terms if lead else None,
                               emb if lead else None, B=4, dim=16,
                               n_results=30,
                               filters=PLANE_FILTERS if lead else None)
    assert (fused is not None) == lead
    torch.save({"seen": seen, "plain": plain, "none": none,
                "counts": (with_lists, without_lists, unfiltered),
                "bm": fused.bm25_ids if lead else None,
                "dn": fused.dense_ids if lead else None},
               os.path.join(out_dir, f"rank{rank}"))
    real.destroy()


def test_plane_gloo_rank1_receives_rank0_lists(tmp_path):
    import torch.multiprocessing as mp
    mpc = mp.get_context("spawn")
    procs = [mpc.Process(target=_list_worker,
                         args=(r, 2, 29567, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    got = [torch.load(tmp_path / f"rank{r}", weights_only=False)
           for r in range(2)]
    want = [None if f is None else pack_pred_sets(f) for f in PLANE_FILTERS]
    # rows without a list arrive as the four words, as before
    want = [w if w is None or w[1] or w[2] else w[0] for w in want]
    for r in range(2):
        assert got[r]["seen"] == want, f"rank {r}: lists not bit-for-bit"
        assert got[r]["plain"] == [pack_pred(DocFilter(site="e.org")),
                                   None, None, None]
        assert got[r]["none"] is None
        # terms, then counts and hashes only for the batch that has lists
        assert got[r]["counts"] == (3, 1, 1)
    _, meta = _shard()
    for ids in (got[0]["bm"], got[0]["dn"]):
        for qi, f in enumerate(PLANE_FILTERS):
            row = ids[qi][ids[qi] >= 0]
            by_rank = {r: row[row % 2 == r] // 2 for r in (0, 1)}
            assert len(by_rank[1]) > 0, "rank 1's shard must answer"
            for r in (0, 1):
                for local in by_rank[r].tolist():
                    l, d, c = meta[local]
                    assert _brute_pass((c, l, d, False), f), (qi, r, local)
        # "de" on c.org: 17 of a shard's 300 documents, fewer than k = 40
        assert 0 < int((ids[0] >= 0).sum()) < 80
        assert (ids[1] >= 0).all()
