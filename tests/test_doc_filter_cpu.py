"""Document attributes, deletes and query filters without a GPU: the
packers, the bitmask oracle, CpuShard, the manifest, the engine, the
services and the 2-rank query plane."""
from __future__ import annotations

import dataclasses
import os

import numpy as np
import pytest
import torch

from infomesh_amd.config import Config, GpuConfig
from infomesh_amd.engine import HybridEngine
from infomesh_amd.hashing import hash64
from infomesh_amd.index.doc_attrs import (DEAD_BIT, DocFilter, pack_attrs,
                                          pack_pred, words_i32)
from infomesh_amd.index.gpu_index import CpuShard, bm25_term_ids
from infomesh_amd.index.local_store import Document
from infomesh_amd.index.manifest import load_shard, save_shard
from infomesh_amd.ops import reference as R
from infomesh_amd.parallel.fabric import Fabric
from infomesh_amd.parallel.query_plane import DistributedQueryPlane
from infomesh_amd.services import AppContext

LANGS = ["en", "de", "fr"]
DOMAINS = ["a.org", "b.org", "c.org", "d.org", "e.org"]
T0 = 1_700_000_000


# --------------------------------------------------------------- packers

def test_pack_attrs_and_pred_round_trip():
    w = pack_attrs("EN", "Kernel.ORG", T0 + 0.75)
    assert w == (T0, (ord("e") << 8) | ord("n"),
                 hash64("kernel.org") & 0xFFFFFFFF, 0)
    assert pack_attrs(None, None, None) == (0, 0, hash64("") & 0xFFFFFFFF, 0)
    assert pack_attrs("", "x", 5)[1] == 0          # unknown language
    assert pack_pred(None) == (0, 0xFFFFFFFF, 0, 0)
    # after rounds up, before rounds down
    x, y, z, ww = pack_pred(DocFilter(language="de", site="Kernel.org",
                                      after=T0 + 0.25, before=T0 + 9.75))
    assert (x, y) == (T0 + 1, T0 + 9)
    assert z == ((ord("d") << 8) | ord("e")) | (1 << 16)
    assert ww == w[2]
    # packed words pass through unchanged (the plane forwards them)
    assert pack_pred((x, y, z, ww)) == (x, y, z, ww)
    # int32 bits survive the trip through a tensor
    t = words_i32([w, (0xFFFFFFFF, DEAD_BIT, 0x80000000, 0)])
    assert t.dtype == np.int32
    assert t.view(np.uint32).tolist() == [
        list(w), [0xFFFFFFFF, DEAD_BIT, 0x80000000, 0]]


def _brute_pass(attr, f: DocFilter | None) -> bool:
    """The predicate spelled out on unpacked fields."""
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
    return True


def _unpack(bits: torch.Tensor, n: int) -> np.ndarray:
    w = bits.numpy().view(np.uint32)
    return np.unpackbits(w.view(np.uint8), axis=1,
                         bitorder="little")[:, :n].astype(bool)


def test_bitmask_oracle_matches_brute_force():
    rng = np.random.default_rng(0)
    n = 203                                   # not a multiple of 64
    docs = []
    for i in range(n):
        lang = [None, "en", "de", "fr"][int(rng.integers(0, 4))]
        docs.append((T0 + int(rng.integers(0, 100)), lang,
                     DOMAINS[int(rng.integers(0, 5))],
                     bool(rng.integers(0, 8) == 0)))
    docs[0] = (T0 + 50, None, "a.org", False)      # unknown language
    docs[1] = (T0 + 50, "en", "a.org", False)      # the date edges
    attrs = words_i32([pack_attrs(l, d, c) for c, l, d, _ in docs])
    attrs[:, 1] |= np.array([DEAD_BIT if dead else 0
                             for *_, dead in docs], dtype=np.int32)
    filters = [
        None,
        DocFilter(language="en"),
        DocFilter(site="b.org"),
        DocFilter(after=T0 + 50),              # after == crawled_at
        DocFilter(before=T0 + 50),             # before == crawled_at
        DocFilter(after=T0 + 50.5), DocFilter(before=T0 + 49.5),
        DocFilter(language="de", site="c.org", after=T0 + 10,
                  before=T0 + 90),
    ]
    preds = torch.from_numpy(words_i32([pack_pred(f) for f in filters]))
    bits = R.filter_bitmask(torch.from_numpy(attrs), preds)
    W = (n + 63) // 64 * 2
    assert bits.shape == (len(filters), W) and bits.dtype == torch.int32
    got = _unpack(bits, W * 32)
    assert not got[:, n:].any(), "bits past N must be zero"
    for p, f in enumerate(filters):
        want = [_brute_pass(d, f) for d in docs]
        assert got[p, :n].tolist() == want, f
    # the edges, spelled out: doc 1 was crawled at exactly T0 + 50
    assert got[3, 1] and got[4, 1] and not got[5, 1] and not got[6, 1]
    # unknown language: fails a language filter, passes none
    assert not got[1, 0] and got[0, 0]


# -------------------------------------------------------------- CpuShard

N_DOCS = 300


def _corpus(seed=3):
    rng = np.random.default_rng(seed)
    toks = [rng.integers(0, 60, size=rng.integers(5, 25)).astype(np.int64)
            for _ in range(N_DOCS)]
    meta = [(LANGS[i % 3], DOMAINS[(i // 3) % 5], T0 + i) for i in range(N_DOCS)]
    emb = torch.nn.functional.normalize(
        torch.randn(N_DOCS, 16, generator=torch.Generator().manual_seed(seed)),
        dim=-1).bfloat16()
    return toks, meta, emb


def _two_segment_shard(with_attrs=True):
    toks, meta, emb = _corpus()
    shard = CpuShard()
    for lo, hi in ((0, 180), (180, N_DOCS)):
        for i in range(lo, hi):
            shard.add_document(1000 + i, toks[i], emb[i],
                               attrs=pack_attrs(*meta[i][:2], meta[i][2])
                               if with_attrs else None)
        shard.build()
    assert len(shard.segments) == 2 and shard.n_docs == N_DOCS
    return shard, toks, meta, emb


def _brute_topk(scores: np.ndarray, ok: np.ndarray, k: int) -> list[int]:
    """Top-k row indices over passing documents only; -1 pads."""
    cand = [i for i in np.argsort(-scores, kind="stable") if ok[i]][:k]
    return cand + [-1] * (k - len(cand))


QUERIES = [np.array([1, 2, 3]), np.array([7, 11]), np.array([20]),
           np.array([5, 6])]


def test_cpu_shard_filtered_search_equals_brute_force():
    shard, toks, meta, emb = _two_segment_shard()
    k = 20
    filters = [DocFilter(language="de"), DocFilter(site="c.org"),
               DocFilter(after=T0 + 100, before=T0 + 140), None]
    qemb = torch.nn.functional.normalize(
        torch.randn(4, 16, generator=torch.Generator().manual_seed(9)), dim=-1)
    full = shard.search(QUERIES, qemb, k=N_DOCS)          # unfiltered scores
    hits = shard.search(QUERIES, qemb, k=k, filters=filters)
    for qi, f in enumerate(filters):
        ok = np.array([_brute_pass((c, l, d, False), f) for l, d, c in meta])
        for ids, scores, fids, fscores in (
                (full.bm25_ids, full.bm25_scores, hits.bm25_ids,
                 hits.bm25_scores),
                (full.dense_ids, full.dense_scores, hits.dense_ids,
                 hits.dense_scores)):
            by_row = np.zeros(N_DOCS, dtype=np.float32)
            by_row[ids[qi].numpy() - 1000] = scores[qi].numpy()
            want = _brute_topk(by_row, ok, k)
            want_scores = [by_row[i] for i in want if i >= 0]
            got = fids[qi].tolist()
            n_ok = len(want_scores)
            # scores equal exactly; ids equal up to ties
            assert fscores[qi, :n_ok].tolist() == want_scores
            assert all(g == -1 for g in got[n_ok:])
            for g, w in zip(got[:n_ok], want[:n_ok]):
                assert g >= 1000 and ok[g - 1000]
                assert g - 1000 == w or by_row[g - 1000] == by_row[w]
            assert len(set(got[:n_ok])) == n_ok


def test_cpu_shard_short_row_pads_with_minus_one():
    shard, *_ = _two_segment_shard()
    # 4 documents pass: "de" on e.org inside a 60 s window
    f = DocFilter(language="de", site="e.org", after=T0, before=T0 + 59)
    hits = shard.search(QUERIES[:1], None, k=10, filters=[f])
    ids = hits.bm25_ids[0].tolist()
    n_ok = sum(1 for i in ids if i >= 0)
    assert 0 < n_ok < 10 and ids[n_ok:] == [-1] * (10 - n_ok)
    assert (hits.bm25_scores[0, n_ok:] == -float("inf")).all()


def test_cpu_shard_delete_hides_documents_in_both_planes():
    shard, toks, meta, emb = _two_segment_shard()
    qemb = emb[:4].float()
    before = shard.search(QUERIES, qemb, k=30)
    victims = set(before.bm25_ids[:, :10].flatten().tolist()) \
        | set(before.dense_ids[:, :10].flatten().tolist())
    victims.discard(-1)
    assert shard.delete(victims) == len(victims)
    assert shard.delete(victims) == 0 and shard.n_dead == len(victims)
    assert shard.n_docs == N_DOCS                # Lucene-style until purge
    after = shard.search(QUERIES, qemb, k=30)
    for ids in (after.bm25_ids, after.dense_ids):
        assert not (set(ids.flatten().tolist()) & victims)
        assert (ids >= 0).all(), "k results while enough documents survive"
    # survivors keep their scores: df / avgdl still count the tombstones
    keep = ~torch.isin(before.dense_ids[0], torch.tensor(sorted(victims)))
    assert torch.equal(before.dense_scores[0][keep][:5],
                       after.dense_scores[0][:5])


def test_purge_equals_bulk_build_from_survivors():
    shard, toks, meta, emb = _two_segment_shard()
    dead = list(range(1000, 1000 + N_DOCS, 7)) + [1000 + N_DOCS - 1]
    shard.delete(dead)
    assert shard.purge() == len(dead)
    assert shard.n_dead == 0 and len(shard.segments) == 1
    live = [i for i in range(N_DOCS) if 1000 + i not in set(dead)]
    oracle = CpuShard()
    oracle.build_from_arrays(
        np.concatenate([toks[i] for i in live]),
        np.repeat(np.arange(len(live)), [len(toks[i]) for i in live]),
        np.array([len(toks[i]) for i in live]),
        np.array([1000 + i for i in live]), emb[live],
        attrs=[pack_attrs(*meta[i][:2], meta[i][2]) for i in live])
    assert shard.n_docs == oracle.n_docs == len(live)
    assert np.array_equal(shard.df, oracle.df)
    assert np.array_equal(shard._doc_lens, oracle._doc_lens)
    assert shard.avgdl == oracle.avgdl
    assert torch.equal(shard.global_ids, oracle.global_ids)
    assert torch.equal(shard.attrs, oracle.attrs)
    assert torch.equal(shard.embeddings, oracle.embeddings)
    a = shard.search(QUERIES, None, k=50)
    b = oracle.search(QUERIES, None, k=50)
    assert torch.equal(a.bm25_scores, b.bm25_scores)
    assert torch.equal(a.bm25_ids, b.bm25_ids)


def test_manifest_keeps_attributes_and_tombstones(tmp_path):
    shard, *_ = _two_segment_shard()
    shard.delete([1003, 1250])
    save_shard(shard, tmp_path / "s.pt")
    loaded = load_shard(tmp_path / "s.pt", device="cpu")
    assert torch.equal(loaded.attrs, shard.attrs) and loaded.n_dead == 2
    f = [DocFilter(language="en")]
    a = shard.search(QUERIES[:1], None, k=40, filters=f)
    b = loaded.search(QUERIES[:1], None, k=40, filters=f)
    assert torch.equal(a.bm25_ids, b.bm25_ids)
    assert not ({1003, 1250} & set(b.bm25_ids.flatten().tolist()))


def test_manifest_without_attributes_loads(tmp_path):
    shard, *_ = _two_segment_shard()
    p = tmp_path / "old.pt"
    save_shard(shard, p)
    blob = torch.load(p, map_location="cpu", weights_only=False)
    del blob["attrs"]                        # as written before attributes
    torch.save(blob, p)
    loaded = load_shard(p, device="cpu")
    assert loaded.n_dead == 0
    assert torch.equal(loaded.attrs, torch.zeros(N_DOCS, 4, dtype=torch.int32))
    a = shard.search(QUERIES, None, k=10)
    b = loaded.search(QUERIES, None, k=10)
    assert torch.equal(a.bm25_ids, b.bm25_ids)
    assert loaded.delete([1001]) == 1        # and it can still delete


def test_hbm_bytes_counts_the_attribute_buffer():
    shard, *_ = _two_segment_shard()
    buf = shard._attr_buf
    assert buf.shape[1] == 4 and buf.dtype == torch.int32
    without = sum(s.hbm_bytes() for s in shard.segments) + sum(
        t.numel() * t.element_size()
        for t in (shard._emb_buf, shard._gid_buf))
    assert shard.hbm_bytes() == without + buf.numel() * 4


# ---------------------------------------------------------------- engine

def _engine_with(docs):
    eng = HybridEngine(device="cpu", use_encoder=False)
    for d in docs:
        eng.add_document(d)
    return eng


def test_engine_delete_pending_and_built():
    docs = [Document(url=f"https://x.org/{i}", doc_id=i + 1,
                     title=f"doc {i}", text=f"zebra stripes number{i}")
            for i in range(6)]
    eng = _engine_with(docs[:4])
    eng.flush()
    eng.add_document(docs[4])
    eng.add_document(docs[5])
    assert eng.delete_documents([2, 6]) == 2      # one built, one pending
    assert eng.pending_count == 1 and eng.stats()["docs_dead"] == 1
    ids = [h.doc_id for h in eng.search("zebra", limit=10)]
    assert sorted(ids) == [1, 3, 4]               # visible with no flush
    eng.flush()
    ids = [h.doc_id for h in eng.search("zebra", limit=10)]
    assert sorted(ids) == [1, 3, 4, 5]


def test_engine_recrawl_replaces_its_predecessor():
    docs = [Document(url=f"https://x.org/{i}", doc_id=i + 1, title="t",
                     text=f"common words plus unique{i}") for i in range(5)]
    docs[2].text = "common words plus oldtopic"
    eng = _engine_with(docs)
    eng.flush()
    assert [h.doc_id for h in eng.search("oldtopic", limit=5)][0] == 3
    eng.add_document(Document(url="https://x.org/2", doc_id=3, title="t",
                              text="common words plus newtopic"))
    eng.flush()
    bm = eng.shard.search([bm25_term_ids("oldtopic")], None, k=5)
    assert not (bm.bm25_scores > 0).any(), "stale text still ranks"
    new = [h.doc_id for h in eng.search("newtopic", limit=5)]
    assert new[0] == 3
    everything = [h.doc_id for h in eng.search("common words", limit=10)]
    assert everything.count(3) == 1 and sorted(everything) == [1, 2, 3, 4, 5]


def test_engine_filters_per_query():
    docs = [Document(url=f"https://{d}/p{i}", doc_id=10 * j + i + 1,
                     title="t", text="shared topic text", language=LANGS[i % 3],
                     crawled_at=T0 + i)
            for j, d in enumerate(DOMAINS[:2]) for i in range(6)]
    eng = _engine_with(docs)
    eng.flush()
    out = eng.search_many(
        ["shared topic", "shared topic", "shared topic"], limit=20,
        filters=[DocFilter(site="b.org"), DocFilter(language="fr"), None])
    assert sorted(h.doc_id for h in out[0]) == [11, 12, 13, 14, 15, 16]
    assert sorted(h.doc_id for h in out[1]) == [3, 6, 13, 16]
    assert len(out[2]) == 12


# -------------------------------------------------------------- services

SERVICE_CORPUS = [
    ("https://kernel.org/sched", "CFS scheduler",
     "The completely fair scheduler balances runnable tasks on cores."),
    ("https://kernel.org/rt", "Realtime scheduler",
     "The deadline scheduler serves realtime tasks first."),
    ("https://lwn.net/sched", "Scheduler news",
     "A new scheduler class was merged for the next release."),
    ("https://rocm.docs/queues", "Hardware queues",
     "The hardware scheduler maps queues onto compute units."),
    ("https://pytorch.org/sched", "LR scheduler",
     "A learning rate scheduler decays the step size over epochs."),
]


@pytest.fixture()
def ctx():
    cfg = dataclasses.replace(Config(), gpu=GpuConfig(filters=True))
    c = AppContext.create(config=cfg, with_engine=True, with_worker=False,
                          in_memory=True)
    assert c.engine is not None and c.batcher is not None
    for url, title, text in SERVICE_CORPUS:
        c.index_document(Document(url=url, title=title, text=text),
                         attest=False, credit=False)
    c.flush_engine()
    yield c
    c.close()


def test_filters_flag_reachable_from_env_and_toml(tmp_path):
    from infomesh_amd.config import load_config
    assert Config().gpu.filters is False
    none = tmp_path / "none.toml"
    assert not load_config(none, env={}).gpu.filters
    assert load_config(none, env={"INFOMESH_GPU_FILTERS": "true"}).gpu.filters
    toml = tmp_path / "config.toml"
    toml.write_text("[gpu]\nfilters = true\n")
    assert load_config(toml, env={}).gpu.filters


def test_filtered_query_runs_on_the_engine(ctx):
    before = ctx.batcher.stats()["queries"]
    resp = ctx.search("scheduler site:kernel.org", use_cache=False,
                      deduct=False)
    assert ctx.batcher.stats()["queries"] == before + 1
    assert sorted(h.url for h in resp.results) == [
        "https://kernel.org/rt", "https://kernel.org/sched"]


def _engine_urls(ctx, query, limit):
    return [h.url for h in ctx.search(query, limit=limit, use_cache=False,
                                      deduct=False).results]


def test_remove_url_reaches_the_engine_without_a_flush(ctx):
    from infomesh_amd.mcp.handlers import Handlers
    assert "https://lwn.net/sched" in _engine_urls(ctx, "scheduler", 4)
    Handlers(ctx).remove_url(url="https://lwn.net/sched")
    assert ctx.engine.stats()["docs_dead"] == 1
    urls = _engine_urls(ctx, "scheduler", 4)
    assert "https://lwn.net/sched" not in urls
    assert len(urls) == 4, "a deleted document must not leave a hole"
    raw = ctx.engine.search("scheduler", limit=4)
    assert len(raw) == 4


def test_gdpr_domain_and_dmca_takedown_reach_the_engine(ctx):
    ctx.deletions.request_deletion("domain:kernel.org")
    urls = _engine_urls(ctx, "scheduler", 5)
    assert urls and not any("kernel.org" in u for u in urls)
    ctx.takedowns.file_notice("https://pytorch.org/sched", "copyright", "x")
    assert ctx.takedowns.apply_pending() == 1
    urls = _engine_urls(ctx, "scheduler", 5)
    assert sorted(urls) == ["https://lwn.net/sched", "https://rocm.docs/queues"]
    assert ctx.engine.stats()["docs_dead"] == 3


# ------------------------------------------------- 2-process gloo plane

def _plane_shard(rank: int, world: int) -> CpuShard:
    toks, meta, emb = _corpus(seed=5 + rank)
    shard = CpuShard()
    flat = np.concatenate(toks)
    shard.build_from_arrays(
        flat, np.repeat(np.arange(N_DOCS), [len(t) for t in toks]),
        np.array([len(t) for t in toks]),
        np.arange(N_DOCS, dtype=np.int64) * world + rank, emb,
        attrs=[pack_attrs(l, d, c) for l, d, c in meta])
    return shard


def _filter_worker(rank: int, world: int, port: int, out_file: str):
    os.environ["HIP_VISIBLE_DEVICES"] = "-1"
    os.environ["CUDA_VISIBLE_DEVICES"] = "-1"
    assert not torch.cuda.is_available(), "GPUs still visible to the worker"
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    fabric = Fabric(backend="gloo")
    plane = DistributedQueryPlane(_plane_shard(rank, world), fabric,
                                  k_per_shard=40)
    filters = [DocFilter(language="de", site="c.org"), None,
               DocFilter(after=T0 + 250)]
    terms = [np.array([1, 2, 3]), np.array([4, 5]), np.array([7])]
    emb = torch.nn.functional.normalize(
        torch.randn(3, 16, generator=torch.Generator().manual_seed(2)), dim=-1)
    fused = plane.search_batch(terms if rank == 0 else None,
                               emb if rank == 0 else None, B=3, dim=16,
                               n_results=30,
                               filters=filters if rank == 0 else None)
    if rank == 0:
        torch.save({"bm": fused.bm25_ids, "dn": fused.dense_ids}, out_file)
    else:
        assert fused is None
    fabric.destroy()


def test_plane_gloo_rank1_receives_rank0_predicates(tmp_path):
    import torch.multiprocessing as mp
    out_file = str(tmp_path / "ids")
    mpc = mp.get_context("spawn")
    procs = [mpc.Process(target=_filter_worker, args=(r, 2, 29557, out_file))
             for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    got = torch.load(out_file, weights_only=True)
    _, meta, _ = _corpus()                       # meta is seed-independent
    filters = [DocFilter(language="de", site="c.org"), None,
               DocFilter(after=T0 + 250)]
    for ids in (got["bm"], got["dn"]):
        for qi, f in enumerate(filters):
            row = ids[qi][ids[qi] >= 0]
            by_rank = {r: row[row % 2 == r] // 2 for r in (0, 1)}
            # rank 1's shard answered, and only with passing documents:
            # it can only have known the predicate from the broadcast
            assert len(by_rank[1]) > 0
            for r in (0, 1):
                for local in by_rank[r].tolist():
                    l, d, c = meta[local]
                    assert _brute_pass((c, l, d, False), f), (qi, r, local)
        # the unfiltered row fills up; the narrow one cannot: 20 of a
        # shard's 300 documents are "de" on c.org, fewer than k = 40
        assert (ids[1] >= 0).all()
        assert int((ids[0] >= 0).sum()) == 40
