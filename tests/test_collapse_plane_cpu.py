"""The per-domain cap across ranks and through the public interface (no
GPU): a 2-rank gloo run of the query plane with capped and uncapped
batches (the caps in the terms broadcast, the extra all-gather, the
merge of two real shards' lists), and per_domain through /search and
MCP web_search."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import term_ops_corpus as C
from infomesh_amd.index.doc_attrs import pack_attrs
from infomesh_amd.index.gpu_index import CpuShard
from infomesh_amd.parallel.fabric import Fabric
from infomesh_amd.parallel.query_plane import (_CAP_BITS, _CAP_SHIFT,
                                               MAX_QUERY_TERMS,
                                               DistributedQueryPlane,
                                               cap_per_domain)

_HALF = 300
CAPS = [2, 0, 1, 4, 1, None]
K_SHARD, N_RES = 20, 10


def _half_shard(lo: int, hi: int) -> CpuShard:
    toks, meta, emb = C.corpus()
    s = CpuShard()
    for i in range(lo, hi):
        s.add_document(C.GID0 + i, toks[i], emb[i],
                       attrs=pack_attrs(*meta[i]))
    s.build()
    s.delete([g for g in C.DEAD if lo <= g - C.GID0 < hi])
    return s


class _RecordingFabric:
    """Forwards to a Fabric, counts its collectives and keeps a copy of
    every broadcast tensor as it is after the broadcast."""

    def __init__(self, fabric):
        self._fabric = fabric
        self.sent, self.gathers = [], 0

    def broadcast(self, t, src=0):
        out = self._fabric.broadcast(t, src)
        self.sent.append(t.detach().cpu().clone())
        return out

    def all_gather(self, t):
        self.gathers += 1
        return self._fabric.all_gather(t)

    def __getattr__(self, name):
        return getattr(self._fabric, name)


def _worker(rank: int, port: int, out_dir: str):
    os.environ["HIP_VISIBLE_DEVICES"] = "-1"
    os.environ["CUDA_VISIBLE_DEVICES"] = "-1"
    assert not torch.cuda.is_available(), "GPUs still visible to the worker"
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": "2",
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    fabric = _RecordingFabric(Fabric(backend="gloo"))
    lead = rank == 0
    terms, q, filters, ops = C.queries()
    shard = _half_shard(_HALF, C.N_DOCS) if rank else _half_shard(0, _HALF)
    plane = DistributedQueryPlane(shard, fabric, k_per_shard=K_SHARD)

    def run(caps):
        fabric.sent, fabric.gathers = [], 0
        f = plane.search_batch(
            terms if lead else None, q if lead else None, B=6, dim=C.DIM,
            n_results=N_RES, filters=filters if lead else None,
            term_ops=ops if lead else None,
            per_domain=caps if lead else None)
        assert (f is not None) == lead
        return {"fused": None if f is None else {
                    "ids": f.ids, "scores": f.scores, "bm25_ids": f.bm25_ids,
                    "bm25_scores": f.bm25_scores, "dense_ids": f.dense_ids,
                    "dense_scores": f.dense_scores},
                "caps": plane._caps, "sent": fabric.sent,
                "gathers": fabric.gathers}
    torch.save({"capped": run(CAPS), "plain": run(None),
                "zeros": run([0, None, 0, 0, None, 0])},
               os.path.join(out_dir, f"r{rank}"))
    fabric.destroy()


@pytest.fixture(scope="module")
def gloo_run(tmp_path_factory):
    import torch.multiprocessing as mp
    out = tmp_path_factory.mktemp("collapse")
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, 29581, str(out)))
             for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return [torch.load(str(out / f"r{r}"), weights_only=False)
            for r in range(2)]


def test_gloo_caps_reach_every_rank_in_the_terms_broadcast(gloo_run):
    r0, r1 = gloo_run
    want = [m or 0 for m in CAPS]
    assert r0["capped"]["caps"] == want and r1["capped"]["caps"] == want
    for name in ("plain", "zeros"):
        assert r0[name]["caps"] is None and r1[name]["caps"] is None
    # an uncapped batch: the same broadcasts, byte for byte, whether
    # per_domain is absent or names no cap; and the same collectives
    for a, b in zip(r0["plain"]["sent"], r0["zeros"]["sent"]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert len(r0["plain"]["sent"]) == len(r0["zeros"]["sent"]) \
        == len(r0["capped"]["sent"])
    assert r0["plain"]["gathers"] == r0["zeros"]["gathers"]
    # a capped batch: one more all-gather, and a terms tensor that
    # differs from the uncapped one in bits 21..23 of z alone
    assert r0["capped"]["gathers"] == r0["plain"]["gathers"] + 1
    assert r1["capped"]["gathers"] == r1["plain"]["gathers"] + 1
    capped, plain = r0["capped"]["sent"][0], r0["plain"]["sent"][0]
    z = capped[:, MAX_QUERY_TERMS + 1]
    assert ((z & _CAP_BITS) >> _CAP_SHIFT).tolist() == want
    stripped = capped.clone()
    stripped[:, MAX_QUERY_TERMS + 1] = z & ~_CAP_BITS
    assert torch.equal(stripped, plain)
    for a, b in zip(r0["capped"]["sent"], r1["capped"]["sent"]):
        assert torch.equal(a, b)


def test_gloo_capped_batch_merges_the_two_shards_lists(gloo_run):
    r0, _ = gloo_run
    got, plain = r0["capped"]["fused"], r0["plain"]["fused"]
    terms, q, filters, ops = C.queries()
    _, meta, _ = C.corpus()
    halves = [_half_shard(0, _HALF), _half_shard(_HALF, C.N_DOCS)]
    hits = [s.search(terms, q, k=K_SHARD, filters=filters, term_ops=ops,
                     per_domain=CAPS) for s in halves]
    m_row = torch.tensor([m or 0 for m in CAPS])
    for plane in ("bm25", "dense"):
        ids = torch.cat([getattr(h, plane + "_ids") for h in hits], dim=1)
        sc = torch.cat([getattr(h, plane + "_scores") for h in hits], dim=1)
        dm = torch.cat([getattr(h, plane + "_dom") for h in hits], dim=1)
        w_ids, w_sc, _ = cap_per_domain(ids, sc, dm, m_row, 2 * K_SHARD)
        for b, m in enumerate(CAPS):
            if m:
                assert torch.equal(got[plane + "_ids"][b], w_ids[b]), plane
                assert torch.equal(got[plane + "_scores"][b], w_sc[b]), plane
            else:
                # as gathered: rank 0's list, then rank 1's
                assert torch.equal(got[plane + "_ids"][b], ids[b]), plane
    for b, m in enumerate(CAPS):
        ids = got["ids"][b]
        real = ids >= 0
        if not m:
            assert torch.equal(ids, plain["ids"][b])
            assert torch.equal(got["scores"][b], plain["scores"][b])
            continue
        assert real.any()
        doms = [meta[int(g) - C.GID0][1] for g in ids[real]]
        assert max(doms.count(d) for d in set(doms)) <= m
        pool = set(got["bm25_ids"][b].tolist()) \
            | set(got["dense_ids"][b].tolist())
        assert set(ids[real].tolist()) <= pool
        s = got["scores"][b][real]
        assert (s[:-1] >= s[1:]).all() and (s > 0).all()
    # the cap bites across ranks: four domains, cap 1 and cap 2
    assert int((got["ids"][2] >= 0).sum()) <= 4
    assert int((got["dense_ids"][0] >= 0).sum()) <= 8
    assert int((plain["dense_ids"][0] >= 0).sum()) == 2 * K_SHARD


# ------------------------------------------------------- public interface

def _ctx():
    import dataclasses
    from infomesh_amd.config import Config, GpuConfig
    from infomesh_amd.index.local_store import Document
    from infomesh_amd.services import AppContext
    cfg = dataclasses.replace(Config(), gpu=GpuConfig(filters=True))
    c = AppContext.create(config=cfg, with_engine=True, with_worker=False,
                          in_memory=True)
    for i in range(40):
        host = "big.com" if i < 30 else f"s{i}.org"
        c.index_document(Document(
            url=f"https://{host}/p{i}", title=f"page {i}",
            text="zebra " * (6 if i < 30 else 1)
            + " ".join(f"w{i}x{j}" for j in range(i + (0 if i < 30 else 40))),
            language="en"), attest=False, credit=False)
    c.flush_engine()
    return c


def _hosts(results) -> list[str]:
    return [r["url"].split("/")[2] for r in results]


def test_http_route_and_mcp_tool_pass_the_parameter_through():
    from fastapi.testclient import TestClient

    from infomesh_amd.api.local_api import create_app
    from infomesh_amd.mcp.handlers import Handlers
    from infomesh_amd.mcp.tools import TOOLS
    c = _ctx()
    try:
        http = TestClient(create_app(c))
        plain = http.get("/search", params={"q": "zebra", "limit": 8}).json()
        assert set(_hosts(plain["results"])) == {"big.com"}
        body = http.get("/search", params={"q": "zebra", "limit": 8,
                                           "per_domain": 2}).json()
        hosts = _hosts(body["results"])
        assert len(hosts) == 8 and hosts.count("big.com") == 2
        assert len(set(hosts)) == 7
        same = http.get("/search", params={"q": "zebra", "limit": 8,
                                           "per_domain": 0}).json()
        assert same["results"] == plain["results"]
        for bad in (5, -1):
            assert http.get("/search", params={
                "q": "zebra", "per_domain": bad}).status_code == 400
        assert http.get("/search", params={
            "q": "zebra persite:7"}).status_code == 400
        # MCP tool
        props = next(t for t in TOOLS if t["name"] == "web_search")[
            "inputSchema"]["properties"]
        assert props["per_domain"] == {**props["per_domain"],
                                       "type": "integer", "minimum": 0,
                                       "maximum": 4}
        h = Handlers(c)
        out = h.web_search(query="zebra", limit=8)
        assert set(_hosts(out["results"])) == {"big.com"}
        out = h.web_search(query="zebra", limit=8, per_domain=1)
        hosts = _hosts(out["results"])
        assert len(hosts) == 8 and len(set(hosts)) == 8
        with pytest.raises(ValueError):
            h.web_search(query="zebra", limit=8, per_domain=5)
        # the cap rides along with a domain list
        out = h.web_search(query="zebra", limit=8, per_domain=1,
                           domain_blocklist=["s30.org"])
        hosts = _hosts(out["results"])
        assert "s30.org" not in hosts and len(set(hosts)) == len(hosts) == 8
    finally:
        c.close()
