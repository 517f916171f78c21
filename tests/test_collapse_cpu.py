"""CPU tests for the per-domain cap: the sort-and-count oracle against a
brute-force double loop; cap_per_domain on hand-written cases; the merge
property the query plane relies on (capping the shards' capped lists
gives the whole corpus's capped list); CpuShard.search(per_domain=...)
against the oracle; the persite:N token."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import term_ops_corpus as C
from infomesh_amd.index.gpu_index import (COLLAPSE_M_MAX, CpuShard,
                                          per_domain_caps)
from infomesh_amd.ops import reference as R
from infomesh_amd.parallel.query_plane import (cap_per_domain,
                                               lookup_domains)
from infomesh_amd.search.nlp import (PERSITE_MAX, parse_persite_token,
                                     with_persite_token)

NEG = -float("inf")


def _bits(ok: np.ndarray) -> torch.Tensor:
    """bool [P, N] -> the mask words the kernels read."""
    P, N = ok.shape
    W = (N + 31) // 32
    full = np.zeros((P, W * 32), dtype=bool)
    full[:, :N] = ok
    return torch.from_numpy(np.packbits(full, axis=1, bitorder="little")
                            .view(np.uint32).reshape(P, W).view(np.int32))


def _brute(s, ok, dom, m, k, positive):
    """The contract, one document at a time: x is in the result iff it is
    eligible, fewer than m eligible documents of its domain stand before
    it, and fewer than k such documents of any domain do."""
    okey = R.ordered_key(torch.from_numpy(s)).numpy()
    N = len(s)
    elig = [d for d in range(N) if ok[d] and (s[d] > 0 or not positive)]

    def before(a, b):                   # a stands before b
        return (okey[a], -a) > (okey[b], -b)
    G = [x for x in elig
         if sum(1 for y in elig if dom[y] == dom[x] and before(y, x)) < m]
    out = [x for x in G if sum(1 for y in G if before(y, x)) < k]
    out.sort(key=lambda x: sum(1 for y in G if before(y, x)))
    return out


@pytest.mark.parametrize("positive", [True, False], ids=["bm25", "dense"])
def test_oracle_against_the_double_loop(positive):
    rng = np.random.default_rng(3 + positive)
    N, B = 41, 3
    vals = np.asarray([0.0, -0.0, -1.0, 0.5, 0.5, 2.0, np.inf, -np.inf],
                      dtype=np.float32)
    s = rng.choice(vals, size=(B, N))
    dom = rng.integers(0, 5, size=N).astype(np.int32)
    ok = rng.random((2, N)) < 0.7
    row_pred = torch.tensor([1, 0, 1], dtype=torch.int32)
    rows = torch.tensor([2, 0], dtype=torch.int32)
    for mask in (None, _bits(ok)):
        for m in (1, 2, 4):
            for k in (1, 6, 60):
                v, i = R.collapse_topk(
                    torch.from_numpy(s), rows, torch.from_numpy(dom), m, k,
                    positive, mask=mask,
                    row_pred=None if mask is None else row_pred)
                assert v.dtype == torch.float32 and i.dtype == torch.int32
                for r, b in enumerate(rows.tolist()):
                    passing = ok[row_pred[b]] if mask is not None \
                        else np.ones(N, dtype=bool)
                    want = _brute(s[b], passing, dom, m, k, positive)
                    assert i[r, :len(want)].tolist() == want
                    assert (i[r, len(want):] == -1).all()
                    assert (v[r, len(want):] == NEG).all()
                    assert v[r, :len(want)].view(torch.int32).tolist() == \
                        torch.from_numpy(s[b, want]).view(torch.int32).tolist()


def test_cap_per_domain_by_hand():
    ids = torch.tensor([[5, 3, 9, -1, 7, 2],
                        [1, 2, 3, 4, -1, -1]])
    sc = torch.tensor([[1.0, 3.0, 3.0, NEG, 2.0, NEG],
                       [4.0, 3.0, 2.0, 1.0, NEG, NEG]])
    dm = torch.tensor([[8, 8, 6, 0, 8, 6],
                       [0, 0, 0, 0, 0, 0]], dtype=torch.int32)
    # row 0 sorted: 3 (3.0, dom 8), 9 (3.0, 6), 7 (2.0, 8), 5 (1.0, 8),
    # 2 (-inf, 6: a real hit whose score is -inf), pad
    i, s, d = cap_per_domain(ids, sc, dm, torch.tensor([1, 2]), 4)
    assert i.tolist() == [[3, 9, -1, -1], [1, 2, -1, -1]]
    assert s.tolist() == [[3.0, 3.0, NEG, NEG], [4.0, 3.0, NEG, NEG]]
    assert d.tolist() == [[8, 6, 0, 0], [0, 0, 0, 0]]
    i, s, d = cap_per_domain(ids, sc, dm, torch.tensor([2, 0]), 6)
    assert i.tolist() == [[3, 9, 7, 2, -1, -1], [1, 2, 3, 4, -1, -1]]
    assert d[0].tolist() == [8, 6, 8, 6, 0, 0]
    # n cuts behind the cap; m = 0 only sorts
    i, s, d = cap_per_domain(ids, sc, dm, torch.tensor([0, 0]), 3)
    assert i.tolist() == [[3, 9, 7], [1, 2, 3]]
    # the pairs' lookup, pads included
    got = lookup_domains(torch.tensor([[9, -1, 5], [4, 1, -1]]), ids, dm)
    assert got.tolist() == [[6, 0, 8], [0, 0, 0]]


def _shard_lists(s, dom, gids, parts, m, k):
    """Per-part oracle lists of one row, as the shards return them:
    (global ids, scores, domains), each [1, W * k]."""
    ids, sc, dm = [], [], []
    for cols in parts:
        v, i = R.collapse_topk(
            torch.from_numpy(s[cols][None]),
            torch.tensor([0], dtype=torch.int32),
            torch.from_numpy(dom[cols]), m, k, False)
        real = i[0] >= 0
        at = torch.from_numpy(cols)[i[0].clamp(min=0).long()]
        ids.append(torch.where(real, torch.from_numpy(gids)[at], -1))
        sc.append(v[0])
        dm.append(torch.where(real, torch.from_numpy(dom)[at], 0))
    return (torch.cat(ids)[None], torch.cat(sc)[None], torch.cat(dm)[None])


@pytest.mark.parametrize("m", [1, 2, 4])
def test_capping_the_shards_lists_gives_the_whole_corpus_list(m):
    rng = np.random.default_rng(40 + m)
    N, W, k, D = 600, 3, 25, 37
    # distinct scores; global ids ascend with the column, as the merge's
    # tie-break would need them to if scores could tie
    s = rng.permutation(N).astype(np.float32) - 100.0
    dom = np.minimum(rng.zipf(1.4, size=N), D).astype(np.int32)
    gids = (np.arange(N) * 3 + 11).astype(np.int64)
    parts = np.array_split(rng.permutation(N), W)
    parts = [np.sort(p) for p in parts]
    ids, sc, dm = _shard_lists(s, dom, gids, parts, m, k)
    got = cap_per_domain(ids, sc, dm, torch.tensor([m]), k)
    v, i = R.collapse_topk(torch.from_numpy(s[None]),
                           torch.tensor([0], dtype=torch.int32),
                           torch.from_numpy(dom), m, k, False)
    assert got[0][0].tolist() == gids[i[0].numpy()].tolist()
    assert torch.equal(got[1][0], v[0])
    assert got[2][0].tolist() == dom[i[0].numpy()].tolist()


def test_a_cap_of_n_is_the_plain_top_k():
    rng = np.random.default_rng(50)
    N, W, k = 300, 3, 20
    s = rng.permutation(N).astype(np.float32)
    dom = rng.integers(0, 4, size=N).astype(np.int32)
    gids = np.arange(N, dtype=np.int64) + 5
    parts = [np.sort(p) for p in np.array_split(rng.permutation(N), W)]
    ids, sc, dm = [], [], []
    for cols in parts:                       # the shards' plain top-k
        v, i = torch.topk(torch.from_numpy(s[cols]), k)
        ids.append(torch.from_numpy(gids[cols])[i])
        sc.append(v)
        dm.append(torch.from_numpy(dom[cols])[i])
    got = cap_per_domain(torch.cat(ids)[None], torch.cat(sc)[None],
                         torch.cat(dm)[None], torch.tensor([N]), k)
    v, i = torch.topk(torch.from_numpy(s), k)
    assert got[0][0].tolist() == gids[i.numpy()].tolist()
    assert torch.equal(got[1][0], v)


def test_merge_with_heavy_ties():
    """Shards break ties by local column, the merge by global id: equal
    score multisets, and no domain over its cap."""
    rng = np.random.default_rng(60)
    N, W, k, m = 500, 3, 30, 2
    s = rng.integers(1, 6, size=N).astype(np.float32)
    dom = rng.integers(0, 40, size=N).astype(np.int32)
    gids = rng.permutation(N).astype(np.int64)   # unrelated to the column
    parts = [np.sort(p) for p in np.array_split(rng.permutation(N), W)]
    ids, sc, dm = _shard_lists(s, dom, gids, parts, m, k)
    got = cap_per_domain(ids, sc, dm, torch.tensor([m]), k)
    v, _ = R.collapse_topk(torch.from_numpy(s[None]),
                           torch.tensor([0], dtype=torch.int32),
                           torch.from_numpy(dom), m, k, False)
    assert (got[0][0] >= 0).all()
    assert torch.equal(got[1][0], v[0])          # sorted: equal multisets
    assert np.bincount(got[2][0].numpy()).max() <= m
    col = {int(g): c for c, g in enumerate(gids)}
    assert [int(dom[col[int(g)]]) for g in got[0][0]] == got[2][0].tolist()


# ------------------------------------------------------------- CpuShard

@pytest.fixture(scope="module")
def shard():
    toks, meta, emb = C.corpus()
    return C.build_shard(CpuShard, toks, meta, emb)


def test_cpu_shard_per_domain_against_the_oracle(shard):
    terms, q, filters, ops = C.queries()
    B, k = len(terms), C.K_CMP
    caps = [2, 0, 1, 4, 1, None]
    plain = shard.search(terms, q, k=k, filters=filters, term_ops=ops)
    got = shard.search(terms, q, k=k, filters=filters, term_ops=ops,
                       per_domain=caps)
    assert plain.bm25_dom is None and plain.dense_dom is None
    # the scores the shard ranks, once more: k = N returns every passing
    # document, and the rest of the row failed the mask
    N = shard.n_docs
    full = shard.search(terms, q, k=N, filters=filters, term_ops=ops)
    dom_keys, dom_id = shard._domain_tables()
    gid = shard.global_ids
    for plane, positive in (("bm25", True), ("dense", False)):
        ids, sc = getattr(got, plane + "_ids"), getattr(got, plane + "_scores")
        f_ids = getattr(full, plane + "_ids")
        f_sc = getattr(full, plane + "_scores")
        doms = getattr(got, plane + "_dom")
        assert doms.dtype == torch.int32 and doms.shape == (B, k)
        for b, m in enumerate(caps):
            if not m:
                assert torch.equal(ids[b], getattr(plain, plane + "_ids")[b])
                assert torch.equal(sc[b], getattr(plain, plane + "_scores")[b])
                continue
            # the row's scores and mask, rebuilt from the full list
            s = torch.zeros(1, N)
            ok = np.zeros((1, N), dtype=bool)
            real = f_ids[b] >= 0
            cols = (f_ids[b][real] - C.GID0).long()
            assert torch.equal(gid[cols], f_ids[b][real])
            s[0, cols] = f_sc[b][real]
            ok[0, cols.numpy()] = True
            v, i = R.collapse_topk(
                s, torch.tensor([0], dtype=torch.int32), dom_id, m, k,
                positive, mask=_bits(ok),
                row_pred=torch.tensor([0], dtype=torch.int32))
            want = torch.where(i[0] >= 0, gid[i[0].clamp(min=0).long()], -1)
            assert ids[b].tolist() == want.tolist(), (plane, b)
            assert torch.equal(sc[b], v[0]), (plane, b)
            hit = ids[b] >= 0
            assert int(hit.sum()) > 0
            w2 = shard.attrs[:, 2][(ids[b][hit] - C.GID0).long()]
            assert doms[b][hit].tolist() == w2.tolist()
            assert not doms[b][~hit].any()
            assert np.unique(w2.numpy(), return_counts=True)[1].max() <= m
    # the cap bites somewhere: four domains, k = 20
    assert not torch.equal(got.bm25_ids[3], plain.bm25_ids[3]) or \
        not torch.equal(got.dense_ids[3], plain.dense_ids[3])
    assert int((got.dense_ids[0] >= 0).sum()) <= 2 * len(C.DOMAINS)


def test_caps_out_of_range_are_value_errors(shard):
    terms, q, _, _ = C.queries()
    assert COLLAPSE_M_MAX == PERSITE_MAX == 4
    assert per_domain_caps(None, 3) is None
    assert per_domain_caps([0, None, 0], 3) is None
    assert per_domain_caps([0, None, 3], 3) == [0, 0, 3]
    for bad in ([5] + [0] * 5, [-1] + [0] * 5):
        with pytest.raises(ValueError, match="per_domain"):
            shard.search(terms, q, k=5, per_domain=bad)


# ---------------------------------------------------------------- token

def test_persite_token_round_trip():
    for m in range(1, PERSITE_MAX + 1):
        sent = with_persite_token("rust async site:a.org,b.org", m)
        assert sent.endswith(f"persite:{m}")
        assert parse_persite_token(sent) == ("rust async site:a.org,b.org", m)
    assert with_persite_token("rust", 0) == "rust"
    assert with_persite_token("rust", None) == "rust"
    assert parse_persite_token("rust") == ("rust", 0)
    assert parse_persite_token("persite:2 rust  persite:3 x") == ("rust x", 3)
    # no token: part of a word, or no number
    for text in ("xpersite:2", "persite:2x", "persite:", "persite:-1"):
        assert parse_persite_token(text) == (text, 0)
    for bad in (0, 5, 99):
        with pytest.raises(ValueError, match="persite"):
            parse_persite_token(f"rust persite:{bad}")
        assert parse_persite_token(f"rust persite:{bad}", clamp=True) \
            == ("rust", min(max(bad, 1), PERSITE_MAX))
    for bad in (-1, 5):
        with pytest.raises(ValueError, match="per_domain"):
            with_persite_token("rust", bad)


# ------------------------------------------------ query plane and engine

def test_search_batch_caps_the_planes_and_the_fused_list(shard):
    from infomesh_amd.parallel.fabric import Fabric
    from infomesh_amd.parallel.query_plane import DistributedQueryPlane
    terms, q, filters, ops = C.queries()
    B, n = len(terms), 12
    caps = [2, 0, 1, 4, 1, None]
    plane = DistributedQueryPlane(shard, Fabric(), k_per_shard=C.K_CMP)
    kw = dict(B=B, dim=C.DIM, n_results=n, filters=filters, term_ops=ops)
    plain = plane.search_batch(terms, q, **kw)
    got = plane.search_batch(terms, q, per_domain=caps, **kw)
    hits = shard.search(terms, q, k=C.K_CMP, filters=filters, term_ops=ops,
                        per_domain=caps)
    w2 = shard.attrs[:, 2]
    for b, m in enumerate(caps):
        ids = got.ids[b]
        real = ids >= 0
        assert real.any() and not (got.scores[b][~real] != 0).any()
        if not m:
            assert torch.equal(ids, plain.ids[b])
            assert torch.equal(got.scores[b], plain.scores[b])
            continue
        doms = w2[(ids[real] - C.GID0).long()]
        assert np.unique(doms.numpy(), return_counts=True)[1].max() <= m
        # one shard: its capped lists are the plane's
        assert got.bm25_ids[b].tolist() == hits.bm25_ids[b].tolist()
        assert got.dense_ids[b].tolist() == hits.dense_ids[b].tolist()
        # fused scores descend, and every hit comes from a plane list
        s = got.scores[b][real]
        assert (s[:-1] >= s[1:]).all() and (s > 0).all()
        pool = set(hits.bm25_ids[b].tolist()) | set(hits.dense_ids[b].tolist())
        assert set(ids[real].tolist()) <= pool
    with pytest.raises(ValueError, match="per_domain"):
        plane.search_batch(terms, q, per_domain=[7] * B, **kw)


def test_engine_per_domain_on_the_cpu():
    from infomesh_amd.engine import HybridEngine
    from infomesh_amd.index.local_store import Document
    eng = HybridEngine(device="cpu", use_encoder=False)
    site = {}
    for i in range(60):
        if i < 40:
            site[i] = "big.org"
            text = "rust " * 6 + " ".join([f"note{i}"] * (i + 1))
        else:
            site[i] = f"small{(i - 40) // 2}.net"
            text = "rust " + " ".join(f"filler{i}x{j}" for j in range(30 + i))
        eng.add_document(Document(
            url=f"https://{site[i]}/{i}", title=f"t{i}", text=text,
            doc_id=i, language="en", crawled_at=1000.0 + i))
    eng.flush()
    limit = 10
    plain = eng.search_many(["rust"] * 3, limit=limit)
    capped, same, one = eng.search_many(["rust"] * 3, limit=limit,
                                        per_domain=[2, None, 1])
    assert {site[h.doc_id] for h in plain[0]} == {"big.org"}
    assert [h.doc_id for h in same] == [h.doc_id for h in plain[1]]
    assert [site[h.doc_id] for h in capped[:2]] == ["big.org"] * 2
    assert [h.doc_id for h in capped[:2]] == [h.doc_id for h in plain[0][:2]]
    assert len(capped) == limit
    tally = {}
    for h in capped:
        tally[site[h.doc_id]] = tally.get(site[h.doc_id], 0) + 1
    assert max(tally.values()) <= 2 and len(tally) == 5
    assert len(one) == limit and len({site[h.doc_id] for h in one}) == limit
    with pytest.raises(ValueError, match="per_domain"):
        eng.search_many(["rust"], limit=limit, per_domain=[5])


# ------------------------------------------------------------- services

def _ctx(engine: bool):
    import dataclasses
    from infomesh_amd.config import Config, GpuConfig
    from infomesh_amd.index.local_store import Document
    from infomesh_amd.services import AppContext
    cfg = dataclasses.replace(Config(), gpu=GpuConfig(filters=True))
    c = AppContext.create(config=cfg, with_engine=engine, with_worker=False,
                          in_memory=True)
    for i in range(40):
        # 30 short pages of one site, then ten sites with one longer each
        host = "big.com" if i < 30 else f"s{i}.org"
        c.index_document(Document(
            url=f"https://{host}/p{i}", title=f"page {i}",
            text="zebra " * (6 if i < 30 else 1)
            + " ".join(f"w{i}x{j}" for j in range(i + (0 if i < 30 else 40))),
            language="en"), attest=False, credit=False)
    if engine:
        c.flush_engine()
    return c


@pytest.mark.parametrize("engine", [True, False], ids=["engine", "fts"])
def test_app_context_per_domain(engine):
    c = _ctx(engine)
    try:
        plain = c.search("zebra", limit=8, deduct=False)
        assert {h.domain for h in plain.results} == {"big.com"}
        resp = c.search("zebra", limit=8, deduct=False, per_domain=2)
        assert resp is not plain, "the cache must keep the two apart"
        doms = [h.domain for h in resp.results]
        assert max(doms.count(d) for d in set(doms)) <= 2
        assert doms.count("big.com") == 2
        if engine:
            # exact over the match set: the list fills up from other sites
            assert len(doms) == 8 and len(set(doms)) == 7
        else:
            # FTS: the cap only thins out the hits SQLite returned
            assert len(doms) < 8
        # the typed token asks for the same and shares the cache entry
        assert c.search("zebra persite:2", limit=8, deduct=False) is resp
        assert "persite" not in resp.query + (resp.effective_query or "")
        # the parameter wins over a typed token
        one = c.search("zebra persite:2", limit=8, deduct=False, per_domain=1)
        assert [h.domain for h in one.results].count("big.com") == 1
        for bad in (dict(per_domain=5), dict(per_domain=-1)):
            with pytest.raises(ValueError):
                c.search("zebra", limit=8, deduct=False, **bad)
        with pytest.raises(ValueError, match="persite"):
            c.search("zebra persite:9", limit=8, deduct=False)
    finally:
        c.close()
