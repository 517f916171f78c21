"""GPU tests for domain allow/block lists: the list kernel of
docfilter.hip against its numpy oracle and against the plain kernel, and
GpuShard list filters against the CpuShard oracle (MI355X only)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from infomesh_amd.ops import _build
    _build.build()
from infomesh_amd.index.doc_attrs import (DEAD_BIT, DocFilter, lang16,
                                          pack_attrs, pack_pred,
                                          pack_pred_sets, words_i32)
from infomesh_amd.ops import kernels as K
from infomesh_amd.ops import reference as R


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.manual_seed(0)


LANGS = ["en", "de", "fr"]
DOMAINS = ["a.org", "b.org", "c.org", "d.org", "e.org"]
T0 = 1_700_000_000

# the hashes a signed compare orders wrongly
EDGES = [0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
_RNG = np.random.default_rng(42)
# the w2 values documents take: the edges and 60 others, half above 2^31
POOL = EDGES + sorted(set(_RNG.integers(1, 0xFFFFFFFF, size=60).tolist()))
# values no document has, to fill the long lists
FILL = sorted(set(_RNG.integers(1, 0xFFFFFFFF, size=2100).tolist())
              - set(POOL))


def _attrs(n: int) -> np.ndarray:
    """[n, 4] records with w2 written directly from POOL."""
    rng = np.random.default_rng(n)
    a = np.zeros((n, 4), dtype=np.uint32)
    a[:, 0] = T0 + np.arange(n)
    a[:, 1] = [lang16([None, *LANGS][int(i)]) for i in rng.integers(0, 4, n)]
    a[:, 1] |= np.where(rng.integers(0, 6, size=n) == 0, DEAD_BIT,
                        0).astype(np.uint32)
    a[:, 2] = np.asarray(POOL, dtype=np.uint32)[rng.integers(0, len(POOL), n)]
    # a live hit on the first entry of the edge lists, one on the last,
    # and a dead document in an allowed domain
    a[0, 1:3] = (0, 0)
    if n > 2:
        a[1, 1:3] = (0, 0xFFFFFFFF)
    if n > 1:
        a[n - 1, 1:3] = (DEAD_BIT, 0xFFFFFFFF)
    return a.view(np.int32)


def _u(*parts) -> tuple[int, ...]:
    return tuple(sorted({int(v) for p in parts for v in p}))


def _list_preds(size: str, P: int):
    """P predicates in the forwarded form (words, allow, block); in a
    batch of three the middle one carries no list."""
    de = pack_pred(DocFilter(language="de"))
    live = pack_pred(None)
    dated = pack_pred(DocFilter(after=T0 + 3, before=T0 + 3000))
    if size == "1":
        first = (live, (0x80000000,), ())
        last = (dated, (), (0x7FFFFFFF,))
    elif size == "2":
        first = (live, (0, 0xFFFFFFFF), ())       # both entries are hits
        last = (dated, (0x7FFFFFFF,), (0x80000000,))
    else:                                         # 2048 in all
        allow = _u(EDGES, POOL[4:34], FILL[:1470])
        block = _u(POOL[30:40], FILL[1470:2004])
        assert len(allow) + len(block) == 2048 and allow[0] == 0 \
            and allow[-1] == 0xFFFFFFFF
        first = (live, allow, block)
        blk = _u(EDGES[1:3], POOL[10:50], FILL[:2006])
        assert len(blk) == 2048
        last = (dated, (), blk)
    return [pack_pred_sets(p) for p in ([first, (de, (), ()), last][:P]
                                        if P == 3 else [first])]


def _tables(packed):
    desc, flat = [], []
    for _, allow, block in packed:
        desc.append((len(flat), len(allow), len(flat) + len(allow),
                     len(block)))
        flat += list(allow) + list(block)
    return (torch.from_numpy(words_i32([w for w, _, _ in packed])),
            torch.tensor(desc, dtype=torch.int32).reshape(-1, 4),
            torch.from_numpy(np.asarray(flat, dtype=np.uint32).view(np.int32)))


# wave (64), workgroup chunk (2048) and tail boundaries
SIZES_N = [1, 63, 64, 65, 2047, 2048, 2049, 4099]


@pytest.mark.parametrize("size", ["1", "2", "2048"])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("N", SIZES_N)
def test_filter_bitmask_sets_bit_exact(N, P, size):
    attrs = torch.from_numpy(_attrs(N))
    preds, desc, doms = _tables(_list_preds(size, P))
    want = R.filter_bitmask_sets(attrs, preds, desc, doms)
    # poison the allocator's next block: words past N must be WRITTEN 0
    W = (N + 63) // 64 * 2
    junk = torch.full((P, W), -1, device="cuda", dtype=torch.int32)
    del junk
    got = K.filter_bitmask_sets(attrs.cuda(), preds.cuda(), desc.cuda(),
                                doms.cuda())
    assert got.shape == (P, W) and got.dtype == torch.int32
    assert torch.equal(got.cpu(), want)
    if N > 2 and size == "2":
        # the first and the last entry both hit; the dead document in an
        # allowed domain does not
        row = want.numpy().view(np.uint32)[0]
        assert row[0] & 3 == 3
        assert not (row[(N - 1) >> 5] >> ((N - 1) & 31)) & 1


def test_desc_is_checked_before_the_launch():
    attrs = torch.from_numpy(_attrs(65)).cuda()
    preds, desc, doms = _tables(_list_preds("2", 1))
    for bad in ([0, 3, 0, 0], [0, 2, 1, 2], [-1, 1, 0, 0], [0, -1, 0, 0]):
        with pytest.raises(AssertionError):
            K.filter_bitmask_sets(attrs, preds.cuda(),
                                  torch.tensor([bad], dtype=torch.int32),
                                  doms.cuda())
    big = torch.zeros(2049, dtype=torch.int32, device="cuda")
    with pytest.raises(AssertionError):
        K.filter_bitmask_sets(attrs, preds.cuda(),
                              torch.tensor([[0, 2049, 0, 0]],
                                           dtype=torch.int32), big)


PLAIN = [DocFilter(language="de", site="c.org", after=T0 + 10,
                   before=T0 + 3000),
         None,
         DocFilter(after=T0 + 64, before=T0 + 64)]


@pytest.mark.parametrize("N", [65, 4099])
def test_empty_lists_equal_the_plain_kernel(N):
    rng = np.random.default_rng(N)
    a = words_i32([pack_attrs([None, *LANGS][int(rng.integers(0, 4))],
                              DOMAINS[int(rng.integers(0, 5))], T0 + i)
                   for i in range(N)])
    a[:, 1] |= np.where(rng.integers(0, 6, size=N) == 0, DEAD_BIT,
                        0).astype(np.int32)
    attrs = torch.from_numpy(a).cuda()
    preds = torch.from_numpy(words_i32([pack_pred(f) for f in PLAIN])).cuda()
    desc = torch.zeros(3, 4, dtype=torch.int32)
    doms = torch.zeros(0, dtype=torch.int32, device="cuda")
    got = K.filter_bitmask_sets(attrs, preds, desc, doms)
    assert torch.equal(got, K.filter_bitmask(attrs, preds))


# -------------------------------------------------- GpuShard vs CpuShard

N_DOCS, SEG0, DIM = 3000, 1800, 64
DEAD = list(range(5000, 5000 + N_DOCS, 30))


def _corpus():
    rng = np.random.default_rng(9)
    toks = [rng.integers(0, 2000, size=rng.integers(5, 40)).astype(np.int64)
            for _ in range(N_DOCS)]
    meta = [(LANGS[i % 3], DOMAINS[(i // 3) % 5], T0 + i)
            for i in range(N_DOCS)]
    emb = torch.nn.functional.normalize(
        torch.randn(N_DOCS, DIM, generator=torch.Generator().manual_seed(9)),
        dim=-1).bfloat16()
    return toks, meta, emb


def _build_shard(cls, toks, meta, emb, **kw):
    shard = cls(**kw)
    for lo, hi in ((0, SEG0), (SEG0, N_DOCS)):
        for i in range(lo, hi):
            shard.add_document(5000 + i, toks[i], emb[i],
                               attrs=pack_attrs(*meta[i]))
        shard.build()
    assert shard.delete(DEAD) == len(DEAD)
    return shard


@pytest.fixture(scope="module")
def shards():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infomesh_amd.index.gpu_index import CpuShard, GpuShard
    toks, meta, emb = _corpus()
    return {"gpu": _build_shard(GpuShard, toks, meta, emb, device="cuda"),
            "cpu": _build_shard(CpuShard, toks, meta, emb), "meta": meta}


def _queries():
    rng = np.random.default_rng(17)
    terms = [rng.integers(0, 2000, size=3).astype(np.int64) for _ in range(4)]
    # bf16-representable queries: both planes then multiply the same
    # numbers and differ only in fp32 summation order
    q = torch.nn.functional.normalize(
        torch.randn(4, DIM, generator=torch.Generator().manual_seed(17)),
        dim=-1).bfloat16().float()
    return terms, q


def test_gpu_shard_list_filters_match_cpu_shard(shards):
    gpu, cpu, meta = shards["gpu"], shards["cpu"], shards["meta"]
    terms, q = _queries()
    k = 50
    filters = [DocFilter(sites=("a.org", "c.org")),                  # allow
               DocFilter(exclude_sites=("b.org", "d.org")),          # block
               DocFilter(language="fr", sites=("a.org", "b.org", "e.org"),
                         exclude_sites=("b.org",),
                         after=T0 + 100.5),                          # mixed
               None]
    got = gpu.search(terms, q.cuda(), k=k, filters=filters)
    torch.cuda.synchronize()
    want = cpu.search(terms, q, k=k + 1, filters=filters)
    dead_set = set(DEAD)

    def passes(gid, f):
        l, d, c = meta[gid - 5000]
        return (gid not in dead_set
                and (f is None or (
                    (not f.language or f.language == l)
                    and (not f.sites or d in f.sites)
                    and d not in f.exclude_sites
                    and (f.after is None or c >= np.ceil(f.after)))))
    for ids in (got.bm25_ids.cpu(), got.dense_ids.cpu()):
        for qi, f in enumerate(filters):
            row = ids[qi][ids[qi] >= 0].tolist()
            assert len(row) == k and len(set(row)) == k
            assert all(passes(g, f) for g in row), (qi, f)
    # BM25: scores to the segment tests' tolerance; ids where the oracle's
    # neighbours are further apart than that tolerance can reorder
    ws, wi = want.bm25_scores, want.bm25_ids
    assert torch.allclose(got.bm25_scores.cpu(), ws[:, :k], atol=1e-4)
    gap = (ws[:, :-1] - ws[:, 1:]).abs() > 1e-3          # [B, k]
    untied = gap.clone()
    untied[:, 1:] &= gap[:, :-1]
    assert untied.sum() >= 8, "corpus too tied to check ids"
    assert torch.equal(got.bm25_ids.cpu()[untied], wi[:, :k][untied])
    # dense: 64 fp32 products of magnitude <= 1 per score, so summation
    # order moves a score by ~64 * 2^-24, far inside 1e-4
    assert torch.allclose(got.dense_scores.cpu(), want.dense_scores[:, :k],
                          atol=1e-4)


def test_batches_without_lists_still_call_the_plain_kernel(shards,
                                                           monkeypatch):
    gpu = shards["gpu"]
    terms, q = _queries()
    calls = []
    real_sets = K.filter_bitmask_sets

    def no_sets(*a, **kw):
        raise AssertionError("list kernel called for a batch without lists")

    def plain(*a, _real=K.filter_bitmask, **kw):
        calls.append("plain")
        return _real(*a, **kw)
    monkeypatch.setattr(K, "filter_bitmask_sets", no_sets)
    monkeypatch.setattr(K, "filter_bitmask", plain)
    gpu._live_bits = None
    gpu.search(terms, q.cuda(), k=20)                 # tombstones only
    assert calls == ["plain"]
    gpu.search(terms, q.cuda(), k=20,
               filters=[DocFilter(site="c.org"), None,
                        DocFilter(language="de"), None])
    assert calls == ["plain", "plain"]
    # and a batch with a list takes the list kernel, once for both planes

    def sets(*a, **kw):
        calls.append("sets")
        return real_sets(*a, **kw)
    monkeypatch.setattr(K, "filter_bitmask_sets", sets)
    gpu.search(terms, q.cuda(), k=20,
               filters=[DocFilter(sites=("c.org",)), None, None, None])
    torch.cuda.synchronize()
    assert calls == ["plain", "plain", "sets"]
