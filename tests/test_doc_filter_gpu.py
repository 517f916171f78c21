"""GPU tests for the document filter: the predicate -> bitmask kernel,
the masked top-k, and GpuShard deletes / filtered search against the
CpuShard oracle (MI355X only)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from infomesh_amd.ops import _build
    _build.build()
from infomesh_amd.index.doc_attrs import (DEAD_BIT, DocFilter, pack_attrs,
                                          pack_pred, words_i32)
from infomesh_amd.ops import kernels as K
from infomesh_amd.ops import reference as R


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.manual_seed(0)


# ------------------------------------------------------- filter_bitmask

LANGS = ["en", "de", "fr"]
DOMAINS = ["a.org", "b.org", "c.org", "d.org", "e.org"]
T0 = 1_700_000_000

PREDS = [DocFilter(language="de", site="c.org", after=T0 + 10,
                   before=T0 + 3000),
         None,
         DocFilter(after=T0 + 64, before=T0 + 64)]


def _random_attrs(n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    rows = [pack_attrs([None, *LANGS][int(rng.integers(0, 4))],
                       DOMAINS[int(rng.integers(0, 5))], T0 + i)
            for i in range(n)]
    a = words_i32(rows)
    a[:, 1] |= np.where(rng.integers(0, 6, size=n) == 0, DEAD_BIT,
                        0).astype(np.int32)
    return a


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000, 4099])
def test_filter_bitmask_bit_exact(N, P):
    attrs = torch.from_numpy(_random_attrs(N, seed=N))
    preds = torch.from_numpy(words_i32([pack_pred(f) for f in PREDS[:P]]))
    # poison the allocator's next block: words past N must be WRITTEN 0
    W = (N + 63) // 64 * 2
    junk = torch.full((P, W), -1, device="cuda", dtype=torch.int32)
    del junk
    got = K.filter_bitmask(attrs.cuda(), preds.cuda())
    want = R.filter_bitmask(attrs, preds)
    assert got.shape == (P, W) and got.dtype == torch.int32
    assert torch.equal(got.cpu(), want)


# ---------------------------------------------------------- masked top-k

def _pack_bits(ok: np.ndarray) -> torch.Tensor:
    """bool [P, N] -> [P, W] i32, W = ceil(N/64)*2, zero past N."""
    P, N = ok.shape
    W = (N + 63) // 64 * 2
    full = np.zeros((P, W * 32), dtype=bool)
    full[:, :N] = ok
    words = np.packbits(full, axis=1, bitorder="little").view(np.uint32)
    return torch.from_numpy(words.view(np.int32).reshape(P, W).copy())


def _mask_config(kind: str, B: int, N: int, k: int, rng):
    """-> (ok bool [P, N], row_pred [B])."""
    def frac(p):
        return rng.random(N) < p
    if kind == "mixed":      # P = 3: ~50 %, ~1 %, 0 % pass, rows mix them
        ok = np.stack([frac(0.5), frac(0.01), np.zeros(N, dtype=bool)])
        return ok, np.arange(B) % 3
    if kind == "short":      # fewer than k documents pass
        ok = np.zeros((1, N), dtype=bool)
        ok[0, rng.choice(N, size=max(k // 2, 1), replace=False)] = True
        return ok, np.zeros(B, dtype=np.int64)
    p = {"p50": 0.5, "p01": 0.01, "p00": 0.0}[kind]
    return frac(p)[None, :], np.zeros(B, dtype=np.int64)


def _check_masked(scores, k, ok, rows):
    bits = _pack_bits(ok)
    row_pred = torch.from_numpy(rows.astype(np.int32))
    vals, idx = K.TopK("cuda")(scores, k, mask=bits.cuda(),
                               row_pred=row_pred.cuda())
    torch.cuda.synchronize()
    vals, idx = vals.cpu(), idx.cpu().long()
    want_v, want_i = R.masked_topk(scores.cpu(), k, bits, row_pred)
    assert torch.equal(vals, want_v), "values must match exactly"
    pad = want_i < 0
    assert torch.equal(idx < 0, pad) and (idx[pad] == -1).all()
    sc = scores.cpu()
    for b in range(scores.shape[0]):
        got = idx[b][~pad[b]]
        assert ok[rows[b]][got.numpy()].all(), "a failing document returned"
        assert got.unique().numel() == got.numel(), "duplicate index"
        assert torch.equal(sc[b, got], vals[b][~pad[b]])
    return vals, idx


SHAPES = [(3, 1000, 10), (2, 4099, 100), (4, 70000, 1024)]


@pytest.mark.parametrize("kind", ["mixed", "p50", "p01", "p00", "short"])
@pytest.mark.parametrize("B,N,k", SHAPES)
def test_masked_topk_matches_oracle(B, N, k, kind):
    rng = np.random.default_rng(N + len(kind))
    scores = torch.randn(B, N, device="cuda")
    ok, rows = _mask_config(kind, B, N, k, rng)
    vals, idx = _check_masked(scores, k, ok, rows)
    if kind in ("p00", "short"):
        n_pass = int(ok[0].sum())
        assert n_pass < k
        assert (idx[:, n_pass:] == -1).all() and (idx[:, :n_pass] >= 0).all()
        assert (vals[:, n_pass:] == -float("inf")).all()


@pytest.mark.parametrize("B,N,k", SHAPES)
def test_all_pass_mask_equals_unmasked(B, N, k):
    scores = torch.randn(B, N, device="cuda")
    bits = _pack_bits(np.ones((1, N), dtype=bool)).cuda()
    row_pred = torch.zeros(B, device="cuda", dtype=torch.int32)
    sel = K.TopK("cuda")
    v0, i0 = sel(scores, k)
    v1, i1 = sel(scores, k, mask=bits, row_pred=row_pred)
    assert torch.equal(v0, v1) and torch.equal(i0, i1)


def test_ext_hist1_with_mask_is_an_error():
    scores = torch.randn(1, 256, device="cuda")
    bits = _pack_bits(np.ones((1, 256), dtype=bool)).cuda()
    hist = torch.zeros(256, device="cuda", dtype=torch.int32)
    with pytest.raises(AssertionError):
        K.TopK("cuda")(scores, 4, ext_hist1=hist, mask=bits,
                       row_pred=torch.zeros(1, device="cuda",
                                            dtype=torch.int32))


def test_masked_topk_bm25_like_row():
    """Mostly-zero row: passing positives first, then passing zeros,
    never a failing document (the massive-tie path of compact)."""
    B, N, k = 2, 20000, 100
    rng = np.random.default_rng(4)
    scores = torch.zeros(B, N)
    pos = [rng.choice(N, size=50, replace=False) for _ in range(B)]
    for b in range(B):
        scores[b, pos[b]] = torch.from_numpy(
            rng.random(50).astype(np.float32) + 0.5)
    ok = (rng.random(N) < 0.3)[None, :]
    vals, idx = _check_masked(scores.cuda(), k, ok, np.zeros(B, dtype=np.int64))
    for b in range(B):
        passing_pos = [p for p in pos[b] if ok[0, p]]
        n = len(passing_pos)
        assert 0 < n < 50
        assert set(idx[b, :n].tolist()) == set(passing_pos)
        assert (vals[b, :n] > 0).all() and (vals[b, n:] == 0).all()
        assert (idx[b, n:] >= 0).all()


# -------------------------------------------------- GpuShard vs CpuShard

N_DOCS, SEG0, DIM = 3000, 1800, 64


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


def _build(cls, toks, meta, emb, with_attrs=True, **kw):
    shard = cls(**kw)
    for lo, hi in ((0, SEG0), (SEG0, N_DOCS)):
        for i in range(lo, hi):
            shard.add_document(
                5000 + i, toks[i], emb[i],
                attrs=pack_attrs(*meta[i]) if with_attrs else None)
        shard.build()
    assert len(shard.segments) == 2
    return shard


@pytest.fixture(scope="module")
def shards():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infomesh_amd.index.gpu_index import CpuShard, GpuShard
    toks, meta, emb = _corpus()
    return {"gpu": _build(GpuShard, toks, meta, emb, device="cuda"),
            "bare": _build(GpuShard, toks, meta, emb, with_attrs=False,
                           device="cuda"),
            "cpu": _build(CpuShard, toks, meta, emb),
            "meta": meta, "toks": toks, "emb": emb}


def _queries():
    rng = np.random.default_rng(17)
    terms = [rng.integers(0, 2000, size=3).astype(np.int64) for _ in range(4)]
    # bf16-representable queries: both planes then multiply the same
    # numbers and differ only in fp32 summation order
    q = torch.nn.functional.normalize(
        torch.randn(4, DIM, generator=torch.Generator().manual_seed(17)),
        dim=-1).bfloat16().float()
    return terms, q


def test_unfiltered_shard_ignores_attributes(shards):
    """No filter, no tombstone: the mask is inactive and the results are
    those of a shard that never had attributes."""
    terms, q = _queries()
    a = shards["gpu"].search(terms, q.cuda(), k=50)
    b = shards["bare"].search(terms, q.cuda(), k=50)
    for x, y in ((a.bm25_scores, b.bm25_scores), (a.bm25_ids, b.bm25_ids),
                 (a.dense_scores, b.dense_scores), (a.dense_ids, b.dense_ids)):
        assert torch.equal(x, y)


def test_gpu_shard_filters_and_deletes_match_cpu_shard(shards):
    """Runs last on the shared shards: it tombstones 100 documents."""
    gpu, cpu, meta = shards["gpu"], shards["cpu"], shards["meta"]
    terms, q = _queries()
    k = 50
    dead = list(range(5000, 5000 + N_DOCS, 30))
    assert len(dead) == 100
    assert gpu.delete(dead) == 100 and cpu.delete(dead) == 100
    assert gpu.delete(dead) == 0 and gpu.n_dead == 100
    filters = [DocFilter(language="fr"), DocFilter(site="d.org"),
               DocFilter(after=T0 + 500.5, before=T0 + 2200), None]
    got = gpu.search(terms, q.cuda(), k=k, filters=filters)
    torch.cuda.synchronize()
    want = cpu.search(terms, q, k=k + 1, filters=filters)

    def passes(gid, f):
        l, d, c = meta[gid - 5000]
        return (gid not in dead_set
                and (f is None or (
                    (not f.language or f.language == l)
                    and (not f.site or f.site == d)
                    and (f.after is None or c >= np.ceil(f.after))
                    and (f.before is None or c <= np.floor(f.before)))))
    dead_set = set(dead)
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
    # order moves a score by ~64 * 2^-24 — far inside the 1e-4 the
    # segment tests allow
    assert torch.allclose(got.dense_scores.cpu(), want.dense_scores[:, :k],
                          atol=1e-4)


def test_gpu_purge_equals_fresh_build(shards):
    """After the deletes above: purge() leaves what a bulk build from
    the survivors gives."""
    from infomesh_amd.index.gpu_index import GpuShard
    gpu, toks, meta, emb = (shards["gpu"], shards["toks"], shards["meta"],
                            shards["emb"])
    if gpu.n_dead == 0:
        gpu.delete(range(5000, 5000 + N_DOCS, 30))
    dead = set(range(5000, 5000 + N_DOCS, 30))
    assert gpu.purge() == 100 and gpu.n_dead == 0
    live = [i for i in range(N_DOCS) if 5000 + i not in dead]
    fresh = GpuShard("cuda")
    fresh.build_from_arrays(
        np.concatenate([toks[i] for i in live]),
        np.repeat(np.arange(len(live)), [len(toks[i]) for i in live]),
        np.array([len(toks[i]) for i in live]),
        np.array([5000 + i for i in live]), emb[live],
        attrs=[pack_attrs(*meta[i]) for i in live])
    assert gpu.n_docs == fresh.n_docs and gpu.avgdl == fresh.avgdl
    assert np.array_equal(gpu.df, fresh.df)
    assert torch.equal(gpu.attrs, fresh.attrs)
    assert torch.equal(gpu.global_ids, fresh.global_ids)
    s0, s1 = gpu.segments[0], fresh.segments[0]
    assert torch.equal(s0.offsets, s1.offsets)
    assert torch.equal(s0.doc_ids, s1.doc_ids)
    assert torch.equal(s0.tfdl, s1.tfdl)
    terms, q = _queries()
    a = gpu.search(terms, q.cuda(), k=50)
    b = fresh.search(terms, q.cuda(), k=50)
    assert torch.equal(a.bm25_scores, b.bm25_scores)
    assert torch.equal(a.bm25_ids, b.bm25_ids)
    assert torch.equal(a.dense_scores, b.dense_scores)


def test_live_only_mask_is_cached_until_the_next_delete(shards):
    """Tombstones and no filter: the live-only mask is built once and
    reused, and a further delete rebuilds it."""
    bare = shards["bare"]            # attribute records all zero
    terms, q = _queries()
    first = bare.search(terms, q.cuda(), k=50)
    gone = first.dense_ids[:, 0].tolist() + first.bm25_ids[:, 0].tolist()
    assert bare.delete(gone) == len(set(gone))
    a = bare.search(terms, q.cuda(), k=50)
    assert bare._live_bits is not None
    cached = bare._live_bits[0]
    b = bare.search(terms, q.cuda(), k=50)
    assert bare._live_bits[0] is cached
    for x, y in ((a.bm25_ids, b.bm25_ids), (a.dense_ids, b.dense_ids),
                 (a.dense_scores, b.dense_scores)):
        assert torch.equal(x, y)
    for ids in (a.bm25_ids, a.dense_ids):
        assert not (set(ids.flatten().tolist()) & set(gone))
        assert (ids >= 0).all()
    # the survivors move up: the best surviving score now leads
    for r in range(4):
        best = [sc for sc, i in zip(first.dense_scores[r].tolist(),
                                    first.dense_ids[r].tolist())
                if i not in gone][0]
        assert float(a.dense_scores[r, 0]) == best
    nxt = int(a.dense_ids[0, 0])
    assert bare.delete([nxt]) == 1 and bare._live_bits is None
    c = bare.search(terms, q.cuda(), k=50)
    assert nxt not in c.dense_ids[0].tolist()
