"""GPU tests for required / excluded query terms: termmask.hip against
its numpy oracle, bit for bit; GpuShard against CpuShard with operators,
filters and tombstones in one batch; HybridEngine require / exclude
(MI355X only)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from infomesh_amd.ops import _build
    _build.build()
import term_ops_corpus as C
from infomesh_amd.index.doc_attrs import (DEAD_BIT, DocFilter, TermOps,
                                          domain_hash, pack_pred,
                                          pack_pred_sets, words_i32)
from infomesh_amd.ops import kernels as K
from infomesh_amd.ops import reference as R


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.manual_seed(0)


# ------------------------------------------------- kernel vs the oracle

T0 = 1_700_000_000
DOMS = [domain_hash(d) for d in ("a.org", "b.org", "c.org")]
NONE, ALL, EDGES = 0, 1, 2          # term ids of the hand-built index
DENSE0, SPARSE0, V = 3, 11, 19      # 8 dense and 8 sparse terms follow


def _sizes(name: str, TB: int) -> int:
    return {"1": 1, "63": 63, "64": 64, "65": 65, "TB-1": TB - 1, "TB": TB,
            "TB+1": TB + 1, "2TB+37": 2 * TB + 37}[name]


def _seg_ranges(layout: str, N: int, TB: int) -> list[tuple[int, int]]:
    """One segment, or segments at doc_base 0, 45, 45 + TB + 3 (those
    that start inside [0, N)): no base but 0 a multiple of 32."""
    bases = [0] if layout == "one" else [b for b in (0, 45, 45 + TB + 3)
                                         if b < N]
    return list(zip(bases, bases[1:] + [N]))


def _members(N: int, TB: int, ranges) -> np.ndarray:
    """bool [V, N]: which documents hold which term."""
    d = np.arange(N)
    m = np.zeros((V, N), dtype=bool)
    m[ALL] = True
    edges = {0, N - 1}
    for lo, hi in ranges:                   # first / last of a segment
        edges |= {lo, hi - 1}
    for b in range(0, N, TB):               # first / last of a block
        edges |= {b, min(b + TB, N) - 1}
    m[EDGES, sorted(edges)] = True
    for j in range(8):
        m[DENSE0 + j] = d % (j + 2) != 1
        m[SPARSE0 + j] = d % (11 + j) == 3
    return m


def _segments(m: np.ndarray, ranges, ids: np.ndarray, device):
    segs = []
    for lo, hi in ranges:
        term, doc = np.nonzero(m[:, lo:hi])   # term-major, docs ascending
        offs = np.zeros(V + 1, dtype=np.int64)
        np.cumsum(np.bincount(term, minlength=V), out=offs[1:])
        segs.append((torch.from_numpy(doc.astype(np.int32)).to(device), lo,
                     hi - lo, torch.from_numpy(offs[ids]),
                     torch.from_numpy(offs[ids + 1])))
    return segs


def _base_bits(N: int) -> torch.Tensor:
    """Three rows to start from: live-only over a shard with dead
    documents, a dated predicate, a predicate with a domain list."""
    d = np.arange(N)
    a = np.zeros((N, 4), dtype=np.uint32)
    a[:, 0] = T0 + d
    a[:, 1] = np.where(d % 7 == 3, DEAD_BIT, 0)
    a[:, 2] = np.asarray(DOMS, dtype=np.uint32)[d % 3]
    packed = [pack_pred_sets(None),
              pack_pred_sets(DocFilter(after=T0 + N // 3)),
              pack_pred_sets((pack_pred(None), (), (DOMS[1],)))]
    desc = torch.tensor([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]],
                        dtype=torch.int32)
    doms = torch.from_numpy(np.asarray([DOMS[1]], dtype=np.uint32)
                            .view(np.int32))
    return R.filter_bitmask_sets(
        torch.from_numpy(a.view(np.int32)),
        torch.from_numpy(words_i32([w for w, _, _ in packed])), desc, doms)


DENSE = list(range(DENSE0, DENSE0 + 8))
SPARSE = list(range(SPARSE0, SPARSE0 + 8))
# (base row, require, exclude) per term row
CASES = {
    # no postings at all, as require and as exclude; a term in every
    # document, as exclude
    "none-all": [(0, [NONE], []), (1, [ALL], [NONE]), (2, [], [ALL])],
    # first / last document of every block and segment; the same id in
    # both lists
    "edges-both": [(0, [EDGES], []), (1, [], [EDGES]),
                   (2, [SPARSE0], [SPARSE0])],
    # the cap: 16 operands; require only; exclude only
    "cap-req-exc": [(0, DENSE, SPARSE), (1, DENSE[:2], []),
                    (2, [], SPARSE[:2])],
    "one-cap": [(2, DENSE[:3] + [ALL], SPARSE + [EDGES, NONE] + DENSE[4:6])],
    "one-edges": [(1, [EDGES, ALL], [NONE])],
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("layout", ["one", "three"])
@pytest.mark.parametrize("size", ["1", "63", "64", "65", "TB-1", "TB", "TB+1",
                                  "2TB+37"])
def test_term_bitmask_bit_exact(size, layout, case):
    TB = K.term_block_docs()
    assert TB % 64 == 0
    N = _sizes(size, TB)
    rows = CASES[case]
    ranges = _seg_ranges(layout, N, TB)
    if layout == "three" and size == "2TB+37":
        assert [lo for lo, _ in ranges] == [0, 45, 45 + TB + 3]
    m = _members(N, TB, ranges)
    ids = np.asarray([t for _, rq, ex in rows for t in rq + ex],
                     dtype=np.int64)
    op_off = np.zeros(len(rows) + 1, dtype=np.int32)
    np.cumsum([len(rq) + len(ex) for _, rq, ex in rows], out=op_off[1:])
    assert op_off.max() <= 16 * len(rows)
    kind = np.asarray([k for _, rq, ex in rows
                       for k in [0] * len(rq) + [1] * len(ex)], dtype=np.int32)
    src = torch.tensor([p for p, _, _ in rows], dtype=torch.int64)
    base = _base_bits(N)
    want = R.term_bitmask(base, src, _segments(m, ranges, ids, "cpu"),
                          torch.from_numpy(op_off), torch.from_numpy(kind), N)
    base_d = base.cuda()
    got = K.term_bitmask(base_d, src.cuda(),
                         _segments(m, ranges, ids, "cuda"),
                         torch.from_numpy(op_off), torch.from_numpy(kind), N)
    W = (N + 63) // 64 * 2
    assert got.shape == (len(rows), W) and got.dtype == torch.int32
    assert torch.equal(got.cpu(), want)                   # all R x W words
    assert torch.equal(base_d.cpu(), base), "the base rows were written"
    # the oracle itself, where the answer is known without it
    w = want.numpy().view(np.uint32)
    if case == "none-all":
        assert not w[0].any() and not w[2].any()
        assert np.array_equal(w[1], base.numpy().view(np.uint32)[1])
    if case == "edges-both":
        assert not w[2].any()
        kept = np.unpackbits(w[0].view(np.uint8), bitorder="little")[:N]
        assert kept.sum() <= m[EDGES].sum() and not kept[~m[EDGES]].any()
        # both ends are edges, and live unless d % 7 == 3
        assert kept[0] == 1 and bool(kept[N - 1]) == ((N - 1) % 7 != 3)


def test_table_is_checked_before_the_launch():
    N = 130
    ranges = [(0, 45), (45, N)]
    m = _members(N, 32768, ranges)
    ids = np.asarray([ALL, EDGES], dtype=np.int64)
    base = _base_bits(N).cuda()
    src = torch.tensor([0], dtype=torch.int64)
    off = torch.tensor([0, 2], dtype=torch.int32)
    kind = torch.tensor([0, 1], dtype=torch.int32)

    def segs():
        return [list(s) for s in _segments(m, ranges, ids, "cuda")]
    K.term_bitmask(base, src, segs(), off, kind, N)       # the good one
    npost = segs()[0][0].numel()
    for begin, end in (([0, -1], [1, 1]), ([2, 0], [1, 1]),
                       ([0, 0], [npost + 1, 1])):
        bad = segs()
        bad[0][3] = torch.tensor(begin, dtype=torch.int64)
        bad[0][4] = torch.tensor(end, dtype=torch.int64)
        with pytest.raises(AssertionError):
            K.term_bitmask(base, src, bad, off, kind, N)
    bad = segs()
    bad[1][1] = 40                                        # overlaps segment 0
    with pytest.raises(AssertionError):
        K.term_bitmask(base, src, bad, off, kind, N)
    bad = segs()
    bad[1][2] = N                                         # runs past N
    with pytest.raises(AssertionError):
        K.term_bitmask(base, src, bad, off, kind, N)
    for bad_off in ([0, 3], [1, 2], [0, 1]):
        with pytest.raises(AssertionError):
            K.term_bitmask(base, src, segs(),
                           torch.tensor(bad_off, dtype=torch.int32), kind, N)
    with pytest.raises(AssertionError):                   # 17 operands
        K.term_bitmask(base, src, _segments(m, ranges, np.full(17, ALL),
                                            "cuda"),
                       torch.tensor([0, 17], dtype=torch.int32),
                       torch.zeros(17, dtype=torch.int32), N)
    with pytest.raises(AssertionError):
        K.term_bitmask(base, torch.tensor([3]), segs(), off, kind, N)
    with pytest.raises(AssertionError):
        K.term_bitmask(base, src, segs(), off,
                       torch.tensor([0, 2], dtype=torch.int32), N)
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


def test_gpu_shard_operators_match_cpu_shard(shards):
    gpu, cpu = shards["gpu"], shards["cpu"]
    meta, sets = shards["meta"], shards["sets"]
    terms, q, filters, ops = C.queries()
    k = C.K_CMP
    gpu.search(terms, q.cuda(), k=k)                      # caches live bits
    live_before = gpu._live_bits[0].clone()
    got = gpu.search(terms, q.cuda(), k=k, filters=filters, term_ops=ops)
    torch.cuda.synchronize()
    want = cpu.search(terms, q, k=k + 1, filters=filters, term_ops=ops)
    for name in ("bm25", "dense"):
        gs = getattr(got, name + "_scores").cpu()
        gi = getattr(got, name + "_ids").cpu()
        ws = getattr(want, name + "_scores")
        wi = getattr(want, name + "_ids")
        for qi, (f, t) in enumerate(zip(filters, ops)):
            row = gi[qi][gi[qi] >= 0].tolist()
            assert all(C.passes(g, meta, f, t, sets) for g in row), (name, qi)
            assert len(row) == len(set(row)) == int((wi[qi, :k] >= 0).sum())
        assert torch.equal(torch.isinf(gs), torch.isinf(ws[:, :k]))
        fin = torch.isfinite(gs)
        assert torch.allclose(gs[fin], ws[:, :k][fin], atol=C.SCORE_ATOL)
        must, tied = C.untied(ws, k)
        print(f"{name}: tied share {tied:.3f}, compared {int(must.sum())}")
        assert tied <= C.MAX_TIED
        assert torch.equal(gi[must], wi[:, :k][must]), name
    # the row without operands and without a filter still drops the dead
    assert (got.bm25_ids[3] >= 0).all()
    # operands alone on a shard with tombstones start from the cached
    # live-only row, which they must not write
    assert live_before is not None
    got = gpu.search(terms, q.cuda(), k=k, term_ops=ops)
    want = cpu.search(terms, q, k=k, term_ops=ops)
    for a, b in ((got.bm25_ids, want.bm25_ids),
                 (got.dense_ids, want.dense_ids)):
        assert torch.equal(a.cpu() >= 0, b >= 0)
        for qi, t in enumerate(ops):
            assert all(C.passes(g, meta, None, t, sets)
                       for g in a[qi][a[qi] >= 0].tolist()), qi
    assert torch.equal(gpu._live_bits[0], live_before), \
        "the cached live-only bits were written"


def test_operators_alone_start_from_the_live_only_row():
    """No filter and no tombstone: the batch is masked all the same."""
    from infomesh_amd.index.gpu_index import CpuShard, GpuShard
    toks, meta, emb = C.corpus()
    pair = []
    for cls, kw in ((GpuShard, {"device": "cuda"}), (CpuShard, {})):
        s = cls(**kw)
        for lo, hi in ((0, 45), (45, 110)):
            for i in range(lo, hi):
                s.add_document(C.GID0 + i, toks[i], emb[i])
            s.build()
        pair.append(s)
    gpu, cpu = pair
    terms, q, _, _ = C.queries()
    ops = [TermOps.of(exclude=[C.EVERY3]), None,
           TermOps.of(require=[C.NOWHERE]),
           TermOps.of(require=[C.EVERY5], exclude=[C.EVERY5])]
    got = gpu.search(terms[:4], q[:4].cuda(), k=110, term_ops=ops)
    want = cpu.search(terms[:4], q[:4], k=110, term_ops=ops)
    for a, b in ((got.bm25_ids, want.bm25_ids),
                 (got.dense_ids, want.dense_ids)):
        a = a.cpu()
        for qi in range(4):
            assert sorted(a[qi].tolist()) == sorted(b[qi].tolist()), qi
        assert (a[2] == -1).all() and (a[3] == -1).all()
        assert (a[1] >= 0).all()
        assert sorted(a[0][a[0] >= 0].tolist()) == [
            C.GID0 + i for i in range(110) if i % 3]
    assert torch.isinf(got.bm25_scores[2]).all()


# ---------------------------------------------------------------- engine

def test_engine_require_and_exclude_on_both_planes():
    from infomesh_amd.engine import HybridEngine
    from infomesh_amd.index.local_store import Document
    eng = HybridEngine(device="cuda", use_encoder=True)
    texts = {}
    for i in range(40):
        words = ["rust"] + (["java"] if i % 2 == 0 else ["golang"]) \
            + (["async"] if i % 4 < 2 else ["threads"]) + [f"note{i}"] * i
        texts[i] = " ".join(words)
        eng.add_document(Document(url=f"https://x.org/{i}", title=f"t{i}",
                                  text=texts[i], doc_id=i))
    eng.flush()
    plain = eng.search("rust", limit=40)
    assert any("java" in texts[h.doc_id] for h in plain)   # today's result
    got = eng.search("rust", limit=40, exclude=("java",))
    assert len(got) == 20
    assert not any("java" in texts[h.doc_id] for h in got)
    got = eng.search("rust", limit=40, require=("async",))
    assert len(got) == 20
    assert all("async" in texts[h.doc_id] for h in got)
    got = eng.search("rust", limit=40, require=("async",),
                     exclude=("java",))
    assert sorted(h.doc_id for h in got) == [i for i in range(40)
                                             if i % 4 == 1]
    # in a batch, the row with neither equals today's result
    batch = eng.search_many(["rust", "rust"], limit=40,
                            exclude=[("java",), None])
    assert [h.doc_id for h in batch[1]] == [h.doc_id for h in plain]
    # rrf_fuse reads a fused score off a running fp32 sum over the row's
    # <= 80 contributions, which reaches ~1: its rounding, <= 80 * 2^-24
    # ~ 5e-6, depends on the batch shape. Neighbouring RRF scores differ
    # by 1/(60+r) - 1/(61+r) >= 1e-4.
    assert [h.score for h in batch[1]] == pytest.approx(
        [h.score for h in plain], abs=5e-6, rel=0)
    assert not any("java" in texts[h.doc_id] for h in batch[0])
