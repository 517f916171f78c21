"""GPU tests for the per-domain cap: collapse.hip's domain_best and
collapse_select against the sort-and-count oracle, bit for bit on both
outputs; GpuShard against CpuShard; HybridEngine.search_many with
per_domain (MI355X only)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from infomesh_amd.ops import _build
    _build.build()
import term_ops_corpus as C
from infomesh_amd.ops import kernels as K
from infomesh_amd.ops import reference as R
from match_set_cases import B, GARBAGE, SCORES, _mask, _size


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.manual_seed(0)


EDGES = np.asarray([0.0, -0.0, np.inf, -np.inf, -1.0, 1.0, -3.0e38],
                   dtype=np.float32)
SIZES = ["1", "63", "64", "65", "257", "C-1", "C", "C+1", "2C+37"]


def _scores(form: str, N: int, rng) -> np.ndarray:
    if form == "bm25":
        # a handful of values: ties abound, the column decides
        return rng.choice(SCORES, size=(B, N))
    s = rng.standard_normal((B, N)).astype(np.float32)
    edge = rng.random((B, N)) < 0.3
    s[edge] = rng.choice(EDGES, size=int(edge.sum()))
    return s


def _collapse(scores, rows, dom_id, D, m, ks, positive, mask=None,
              row_pred=None, out=None):
    """Kernel and oracle on the same arguments, for every k of ks over
    one domain_best -> the oracle's (vals, idx) of the last k."""
    s = torch.from_numpy(scores)
    rows_t = torch.tensor(rows, dtype=torch.int32)
    ids = torch.from_numpy(np.asarray(dom_id, dtype=np.int32))
    best = K.domain_best(
        s.cuda(), rows_t, ids.cuda(), D, m, positive,
        mask=None if mask is None else mask.cuda(),
        row_pred=None if row_pred is None else row_pred.cuda(), out=out)
    assert best.dtype == torch.int64 and best.shape == (m, len(rows), D)
    want = None
    for k in ks:
        want = R.collapse_topk(s, rows_t, ids, m, k, positive, mask=mask,
                               row_pred=row_pred)
        vals, idx = K.collapse_select(best, k)
        torch.cuda.synchronize()
        assert vals.dtype == torch.float32 and idx.dtype == torch.int32
        assert vals.shape == idx.shape == (len(rows), k)
        assert torch.equal(idx.cpu(), want[1]), (m, k)
        # bit for bit: -0.0 is not +0.0 here
        assert torch.equal(vals.cpu().view(torch.int32),
                           want[0].view(torch.int32)), (m, k)
    return want[0].numpy(), want[1].numpy()


def test_exported_sizes():
    CH, S = K.collapse_chunk_docs(), K.collapse_lds_slots()
    assert CH == K.domtop_chunk_docs() == K.facet_chunk_docs()
    assert S >= 64 and S & (S - 1) == 0 and S < CH
    assert K.collapse_m_max() == 4 and K.collapse_k_max() == 1024


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("form", ["bm25", "dense"])
@pytest.mark.parametrize("size", SIZES)
def test_collapse_exact(size, form, masked):
    CH = K.collapse_chunk_docs()
    N = _size(size, CH)
    rng = np.random.default_rng(N * 11 + masked + 2 * (form == "dense"))
    rows = [2, 0, 3]
    scores = _scores(form, N, rng)
    scores[1] = GARBAGE
    # a few heavy domains and a long tail, as a Zipf draw gives them;
    # the tail's domains hold fewer than m eligible documents
    D = 300
    dom_id = np.minimum(rng.zipf(1.3, size=N) - 1, D - 1)
    mask = row_pred = None
    if masked:
        mask = _mask(N, CH, rng)
        row_pred = torch.tensor([0, 2, 0, 1], dtype=torch.int32)
    ks = [1, 10, min(N + 3, K.collapse_k_max())]
    if size == "2C+37":
        ks.append(K.collapse_k_max())
    for m in (1, 2, 4):
        vals, idx = _collapse(scores, rows, dom_id, D, m, ks,
                              form == "bm25", mask, row_pred)
        real = idx >= 0
        assert (real[:, :-1] >= real[:, 1:]).all(), "padding comes last"
        assert (vals[~real] == -np.inf).all()
        if masked:
            assert not real[2].any(), "the all-zero mask row returned hits"
        for r in range(len(rows)):
            got = dom_id[idx[r][real[r]]]
            assert np.bincount(got, minlength=D).max(initial=0) <= m
        if not masked and form == "dense":
            # every document is eligible: each domain present fills up
            present = np.minimum(np.bincount(dom_id, minlength=D), m).sum()
            assert real.sum(1).tolist() == [min(present, ks[-1])] * 3
        assert (vals != np.float32(GARBAGE)).all(), "the garbage row leaked"


@pytest.mark.parametrize("form", ["bm25", "dense"])
def test_every_document_its_own_domain_overflows_the_lds_table(form):
    CH = K.collapse_chunk_docs()
    N = CH + 1
    assert CH > K.collapse_lds_slots()
    rng = np.random.default_rng(5)
    scores = _scores(form, N, rng)
    perm = rng.permutation(N)
    for m in (1, 2):
        # the cap never bites: the plain order of the eligible documents
        vals, idx = _collapse(scores, [1, 3], perm, N, m,
                              [10, K.collapse_k_max()], form == "bm25")
        assert (idx >= 0).all()


@pytest.mark.parametrize("form", ["bm25", "dense"])
def test_one_domain_for_every_document(form):
    CH = K.collapse_chunk_docs()
    N = 2 * CH + 37
    rng = np.random.default_rng(6)
    scores = _scores(form, N, rng)
    # among several ids, and with the workspace form of `out`
    ws = torch.full((4 * 3 * 7 + 5,), 77, dtype=torch.int64, device="cuda")
    vals, idx = _collapse(scores, [1, 3, 0], np.full(N, 4), 7, 4, [1, 10],
                          form == "bm25", out=ws[:84].view(4, 3, 7))
    assert ((idx >= 0).sum(1) == 4).all()
    assert (ws[84:] == 77).all()
    # D = 1, m = 1: the row's best document and nothing else
    vals, idx = _collapse(scores, [2], np.zeros(N), 1, 1, [3],
                          form == "bm25")
    assert (idx[0, 1:] == -1).all() and idx[0, 0] >= 0


def test_a_domain_with_fewer_than_m_eligible_documents():
    N = 65
    scores = np.zeros((B, N), dtype=np.float32)
    scores[0, [3, 9, 20, 21, 64]] = [2.0, 1.0, 2.0, 3.0, 1.0]
    dom = np.zeros(N, dtype=np.int32)
    dom[[9, 64]] = 1                      # two eligible documents
    dom[20] = 2                           # one
    vals, idx = _collapse(scores, [0], dom, 3, 4, [8], True)
    assert idx[0].tolist() == [21, 3, 20, 9, 64, -1, -1, -1]
    vals, idx = _collapse(scores, [0], dom, 3, 1, [8], True)
    assert idx[0].tolist() == [21, 20, 9, -1, -1, -1, -1, -1]
    assert vals[0, :3].tolist() == [3.0, 2.0, 1.0]


# ------------------------------------- collapse_select on hand-built keys

SELECT_KS = (1, 1024)


def _hand_keys(scores: np.ndarray, cols: np.ndarray) -> np.ndarray:
    """collapse.hip's key, float_to_ordered(score) << 32 |
    (0xFFFFFFFF - col), in numpy."""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    okey = np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000))
    return (okey.astype(np.uint64) << np.uint64(32)) \
        | (0xFFFFFFFF - cols).astype(np.uint64)


def _decode_keys(keys: np.ndarray, k: int):
    """The first k of `keys` (sorted) as (vals, idx), -inf / -1 behind."""
    hi = (keys[:k] >> np.uint64(32)).astype(np.uint32)
    bits = np.where(hi >> 31 != 0, hi & np.uint32(0x7FFFFFFF), ~hi)
    vals = np.full(k, -np.inf, dtype=np.float32)
    idx = np.full(k, -1, dtype=np.int32)
    vals[:len(hi)] = bits.astype(np.uint32).view(np.float32)
    idx[:len(hi)] = (0xFFFFFFFF - (keys[:k] & np.uint64(0xFFFFFFFF))) \
        .astype(np.int64)
    return vals, idx


def _select_case(nnz: int, m: int):
    """best [m, 2, D] u64 holding nnz keys per row among zeros, and per k
    of SELECT_KS the oracle (vals [2, k], idx [2, k]): np.sort of the
    row's non-zero keys, descending, decoded. Row 0: scores from EDGES
    and normals, columns below 2^31. Row 1: one score and columns below
    2^24, so all keys share their top 40 bits."""
    rng = np.random.default_rng(nnz * 5 + m)
    D = (nnz + m - 1) // m + 37
    s0 = rng.standard_normal(nnz).astype(np.float32)
    edge = rng.random(nnz) < 0.5
    s0[edge] = rng.choice(EDGES, size=int(edge.sum()))
    c0 = rng.choice(1 << 20, size=nnz, replace=False).astype(np.int64) \
        * 2047 + rng.integers(0, 2047, size=nnz)
    c1 = rng.choice(1 << 24, size=nnz, replace=False).astype(np.int64)
    rows = [_hand_keys(s0, c0),
            _hand_keys(np.full(nnz, 0.75, dtype=np.float32), c1)]
    assert ((rows[1] >> np.uint64(24)) == (rows[1][:1] >> np.uint64(24))).all()
    best = np.zeros((m, 2, D), dtype=np.uint64)
    want = {k: ([], []) for k in SELECT_KS}
    for r, keys in enumerate(rows):
        assert len(np.unique(keys)) == nnz and (keys != 0).all()
        at = rng.choice(m * D, size=nnz, replace=False)
        best[at // D, r, at % D] = keys
        tab = best[:, r, :].reshape(-1)
        ordered = np.sort(tab[tab != 0])[::-1]
        assert len(ordered) == nnz
        for k in SELECT_KS:
            vals, idx = _decode_keys(ordered, k)
            # the oracle's own invariants: real entries first, in key
            # order, every one a pair that went in
            n = min(nnz, k)
            assert (idx[:n] >= 0).all() and (idx[n:] == -1).all()
            assert (vals[n:] == -np.inf).all()
            assert (_hand_keys(vals[:n], idx[:n].astype(np.int64))
                    == ordered[:n]).all()
            assert (ordered[:-1] > ordered[1:]).all()
            want[k][0].append(vals)
            want[k][1].append(idx)
    return best, {k: (np.stack(v), np.stack(i)) for k, (v, i) in want.items()}


@pytest.mark.parametrize("m", [1, 4])
@pytest.mark.parametrize("nnz", [0, 1, 1023, 1024, 1025, 2049, 4096, 4097,
                                 20000])
def test_collapse_select_on_hand_built_keys(nnz, m):
    """collapse_select alone, on keys built here: the non-zero counts
    around k = 1024, around the 4096 candidate keys it sorts in LDS
    (2049 pads to 4096; 4096 fills it with no radix pass; 4097 forces
    one) and far above; row 1 takes several passes to tell its keys
    apart."""
    best, want = _select_case(nnz, m)
    best_t = torch.from_numpy(best.view(np.int64)).cuda()
    for k in SELECT_KS:
        vals, idx = K.collapse_select(best_t, k)
        torch.cuda.synchronize()
        assert vals.shape == idx.shape == (2, k)
        assert np.array_equal(idx.cpu().numpy(), want[k][1]), (nnz, m, k)
        # bit for bit: -0.0 is not +0.0 here
        assert np.array_equal(vals.cpu().numpy().view(np.int32),
                              want[k][0].view(np.int32)), (nnz, m, k)


def test_over_a_cap_is_a_value_error_before_the_launch():
    N = 64
    scores = torch.ones((B, N), device="cuda")
    ids = torch.zeros(N, dtype=torch.int32, device="cuda")
    rows = torch.tensor([0], dtype=torch.int32)
    best = K.domain_best(scores, rows, ids, 3, 2, True)    # the good ones
    K.collapse_select(best, 1024)
    for bad in (0, 5, -1):
        with pytest.raises(ValueError, match="m ="):
            K.domain_best(scores, rows, ids, 3, bad, True)
    for bad in (0, 1025, -1):
        with pytest.raises(ValueError, match="k ="):
            K.collapse_select(best, bad)
    with pytest.raises(ValueError, match="D ="):
        K.domain_best(scores, rows, ids, 0, 1, False)
    # what would index outside an array is refused too
    for bad_rows in ([4], [-1]):
        with pytest.raises(AssertionError):
            K.domain_best(scores, torch.tensor(bad_rows, dtype=torch.int32),
                          ids, 3, 1, True)
    with pytest.raises(AssertionError):
        K.domain_best(scores, rows, ids[:-1], 3, 1, True)
    torch.cuda.synchronize()


# -------------------------------------------------- GpuShard vs CpuShard

@pytest.fixture(scope="module")
def shards():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infomesh_amd.index.gpu_index import CpuShard, GpuShard
    toks, meta, emb = C.corpus()
    return {"gpu": C.build_shard(GpuShard, toks, meta, emb, device="cuda"),
            "cpu": C.build_shard(CpuShard, toks, meta, emb)}


def _bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.dtype == b.dtype and torch.equal(a, b)


def test_gpu_shard_per_domain_matches_cpu_shard(shards):
    """Capped and uncapped rows in one batch, with filters and term
    operands. The two shards' scores agree to C.SCORE_ATOL, so the hits
    are compared as test_term_ops_gpu.py compares them: scores within
    the tolerance, ids equal wherever the oracle's neighbours are not
    tied. The uncapped rows equal the same batch without caps, bit for
    bit."""
    gpu, cpu = shards["gpu"], shards["cpu"]
    terms, q, filters, ops = C.queries()
    caps = [2, 0, 1, 4, 1, None]
    k = C.K_CMP
    kw = dict(filters=filters, term_ops=ops)
    plain = gpu.search(terms, q.cuda(), k=k, **kw)
    got = gpu.search(terms, q.cuda(), k=k, per_domain=caps, **kw)
    torch.cuda.synchronize()
    assert plain.bm25_dom is None and plain.dense_dom is None
    want = cpu.search(terms, q, k=k + 1, per_domain=caps, **kw)
    names = ("bm25_scores", "bm25_ids", "dense_scores", "dense_ids")
    for b, m in enumerate(caps):
        if not m:
            for name in names:
                assert _bits_equal(getattr(got, name)[b],
                                   getattr(plain, name)[b]), (name, b)
    capped = [b for b, m in enumerate(caps) if m]
    tied_share = []
    for plane in ("bm25", "dense"):
        g_s = getattr(got, plane + "_scores").cpu()[capped]
        g_i = getattr(got, plane + "_ids").cpu()[capped]
        g_d = getattr(got, plane + "_dom").cpu()[capped]
        w_s = getattr(want, plane + "_scores")[capped]
        w_i = getattr(want, plane + "_ids")[capped]
        w_d = getattr(want, plane + "_dom")[capped]
        assert g_d.dtype == torch.int32 and g_d.shape == (len(capped), k)
        real = torch.isfinite(w_s[:, :k])
        assert torch.equal(torch.isfinite(g_s), real), plane
        assert torch.allclose(g_s[real], w_s[:, :k][real], rtol=0,
                              atol=C.SCORE_ATOL), plane
        must, tied = C.untied(w_s, k)
        tied_share.append(tied)
        assert torch.equal(g_i[must], w_i[:, :k][must]), plane
        assert torch.equal(g_d[must], w_d[:, :k][must]), plane
        # the cap itself holds exactly, ties or not
        for r, b in enumerate(capped):
            hit = g_i[r] >= 0
            assert int(hit.sum()) > 0 and not g_d[r][~hit].any()
            assert np.unique(g_d[r][hit].numpy(),
                             return_counts=True)[1].max() <= caps[b]
    assert max(tied_share) <= C.MAX_TIED
    # four domains, cap 4, k = 20: the cap bites
    assert int((got.dense_ids[3] >= 0).sum()) <= 16
    assert int((plain.dense_ids[3] >= 0).sum()) == k


def test_capped_rows_take_slices_when_the_workspace_is_small(shards,
                                                             monkeypatch):
    """With a workspace cap that holds one row, the capped rows go
    through domain_best one at a time and the result is the same."""
    from infomesh_amd.index import gpu_index
    gpu = shards["gpu"]
    terms, q, _, _ = C.queries()
    caps = [2, 2, 0, 2, 1, 2]
    whole = gpu.search(terms, q.cuda(), k=10, per_domain=caps)
    monkeypatch.setattr(gpu_index, "COLLAPSE_WS_BYTES", 1)
    sliced = gpu.search(terms, q.cuda(), k=10, per_domain=caps)
    torch.cuda.synchronize()
    for name in ("bm25_scores", "bm25_ids", "dense_scores", "dense_ids",
                 "bm25_dom", "dense_dom"):
        assert _bits_equal(getattr(whole, name), getattr(sliced, name)), name


# ---------------------------------------------------------------- engine

def _site_engine(device: str, use_encoder: bool):
    from infomesh_amd.engine import HybridEngine
    from infomesh_amd.index.local_store import Document
    eng = HybridEngine(device=device, use_encoder=use_encoder)
    site = {}
    for i in range(60):
        # one site holds 40 short documents full of the query word; ten
        # small sites hold two longer ones each
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
    return eng, site


def test_engine_per_domain_on_the_device():
    eng, site = _site_engine("cuda", True)
    limit = 10
    plain = eng.search_many(["rust"] * 3, limit=limit)
    rows = eng.search_many(["rust", "rust", "rust"], limit=limit,
                           per_domain=[2, None, 1])
    capped, same, one = rows
    assert [h.doc_id for h in same] == [h.doc_id for h in plain[1]]
    big = sum(site[h.doc_id] == "big.org" for h in plain[0])
    assert len(plain[0]) == limit and big > 2, "one site dominates"
    assert len(capped) == limit
    tally = {}
    for h in capped:
        tally[site[h.doc_id]] = tally.get(site[h.doc_id], 0) + 1
    assert max(tally.values()) <= 2 and len(tally) >= limit // 2
    assert len(one) == limit
    assert len({site[h.doc_id] for h in one}) == limit
    with pytest.raises(ValueError, match="per_domain"):
        eng.search_many(["rust"], limit=limit, per_domain=[5])
