"""Distributed query plane: broadcast queries to every GPU shard, score
locally, all-gather fixed-size top-k, fuse on rank 0.

This is the MI355X-native replacement for the reference's
QueryRouter.route_query scatter-gather over libp2p
(infomesh/p2p/routing.py:133-267) and DHT-pointer aggregation
(infomesh/index/distributed.py:235-276): exhaustive fan-out to all
shards instead of probabilistic top-5 peers, all-gather of
k-per-shard candidate records over xGMI instead of msgpack streams.

The RRF fusion is fully vectorized (sort + segment-sum) so the host
merge never bottlenecks the GPU planes.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from ..index.doc_attrs import (HAS_ALLOW_BIT, HAS_BLOCK_BIT, TOP_FETCH,
                               U32_MAX, FacetSpec, PackedFacets, TermOps,
                               pack_facets, pack_pred_sets)
from ..index.gpu_index import GpuShard, ShardHits, per_domain_caps
from .fabric import Fabric

RRF_K = 60
MAX_QUERY_TERMS = 32
# Filter predicates ride in the terms broadcast as two extra int64
# columns per row: x | y<<32 and z | w<<32 of doc_attrs.pack_pred. Bit 17
# of z is unused by the predicate and marks "this row has a filter";
# an unfiltered row carries two zeros. Bits 18 / 19 of z (has_allow /
# has_block) announce domain lists; only a batch with such a row is
# followed by the two list broadcasts of _broadcast_lists.
_PRED_COLS = 2
_HAS_FILTER = 1 << 17
_HAS_LISTS = HAS_ALLOW_BIT | HAS_BLOCK_BIT
# Bit 20 of ROW 0's z marks a batch that carries a FacetSpec: the spec
# belongs to the batch, not to a row, and row 0 always exists. It is
# stripped before the predicates are unpacked, and only such a batch is
# followed by the two broadcasts of _broadcast_facets.
_HAS_FACETS = 1 << 20
# Bits 21..23 of a row's z hold its per-domain cap m (0 = none, at most
# COLLAPSE_M_MAX = 4). They are stripped before the predicates are
# unpacked; an uncapped batch's broadcast is what it always was.
_CAP_SHIFT = 21
_CAP_BITS = 7 << _CAP_SHIFT
# Bit 40 of the hash count in _broadcast_facets' header: the spec asks
# for top domains somewhere, and its body carries one T per counted row.
_HAS_TOP = 1 << 40
# Term operands (TermOps) ride in the same broadcast, as flag bits on the
# row's term entries; term ids are below 2^17, so bits 40.. are free. A
# require operand is its scoring term with bit 40 set, an exclude operand
# an extra entry with bit 41 set, which is no scoring term. A require id
# that is not among the row's scoring terms carries bit 42 as well and is
# not scored either. Operands come first in the row, so the cut at
# MAX_QUERY_TERMS entries drops scoring terms, never an operand.
_OP_REQUIRE = 1 << 40
_OP_EXCLUDE = 1 << 41
_OP_UNSCORED = 1 << 42
_OP_FLAGS = _OP_REQUIRE | _OP_EXCLUDE | _OP_UNSCORED


def pack_term_row(terms: np.ndarray, ops: TermOps | None,
                  T: int = MAX_QUERY_TERMS) -> np.ndarray:
    """One query's entries of the terms broadcast, at most T: the
    operands, flagged, then the remaining scoring terms. A required id
    stands for ONE of its occurrences among the scoring terms; repeats
    stay behind it, so the receivers see every term as often as rank 0
    does. The order differs from the caller's; the shards dedupe and
    sort a row's terms before scoring (GpuShard.dedupe_terms), so
    neither order nor repeats change a score."""
    terms = np.asarray(terms, dtype=np.int64)
    if not ops:
        return terms[:T]
    rest = terms.tolist()
    head = []
    for t in ops.require:
        if t in rest:
            rest.remove(t)              # the first occurrence only
            head.append(t | _OP_REQUIRE)
        else:
            head.append(t | _OP_REQUIRE | _OP_UNSCORED)
    head += [t | _OP_EXCLUDE for t in ops.exclude]
    return np.asarray(head + rest, dtype=np.int64)[:T]


def unpack_term_row(row: np.ndarray) -> tuple[np.ndarray, TermOps | None]:
    """(scoring terms, TermOps or None) of a row pack_term_row wrote
    (negative entries are padding)."""
    row = np.asarray(row, dtype=np.int64)
    row = row[row >= 0]
    ids = row & ~np.int64(_OP_FLAGS)
    unscored = (row & np.int64(_OP_EXCLUDE | _OP_UNSCORED)) != 0
    req = ids[(row & np.int64(_OP_REQUIRE)) != 0]
    exc = ids[(row & np.int64(_OP_EXCLUDE)) != 0]
    ops = TermOps.of(req.tolist(), exc.tolist()) \
        if len(req) or len(exc) else None
    return ids[~unscored], ops


@dataclass
class FusedHits:
    """Final fused results: global doc ids + fused scores [B, n]."""
    ids: torch.Tensor     # [B, n] i64 (-1 pad)
    scores: torch.Tensor  # [B, n] f32
    bm25_ids: torch.Tensor
    bm25_scores: torch.Tensor
    dense_ids: torch.Tensor
    dense_scores: torch.Tensor
    degraded: bool = False   # served by a shrunk rank group
    # [R, F] i32 facet counts summed over the shards, one row per row the
    # FacetSpec names (doc_attrs.facet_results maps them back); None
    # when the batch had no spec
    facets: torch.Tensor | None = None
    # one (pairs, exact, bound) per row that asked for top domains, in
    # PackedFacets.top_rows order (rank_top_domains says what they are);
    # None when no row asked
    top_domains: list | None = None


def gather_top_domains(reports: torch.Tensor, lookup, all_gather):
    """Round 2 of the top domains, on every rank alike. reports
    [W, Rt, TOP_FETCH + 1, 2] i32: every serving shard's first domains
    per row as (hash bits, count) pairs in the contract's order (count
    descending, then hash ascending as unsigned), the last entry being
    the shard's cut-off: no domain it left unreported has a larger local
    count there; 0 when it reported everything. lookup: this shard's
    DomainTally.lookup; all_gather: the fabric's.

    Every rank forms per row the sorted union of the reported hashes,
    padded with 2^32 to the fixed width W * TOP_FETCH (all ranks hold
    the same reports, hence the same union), looks up its own counts of
    them, and the gathered lookups are summed: the exact global count of
    every domain in the union. -> (union [Rt, U] i64, total [Rt, U]
    i64, cut [Rt] i64, the sum of the cut-offs)."""
    W, Rt = reports.shape[:2]
    F = TOP_FETCH
    h = reports[:, :, :F, 0].long() & U32_MAX
    pad = U32_MAX + 1                       # sorts behind every hash
    h = torch.where(reports[:, :, :F, 1] > 0, h, torch.full_like(h, pad))
    h = h.permute(1, 0, 2).reshape(Rt, W * F).sort(dim=1).values
    dup = torch.zeros_like(h, dtype=torch.bool)
    dup[:, 1:] = h[:, 1:] == h[:, :-1]
    union = torch.where(dup, torch.full_like(h, pad), h).sort(dim=1).values
    mine = lookup((union & U32_MAX).to(torch.int32)).to(reports.device)
    mine = torch.where(union < pad, mine, torch.zeros_like(mine))
    total = all_gather(mine.contiguous()).long().sum(0)
    return union, total, reports[:, :, F, 1].long().sum(0)


def rank_top_domains(union, total, cut, W: int, tops) -> list:
    """What rank 0 makes of gather_top_domains' result: per row the
    union's first T = tops[r] domains in the contract's order as
    ((hash, count) pairs, exact, bound). bound = S, the sum of the
    serving shards' cut-offs: a domain that no shard reported holds at
    most S matches, so the row is exact iff one shard serves, or S == 0,
    or the T-th count is larger than S. The counts are exact either
    way."""
    pad = U32_MAX + 1
    union, total = union.cpu().numpy(), total.cpu().numpy()
    out = []
    for r, T in enumerate(tops):
        keep = (union[r] < pad) & (total[r] > 0)
        hs, cs = union[r][keep], total[r][keep]
        order = np.lexsort((hs, -cs))[:T]
        pairs = tuple((int(hs[i]), int(cs[i])) for i in order)
        S = int(cut[r])
        c_T = pairs[T - 1][1] if len(pairs) >= T else 0
        out.append((pairs, W == 1 or S == 0 or c_T > S, S))
    return out


def rrf_fuse(ids_lists: list[torch.Tensor], score_lists: list[torch.Tensor],
             weights: list[float], n: int, k: int = RRF_K) -> tuple[torch.Tensor, torch.Tensor]:
    """Vectorized multi-source RRF.

    Each source: ids [B, M_s] i64 (-1 = pad), scores [B, M_s] f32 (higher
    better). Per source, global rank = position after a descending sort;
    contribution = w / (k + rank). Contributions are summed per id via a
    sort + segment-sum, then the top-n fused ids are returned."""
    B = ids_lists[0].shape[0]
    contribs, all_ids = [], []
    for ids, scores, w in zip(ids_lists, score_lists, weights):
        order = torch.argsort(scores, dim=1, descending=True)
        sorted_ids = torch.gather(ids, 1, order)
        ranks = torch.arange(1, ids.shape[1] + 1, device=ids.device,
                             dtype=torch.float32).expand(B, -1)
        c = w / (k + ranks)
        valid = sorted_ids >= 0
        all_ids.append(torch.where(valid, sorted_ids,
                                   torch.full_like(sorted_ids, 2**62)))
        contribs.append(torch.where(valid, c, torch.zeros_like(c)))
    ids_cat = torch.cat(all_ids, dim=1)          # [B, M]
    c_cat = torch.cat(contribs, dim=1)
    # Segment-sum per row over equal ids.
    ids_sorted, order = torch.sort(ids_cat, dim=1)
    c_sorted = torch.gather(c_cat, 1, order)
    csum = torch.cumsum(c_sorted, dim=1)
    M = ids_cat.shape[1]
    is_last = torch.ones_like(ids_sorted, dtype=torch.bool)
    is_last[:, :-1] = ids_sorted[:, :-1] != ids_sorted[:, 1:]
    # fused score at each last-position = csum[last] - csum[prev_last]
    prev = torch.zeros_like(csum)
    prev[:, 1:] = csum[:, :-1]
    seg_start = torch.ones_like(is_last)
    seg_start[:, 1:] = ids_sorted[:, 1:] != ids_sorted[:, :-1]
    # carry the csum value at the position before each segment start
    base = torch.where(seg_start, prev, torch.zeros_like(prev))
    base_ff = torch.cummax(
        torch.where(seg_start, prev,
                    torch.full_like(prev, -1.0)), dim=1).values
    fused = csum - base_ff
    fused = torch.where(is_last & (ids_sorted < 2**62), fused,
                        torch.full_like(fused, -1.0))
    top = torch.topk(fused, min(n, M), dim=1)
    out_ids = torch.gather(ids_sorted, 1, top.indices)
    out_ids = torch.where(top.values > 0, out_ids,
                          torch.full_like(out_ids, -1))
    out_scores = torch.clamp(top.values, min=0.0)
    return out_ids, out_scores


def cap_per_domain(ids: torch.Tensor, scores: torch.Tensor,
                   doms: torch.Tensor, m_row: torch.Tensor, n: int
                   ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """At most m_row[b] entries per domain in every row of a hit list,
    pure torch: ids [B, M] i64 (-1 = pad), scores [B, M] f32, doms
    [B, M] the entries' domain words (any integer dtype, compared as
    they are), m_row [B] integer, 0 = no cap. Each row is sorted by
    score descending, then id ascending; an entry whose rank among the
    entries of its domain is >= m is dropped; the first n of the rest
    are returned as (ids, scores, doms) [B, min(n, M)], padded with
    -1 / -inf / 0. Ids are unique within a row (a document lives in one
    shard)."""
    B, M = ids.shape
    dev = ids.device
    pad = ids < 0
    # three stable sorts, least significant key first: id, score, pad
    order = torch.sort(ids, dim=1, stable=True).indices
    s = torch.gather(scores, 1, order)
    o2 = torch.sort(s, dim=1, descending=True, stable=True).indices
    order = torch.gather(order, 1, o2)
    o3 = torch.sort(torch.gather(pad, 1, order).to(torch.int8), dim=1,
                    stable=True).indices
    order = torch.gather(order, 1, o3)
    ids = torch.gather(ids, 1, order)
    scores = torch.gather(scores, 1, order)
    doms = torch.gather(doms, 1, order)
    pad = ids < 0
    # rank within the domain: group each row by domain, stably, and
    # count from the group's start (pads sort last, so they stand behind
    # every real entry of a domain that shares their word)
    ds, by_dom = torch.sort(doms, dim=1, stable=True)
    pos = torch.arange(M, device=dev).expand(B, M)
    start = torch.zeros_like(pos)
    start[:, 1:] = torch.where(ds[:, 1:] != ds[:, :-1], pos[:, 1:],
                               torch.zeros_like(pos[:, 1:]))
    start = torch.cummax(start, dim=1).values
    rank = torch.empty_like(pos).scatter_(1, by_dom, pos - start)
    m = m_row.to(dev).long().reshape(B, 1)
    keep = ~pad & ((m == 0) | (rank < m))
    front = torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices
    front = front[:, :min(n, M)]
    keep = torch.gather(keep, 1, front)
    ids = torch.where(keep, torch.gather(ids, 1, front),
                      torch.full_like(front, -1))
    scores = torch.gather(scores, 1, front)
    scores = torch.where(keep, scores,
                         torch.full_like(scores, -float("inf")))
    doms = torch.gather(doms, 1, front)
    return ids, scores, torch.where(keep, doms, torch.zeros_like(doms))


def lookup_domains(ids: torch.Tensor, pair_ids: torch.Tensor,
                   pair_doms: torch.Tensor) -> torch.Tensor:
    """The domain words of ids [B, n] (-1 = pad) from the row's
    (id, domain) pairs pair_ids / pair_doms [B, M]; every real id is
    among its row's pairs. 0 at padding."""
    ps, order = torch.sort(pair_ids, dim=1)
    pd = torch.gather(pair_doms, 1, order)
    at = torch.searchsorted(ps, ids.clamp(min=0).contiguous())
    d = torch.gather(pd, 1, at.clamp(max=ps.shape[1] - 1))
    return torch.where(ids >= 0, d, torch.zeros_like(d))


def _as_i64(sl: torch.Tensor) -> torch.Tensor:
    """Bit-cast a float32 id slice back to int64 [..., 2k] -> [..., k],
    robust to storage offset/stride parity (a contiguous slice keeps
    its parent's offset, and float->int64 view demands even offset,
    stride-1 last dim and even length)."""
    shp = sl.shape[:-1] + (sl.shape[-1] // 2,)
    flat = sl.contiguous().reshape(-1)
    if flat.storage_offset() % 2:
        flat = flat.clone()
    return flat.view(torch.int64).reshape(shp)


class DistributedQueryPlane:
    """SPMD query plane: every rank calls search_batch collectively."""

    def __init__(self, shard: GpuShard, fabric: Fabric | None = None,
                 k_per_shard: int = 100):
        self.shard = shard
        self.fabric = fabric or Fabric()
        self.k = k_per_shard
        self.fault_stale_s = 5.0
        self._scores_buf: torch.Tensor | None = None
        self._bm25_stream = None
        # RRF fusion is ~30 tiny fixed-shape kernels (~0.5 ms of launch
        # overhead per batch) -> hipGraph-captured per n_results.
        self._fuse_graphs: dict = {}

    @property
    def world_size(self) -> int:
        return self.fabric.world

    def search_batch(self, queries_terms: list[np.ndarray] | None,
                     query_emb: torch.Tensor | None,
                     B: int, dim: int = 384, n_results: int = 10,
                     use_dense: bool = True,
                     phase_t: dict | None = None,
                     encode_fn=None,
                     encode_shard=None,
                     filters: list | None = None,
                     term_ops: list | None = None,
                     facets: FacetSpec | None = None,
                     per_domain: list | None = None) -> FusedHits | None:
        """filters (rank 0): one DocFilter or None per row; every shard
        applies them in its top-k selection. term_ops (rank 0): one
        TermOps or None per row, honoured by every shard alike. facets
        (rank 0): a FacetSpec; every shard counts its matching documents
        for the rows it names and FusedHits.facets holds the sums.
        per_domain (rank 0): one int or None per row; a row with a
        cap m, 1 <= m <= 4, gets at most m hits per domain: every shard
        caps both planes over its whole score row
        (ops/csrc/collapse.hip), the gathered lists are capped again per
        plane (exact up to exchange of equal scores, as the plain top-k
        is at rank k), RRF-fused to the full candidate width, and the
        fused list is capped once more before the cut to n_results.
        Domains compare by 32-bit hash: a collision can only
        over-collapse. A capped batch fuses uncaptured and does one more
        all-gather; every other batch is served as it always was.

        Collective search with rank-fault tolerance: on a collective
        failure (dead rank → timeout) the fabric shrinks to the
        pre-created exclusion subgroup and the batch retries once,
        flagged degraded (reference parity: local-only serving when
        peers are absent, infomesh/search/query.py:471-490)."""
        if facets is not None:
            # packed once, before any collective: over a cap is a
            # ValueError on rank 0 alone, with nothing sent; the retry
            # below carries the packed spec along
            facets = pack_facets(facets, B)
        # checked before any collective as well: a ValueError on rank 0
        per_domain = per_domain_caps(per_domain, B)
        try:
            return self._search_batch(queries_terms, query_emb, B, dim,
                                      n_results, use_dense, phase_t,
                                      encode_fn, encode_shard, filters,
                                      term_ops, facets, per_domain)
        except RuntimeError as e:
            if not self.fabric.initialized or not self.fabric.collective_ok:
                raise
            import logging
            import time as _t
            log = logging.getLogger("infomesh.plane")
            # heartbeat staleness disambiguates a dead rank from a
            # plain kernel error; survivors may hit their collective
            # failures at different times, so give the heartbeat a
            # staleness window before deciding
            dead = self.fabric.dead_ranks(stale_s=self.fault_stale_s)
            if not dead:
                _t.sleep(self.fault_stale_s)
                dead = self.fabric.dead_ranks(stale_s=self.fault_stale_s)
            if not dead:
                raise   # not a rank failure (e.g. a kernel error)
            log.warning("collective failed (%s); dead ranks %s — "
                        "shrinking group", type(e).__name__, dead)
            self.fabric.degrade(dead)
            # resync through the store (collective-free: a timed-out op
            # closes its gloo pairs / poisons its NCCL comm, so the
            # fresh subgroup must stay untouched until every survivor
            # has drained its own failure)
            if self.fabric.collective_ok and not self.fabric.resync():
                more = self.fabric.dead_ranks(stale_s=self.fault_stale_s)
                log.warning("resync failed (dead %s) — serving "
                            "local-only", more)
                self.fabric.degrade(more or list(
                    r for r in self.fabric.active_ranks
                    if r != self.fabric.rank))
            return self._search_batch(queries_terms, query_emb, B, dim,
                                      n_results, use_dense, phase_t,
                                      encode_fn, encode_shard, filters,
                                      term_ops, facets, per_domain)

    def _sharded_encode(self, encode_shard: dict, B: int,
                        dim: int) -> torch.Tensor:
        """Per-rank query-encode sharding (BACKLOG 8-GPU win): rank 0
        broadcasts the token-id batch; every ACTIVE rank encodes an
        equal slice with its own (identically-seeded) encoder; slices
        all-gather back into the full [B, dim] embedding matrix on
        every rank — which also replaces the embedding broadcast.
        Encoder wall time scales 1/W at the cost of one [B,S] i32
        broadcast + one [B/W, dim] all-gather (tens of KB over xGMI)."""
        fa = self.fabric
        dev = fa.device
        S = int(encode_shard["S"])
        fn = encode_shard["fn"]
        W = fa.effective_world
        Bs = (B + W - 1) // W
        Bp = Bs * W
        ids_t = torch.zeros(Bp, S, dtype=torch.int32, device=dev)
        lens_t = torch.ones(Bp, dtype=torch.int32, device=dev)
        if fa.rank == 0:
            qids = encode_shard["qids"]
            qlens = encode_shard["qlens"]
            ids_t[:B] = qids.to(dev)
            lens_t[:B] = qlens.to(dev)
        fa.broadcast(ids_t)
        fa.broadcast(lens_t)
        my = fa.active_ranks.index(fa.rank)
        sl = slice(my * Bs, (my + 1) * Bs)
        emb_slice = fn(ids_t[sl].contiguous(),
                       lens_t[sl].contiguous())
        gath = fa.all_gather(emb_slice.contiguous())
        return gath.reshape(Bp, dim)[:B]

    def _search_batch(self, queries_terms: list[np.ndarray] | None,
                      query_emb: torch.Tensor | None,
                      B: int, dim: int = 384, n_results: int = 10,
                      use_dense: bool = True,
                      phase_t: dict | None = None,
                      encode_fn=None, encode_shard=None, filters=None,
                      term_ops=None, facets=None,
                      per_domain=None) -> FusedHits | None:
        """One collective search attempt. Rank 0 passes real queries and
        gets the FusedHits; other ranks pass None and get None.

        With encode_fn (rank 0), the BM25 plane is launched on a side
        stream BEFORE the query encoding runs, overlapping the encoder's
        MFMA work with the BM25 scatter/top-k (they are independent
        until fusion). Collective order stays identical on all ranks:
        bcast(terms) -> [local overlap] -> bcast(emb) -> all-gathers."""
        import time as _time

        def mark(name, t0):
            if phase_t is None:
                return t0
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            t1 = _time.perf_counter()
            phase_t[name] = phase_t.get(name, 0.0) + (t1 - t0)
            return t1

        tp = _time.perf_counter()
        if torch.cuda.is_available() and self.shard.device.type == "cuda":
            hits = self._search_overlapped(queries_terms, query_emb,
                                           encode_fn, B, dim, use_dense,
                                           phase_t=phase_t,
                                           encode_shard=encode_shard,
                                           filters=filters,
                                           term_ops=term_ops,
                                           facets=facets,
                                           per_domain=per_domain)
            tp = mark("plane.shard", tp)
        else:
            terms, filters, term_ops, facets, per_domain = \
                self._broadcast_batch(queries_terms, B, filters, term_ops,
                                      facets, per_domain)
            if encode_shard is not None:
                emb = self._sharded_encode(encode_shard, B, dim).float()
            else:
                if encode_fn is not None and self.fabric.rank == 0:
                    query_emb = encode_fn()
                dev = self.fabric.device
                emb = (query_emb.to(dev).float()
                       if query_emb is not None
                       else torch.zeros(B, dim, device=dev))
                self.fabric.broadcast(emb)
            tp = mark("plane.pack", tp)
            hits = self.shard.search(
                terms, emb if use_dense else None, k=self.k,
                scores_buf=self._get_scores_buf(B), phase_t=phase_t,
                filters=filters, term_ops=term_ops, facets=facets,
                per_domain=per_domain)
            tp = mark("plane.shard", tp)
        # ONE packed all-gather instead of four: xGMI collectives at
        # this payload size (a few hundred KB) are latency-dominated,
        # so the [B,k] score blocks and the bit-reinterpreted i64 id
        # blocks ride together -> [W, B, 6k], unpacked after
        B_, k_ = hits.bm25_scores.shape
        packed = torch.cat([
            hits.bm25_scores, hits.dense_scores,
            hits.bm25_ids.view(torch.float32).reshape(B_, 2 * k_),
            hits.dense_ids.view(torch.float32).reshape(B_, 2 * k_),
        ], dim=1)
        g = self.fabric.all_gather(packed)        # [W, B, 6k]
        bm_s = g[:, :, :k_].contiguous()
        dn_s = g[:, :, k_:2 * k_].contiguous()
        # .contiguous() is a no-op for an already-contiguous slice, which
        # at world=1 leaves an ODD float storage offset when k is odd —
        # view(int64) then raises. _as_i64 guarantees offset-0 storage.
        bm_i = _as_i64(g[:, :, 2 * k_:4 * k_])
        dn_i = _as_i64(g[:, :, 4 * k_:6 * k_])
        facet_sum = None
        if hits.facets is not None:
            # counts are additive over shards: one more all-gather, only
            # for a batch with a spec (every rank holds the same one, so
            # all of them take this branch together)
            facet_sum = self.fabric.all_gather(
                hits.facets.to(self.fabric.device)).sum(0).to(torch.int32)
        top_reports = None
        if hits.dom_top is not None:
            # top domains: gather every shard's report (round 1); the
            # union's exact counts take one more gather (round 2, in
            # gather_top_domains). Only for a batch with a top row; every
            # rank holds the same spec and takes the branch
            top_reports = self.fabric.all_gather(
                hits.dom_top.to(self.fabric.device).contiguous())
        hit_doms = None
        if hits.bm25_dom is not None:
            # a capped batch: the hits' domain words, both planes in one
            # more all-gather (every rank read the same caps from the
            # terms broadcast and takes the branch)
            hit_doms = self.fabric.all_gather(torch.cat(
                [hits.bm25_dom, hits.dense_dom], dim=1)
                .to(self.fabric.device).contiguous())      # [W, B, 2k]
        tp = mark("plane.gather", tp)
        top_merged = None
        if top_reports is not None:
            top_merged = gather_top_domains(
                top_reports, hits.dom_tally.lookup, self.fabric.all_gather)
            tp = mark("plane.topdomains", tp)
        if self.fabric.rank != 0:
            return None
        top_domains = None
        if top_merged is not None:
            # rank 0 packed the spec before the first collective
            top_domains = rank_top_domains(
                *top_merged, W=top_reports.shape[0],
                tops=[t for t in facets.top if t > 0])
        W, _, k = bm_s.shape
        bm_s = bm_s.permute(1, 0, 2).reshape(B, W * k)
        bm_i = bm_i.permute(1, 0, 2).reshape(B, W * k)
        dn_s = dn_s.permute(1, 0, 2).reshape(B, W * k)
        dn_i = dn_i.permute(1, 0, 2).reshape(B, W * k)
        if hit_doms is not None:
            ids, scores, (bm_i, bm_s), (dn_i, dn_s) = self._fuse_capped(
                bm_i, bm_s, dn_i, dn_s,
                hit_doms.permute(1, 0, 2)[:, :, :k].reshape(B, W * k),
                hit_doms.permute(1, 0, 2)[:, :, k:].reshape(B, W * k),
                torch.tensor(self._caps, device=bm_i.device), n_results,
                use_dense)
        elif use_dense:
            if bm_i.is_cuda:
                gf = self._fuse_graphs.get(n_results)
                if gf is None:
                    from ..ops.graphs import GraphedCallable

                    def _fuse(a, b, c, d, _n=n_results):
                        return rrf_fuse([a, b], [c, d], [1.0, 1.0], _n)
                    gf = GraphedCallable(_fuse)
                    self._fuse_graphs[n_results] = gf
                ids, scores = gf(bm_i, dn_i, bm_s, dn_s)
                # detach results from the graph's static output buffers
                # (the next replay overwrites them)
                ids, scores = ids.clone(), scores.clone()
            else:
                ids, scores = rrf_fuse([bm_i, dn_i], [bm_s, dn_s],
                                       [1.0, 1.0], n_results)
        else:
            order = torch.argsort(bm_s, dim=1, descending=True)
            ids = torch.gather(bm_i, 1, order)[:, :n_results]
            scores = torch.gather(bm_s, 1, order)[:, :n_results]
        mark("plane.fuse", tp)
        return FusedHits(ids=ids, scores=scores, bm25_ids=bm_i,
                         bm25_scores=bm_s, dense_ids=dn_i,
                         dense_scores=dn_s,
                         degraded=self.fabric.degraded, facets=facet_sum,
                         top_domains=top_domains)

    @staticmethod
    def _fuse_capped(bm_i, bm_s, dn_i, dn_s, bm_d, dn_d, m_row, n_results,
                     use_dense):
        """The fused result of a batch with capped rows (rank 0): cap
        each plane's gathered list, RRF-fuse to the full candidate
        width, cap the fused list, cut to n_results. -> (ids, scores,
        (bm25 ids, scores), (dense ids, scores)), a capped row's plane
        lists as capped and sorted."""
        M = bm_i.shape[1]
        # an uncapped row keeps its lists as gathered, so that the order
        # among its equal scores, and with it the fused list, is what an
        # uncapped batch gives it
        free = (m_row == 0).reshape(-1, 1)

        def capped(i, s, d):
            ci, cs, cd = cap_per_domain(i, s, d, m_row, M)
            return (torch.where(free, i, ci), torch.where(free, s, cs),
                    torch.where(free, d, cd))
        bm_i, bm_s, bm_d = capped(bm_i, bm_s, bm_d)
        dn_i, dn_s, dn_d = capped(dn_i, dn_s, dn_d)
        if not use_dense:
            # a capped row is sorted already; a free one as always
            order = torch.argsort(bm_s, dim=1, descending=True)
            order = torch.where(free, order,
                                torch.arange(M, device=order.device)
                                .expand_as(order))[:, :n_results]
            return (torch.gather(bm_i, 1, order),
                    torch.gather(bm_s, 1, order), (bm_i, bm_s),
                    (dn_i, dn_s))
        ids, scores = rrf_fuse([bm_i, dn_i], [bm_s, dn_s], [1.0, 1.0],
                               2 * M)
        doms = lookup_domains(ids, torch.cat([bm_i, dn_i], dim=1),
                              torch.cat([bm_d, dn_d], dim=1))
        c_ids, c_scores, _ = cap_per_domain(ids, scores, doms, m_row,
                                            n_results)
        # padding carries score 0 in a fused list, as rrf_fuse pads
        c_scores = torch.clamp(c_scores, min=0.0)
        # a free row is fused as an uncapped batch fuses it, to n_results:
        # the order among equal fused scores depends on the width asked
        # for
        p_ids, p_scores = rrf_fuse([bm_i, dn_i], [bm_s, dn_s], [1.0, 1.0],
                                   n_results)
        return (torch.where(free, p_ids, c_ids),
                torch.where(free, p_scores, c_scores), (bm_i, bm_s),
                (dn_i, dn_s))

    def _search_overlapped(self, queries_terms, query_emb, encode_fn,
                           B, dim, use_dense, phase_t=None,
                           encode_shard=None, filters=None,
                           term_ops=None, facets=None,
                           per_domain=None) -> ShardHits:
        """BM25 on a side stream || query encoding on the main stream.

        Broadcast order (terms, then embeddings) is identical on all
        ranks; the BM25 launch between the two is rank-local.

        phase_t (diagnostic only): sub-phase wall times WITH syncs —
        the syncs break the overlap, so only enable to locate time."""
        import time as _time

        def mark(name, t0):
            if phase_t is None:
                return t0
            torch.cuda.synchronize()
            t1 = _time.perf_counter()
            phase_t[name] = phase_t.get(name, 0.0) + (t1 - t0)
            return t1
        dev = self.shard.device
        self.shard.graph_dense = True
        if self._bm25_stream is None:
            self._bm25_stream = torch.cuda.Stream(dev)
        # terms must be broadcast before any rank's shard work
        tp = _time.perf_counter()
        terms, filters, term_ops, facets, per_domain = \
            self._broadcast_batch(queries_terms, B, filters, term_ops,
                                  facets, per_domain)
        tp = mark("ov.terms", tp)
        main = torch.cuda.current_stream(dev)
        mask = None
        if term_ops is not None:
            # the operand kernel walks posting lists: run it once, here,
            # for both planes (the side stream below waits for this one)
            mask = self.shard._mask_for(filters, B, term_ops)
            for t in mask or ():
                t.record_stream(self._bm25_stream)
        if per_domain is not None:
            # both planes read the epoch's domain tables, on two streams:
            # build them here, before the side stream branches off
            self.shard._domain_tables()
        self._bm25_stream.wait_stream(main)
        counts = dom_top = tally = None
        doms = {}
        with torch.cuda.stream(self._bm25_stream):
            if facets is None:
                bm_vals, bm_idx = self.shard.search_bm25(
                    terms, self.k, scores_buf=self._get_scores_buf(B),
                    filters=filters, _mask=mask, per_domain=per_domain)
            else:
                # the counts ride the side stream with the scores they
                # read; main waits for that stream before the gathers
                bm_vals, bm_idx, counts, dom_top, tally = \
                    self.shard.search_bm25_top(
                        terms, self.k, facets,
                        scores_buf=self._get_scores_buf(B), filters=filters,
                        _mask=mask, per_domain=per_domain)
            bm_ids = self.shard.to_global(bm_idx)
            if per_domain is not None:
                doms["bm25_dom"] = self.shard.hit_domains(bm_idx)
        tp = mark("ov.bm25", tp)
        if encode_shard is not None:
            emb_t = self._sharded_encode(encode_shard, B, dim).float()
        else:
            if self.fabric.rank == 0:
                emb = encode_fn() if encode_fn is not None else query_emb
            else:
                emb = None
            emb_t = (emb.to(dev).float() if emb is not None
                     else torch.zeros(B, dim, device=dev))
            self.fabric.broadcast(emb_t)
        tp = mark("ov.encode", tp)
        if use_dense and self.shard.embeddings is not None:
            dn_vals, dn_idx = self.shard.search_dense(emb_t, self.k,
                                                      filters=filters,
                                                      _mask=mask,
                                                      per_domain=per_domain)
            dn_ids = self.shard.to_global(dn_idx)
            if per_domain is not None:
                doms["dense_dom"] = self.shard.hit_domains(dn_idx)
            tp = mark("ov.dense", tp)
        else:
            k = min(self.k, self.shard.n_docs)
            dn_vals = torch.full((B, k), -float("inf"), device=dev)
            dn_ids = torch.full((B, k), -1, device=dev, dtype=torch.int64)
            if per_domain is not None:
                doms["dense_dom"] = torch.zeros((B, k), device=dev,
                                                dtype=torch.int32)
        main.wait_stream(self._bm25_stream)
        return ShardHits(bm25_scores=bm_vals, bm25_ids=bm_ids,
                         dense_scores=dn_vals, dense_ids=dn_ids,
                         facets=counts, dom_top=dom_top, dom_tally=tally,
                         **doms)

    def _broadcast_terms(self, queries_terms, B, filters=None):
        """-> (terms, filters) of a batch without term operands."""
        return self._broadcast_query(queries_terms, B, filters)[:2]

    def _broadcast_query(self, queries_terms, B, filters=None,
                         term_ops=None, facets=None):
        """_broadcast_batch of a batch without per-domain caps:
        -> (terms, filters, term_ops, facets)."""
        return self._broadcast_batch(queries_terms, B, filters, term_ops,
                                     facets)[:4]

    def _broadcast_batch(self, queries_terms, B, filters=None,
                         term_ops=None, facets=None, per_domain=None):
        """-> (terms, filters, term_ops, facets, per_domain) as every
        rank must see them. At world > 1 the predicates ride in the one terms broadcast
        (packed words, which the shards accept in place of DocFilter
        objects), and so do the term operands, as flag bits on the term
        entries (pack_term_row). term_ops comes back None when no row
        has an operand. facets (rank 0: a FacetSpec or PackedFacets)
        comes back as PackedFacets, or None when no row is counted; the
        terms broadcast only announces it (_HAS_FACETS), the spec itself
        follows in _broadcast_facets. per_domain (rank 0: one cap per
        row, or None) rides in bits 21..23 of the row's z word and comes
        back as a list of ints, or None when no row is capped; it is
        kept in self._caps for the fusion on rank 0."""
        if term_ops is not None and not any(term_ops):
            term_ops = None
        facets = pack_facets(facets, B)
        per_domain = per_domain_caps(per_domain, B)
        self._caps = per_domain
        if self.fabric.world == 1 and queries_terms is not None:
            # no collective needed: skip the pack + GPU round-trip +
            # device sync entirely
            return queries_terms, filters, term_ops, facets, per_domain
        dev = self.fabric.device
        T = MAX_QUERY_TERMS
        terms_t = torch.full((B, T + _PRED_COLS), -1, dtype=torch.int64)
        terms_t[:, T:] = 0
        lists: dict = {}      # row -> (allow, block), rank 0 only
        if queries_terms is not None:
            for i, t in enumerate(queries_terms):
                t = pack_term_row(t, term_ops[i] if term_ops else None, T)
                terms_t[i, :len(t)] = torch.from_numpy(t.astype(np.int64))
            if filters is not None:
                cols = np.zeros((B, _PRED_COLS), dtype=np.uint64)
                for i, f in enumerate(filters):
                    if f is None:
                        continue
                    (x, y, z, w), allow, block = pack_pred_sets(f)
                    cols[i] = (x | (y << 32), z | _HAS_FILTER | (w << 32))
                    if allow or block:
                        lists[i] = (allow, block)
                terms_t[:, T:] = torch.from_numpy(cols.view(np.int64))
            if facets is not None:
                terms_t[0, T + 1] |= _HAS_FACETS
            if per_domain is not None:
                terms_t[:, T + 1] |= torch.tensor(per_domain) << _CAP_SHIFT
        terms_t = terms_t.to(dev)
        self.fabric.broadcast(terms_t)
        tt = terms_t.cpu().numpy()
        cols = np.ascontiguousarray(tt[:, T:]).view(np.uint64)
        # the batch's facet mark, stripped before the predicates are
        # unpacked: row 0 keeps its own words, filtered or not
        has_facets = bool(cols[0, 1] & np.uint64(_HAS_FACETS))
        cols[0, 1] &= ~np.uint64(_HAS_FACETS)
        caps = ((cols[:, 1] & np.uint64(_CAP_BITS)) >> np.uint64(_CAP_SHIFT))
        cols[:, 1] &= ~np.uint64(_CAP_BITS)
        self._caps = [int(c) for c in caps] if caps.any() else None
        if has_facets:
            facets = self._broadcast_facets(facets)
        has = (cols[:, 1] & np.uint64(_HAS_FILTER)) != 0
        filters = None
        if has.any():
            filters = [
                (int(c0) & U32_MAX, int(c0) >> 32,
                 int(c1) & U32_MAX & ~_HAS_FILTER, int(c1) >> 32)
                if h else None
                for (c0, c1), h in zip(cols, has)]
            if (cols[:, 1] & np.uint64(_HAS_LISTS)).any():
                # every rank read the same flag bits, so all of them
                # take this branch together
                self._broadcast_lists(filters, lists, B)
        rows = [unpack_term_row(tt[i, :T]) for i in range(B)]
        term_ops = [ops for _, ops in rows]
        return ([terms for terms, _ in rows], filters,
                term_ops if any(term_ops) else None,
                facets if has_facets else None, self._caps)

    def _broadcast_facets(self, packed: PackedFacets | None) -> PackedFacets:
        """The spec of a batch whose terms broadcast announced one, in
        two broadcasts: a fixed-shape header (E, L, R, number of
        hashes), then one flat array: edges, language codes, counted
        rows, each row's list length, all the hashes. Rank 0 passes its
        PackedFacets; every rank returns the same one."""
        dev = self.fabric.device
        head = torch.zeros(4, dtype=torch.int64)
        flat: list[int] = []
        if packed is not None:
            hashes = [h for lst in packed.lists for h in lst]
            head = torch.tensor([len(packed.edges), len(packed.langs),
                                 len(packed.rows),
                                 len(hashes) | (_HAS_TOP if packed.top
                                                else 0)],
                                dtype=torch.int64)
            flat = [*packed.edges, *packed.langs, *packed.rows,
                    *(len(lst) for lst in packed.lists), *hashes,
                    *packed.top]
        head = head.to(dev)
        self.fabric.broadcast(head)
        E, L, R, H = head.cpu().tolist()
        # a spec without top domains is broadcast as it always was
        has_top, H = bool(H & _HAS_TOP), H & ~_HAS_TOP
        n_top = R if has_top else 0
        body = (torch.tensor(flat, dtype=torch.int64) if packed is not None
                else torch.zeros(E + L + 2 * R + H + n_top,
                                 dtype=torch.int64))
        body = body.to(dev)
        self.fabric.broadcast(body)
        v = body.cpu().tolist()
        edges, langs = v[:E], v[E:E + L]
        rows = v[E + L:E + L + R]
        lens = v[E + L + R:E + L + 2 * R]
        at = E + L + 2 * R
        lists = []
        for n in lens:
            lists.append(tuple(v[at:at + n]))
            at += n
        return PackedFacets(edges=tuple(edges), langs=tuple(langs),
                            rows=tuple(rows), lists=tuple(lists),
                            top=tuple(v[at:at + n_top]))

    def _broadcast_lists(self, filters: list, lists: dict, B: int) -> None:
        """The domain lists of a batch whose flag bits announce some:
        one fixed-shape [B, 2] count broadcast (allow_n, block_n per
        row), then one flat broadcast of all the hashes, rows in order,
        allow before block. Rewrites the listed rows of `filters` from
        packed words to (words, allow, block), on every rank alike."""
        dev = self.fabric.device
        counts = torch.zeros((B, 2), dtype=torch.int64)
        for i, (allow, block) in lists.items():
            counts[i, 0], counts[i, 1] = len(allow), len(block)
        counts = counts.to(dev)
        self.fabric.broadcast(counts)
        counts = counts.cpu().numpy()
        flat = torch.zeros(int(counts.sum()), dtype=torch.int64)
        if lists:
            flat = torch.tensor(
                [h for i in sorted(lists) for part in lists[i] for h in part],
                dtype=torch.int64)
        flat = flat.to(dev)
        self.fabric.broadcast(flat)
        hashes = flat.cpu().tolist()
        at = 0
        for i, (an, bn) in enumerate(counts.tolist()):
            if an or bn:
                filters[i] = (filters[i], tuple(hashes[at:at + an]),
                              tuple(hashes[at + an:at + an + bn]))
                at += an + bn

    def _get_scores_buf(self, B: int) -> torch.Tensor | None:
        N = self.shard.n_docs
        if N == 0:
            return None
        if (self._scores_buf is None or
                self._scores_buf.shape != (B, N)):
            self._scores_buf = torch.zeros(
                B, N, device=self.shard.device, dtype=torch.float32)
        return self._scores_buf
