"""HybridEngine: the GPU-side search engine for REAL documents.

Bridges the durable LocalStore ground truth to GPU shards: documents are
tokenized (BM25 term ids) + encoded (bge-small MFMA encoder), staged in
pending buffers, and flipped into the scored index on flush() — the GPU
analogue of FTS5's WAL+optimize cycle (SURVEY.md §7 "hard parts").

On CPU-only machines the same engine runs with CpuShard + no encoder
(BM25-only or externally-supplied embeddings), so the whole orchestration
is testable without a GPU and the GPU path is identical code.
"""
from __future__ import annotations

import logging
import time

import numpy as np
import torch

from .index.doc_attrs import (DocFilter, FacetCounts, FacetSpec, TermOps,
                              domain_hash, facet_results, pack_attrs,
                              pack_facets)
from .index.gpu_index import (CpuShard, GpuShard, bm25_term_ids,
                              per_domain_caps)
from .index.local_store import (Document, LocalStore, SearchHit,
                                extract_domain)
from .parallel.fabric import Fabric
from .parallel.query_plane import DistributedQueryPlane

log = logging.getLogger("infomesh.engine")


class HybridEngine:
    def __init__(self, device: str | None = None, k_per_shard: int = 100,
                 use_encoder: bool = True, encoder_max_len: int = 128,
                 fabric: Fabric | None = None, emb_dtype: str = "bf16",
                 hbm_budget_gb: float = 260.0,
                 embed_max_chars: int = 2000,
                 require_extension: bool = True):
        self.gpu = torch.cuda.is_available() if device is None \
            else device.startswith("cuda")
        self.device = device or ("cuda" if self.gpu else "cpu")
        self.fabric = fabric or Fabric()
        self.emb_dtype = emb_dtype
        self.hbm_budget_bytes = int(hbm_budget_gb * 1e9)
        self.embed_max_chars = int(embed_max_chars)
        if self.gpu and require_extension:
            # fail at startup, not at the first query (gpu.require_extension)
            from .ops import _ext
            if not _ext.available():
                from .errors import GpuExtensionMissing
                raise GpuExtensionMissing(
                    "GPU present but the HIP extension failed to load "
                    "(gpu.require_extension=true)")
        self.shard: GpuShard = (
            GpuShard(self.device, emb_dtype=emb_dtype) if self.gpu
            else CpuShard(emb_dtype=emb_dtype))
        self.plane = DistributedQueryPlane(self.shard, self.fabric,
                                           k_per_shard=k_per_shard)
        self.encoder = None
        if self.gpu and use_encoder:
            from .models.encoder import EmbeddingEncoder
            self.encoder = EmbeddingEncoder(device=self.device,
                                            max_len=encoder_max_len)
        # pending (not yet searchable) docs
        self._pending_tokens: list[np.ndarray] = []
        self._pending_texts: list[str] = []
        self._pending_ids: list[int] = []
        self._pending_attrs: list[tuple] = []
        # 32-bit domain hash -> the first name seen with it, for the top
        # domains of search_with_facets (which come back as hashes)
        self._domain_names: dict[int, str] = {}
        # (embeddings and postings of already-built docs live in the
        # shard itself: flush merges rather than re-accumulating, so
        # engine memory does not grow with corpus size)

    # ------------------------------------------------------------ ingest
    def add_document(self, doc: Document) -> None:
        assert doc.doc_id is not None
        text = f"{doc.title}\n{doc.text}"[:4000]
        self._pending_tokens.append(bm25_term_ids(text))
        # embed truncation (config index.embed_max_chars; reference
        # vector_store.py:144-157 truncates at 2000 chars)
        self._pending_texts.append(text[:self.embed_max_chars])
        self._pending_ids.append(doc.doc_id)
        # filter attributes (site:/lang:/after:/before: on the GPU plane)
        domain = doc.domain or extract_domain(doc.url)
        self._pending_attrs.append(pack_attrs(
            doc.language, domain, doc.crawled_at or time.time()))
        self.note_domain(domain)

    def note_domain(self, domain: str | None) -> None:
        """Remember a stored domain's name under its hash; the first
        name wins."""
        name = (domain or "").strip().lower()
        self._domain_names.setdefault(domain_hash(name), name)

    def domain_name(self, h: int) -> str | None:
        """The name of a domain hash that FacetCounts.top_domains
        reports, None for one no add_document brought (a shard loaded
        from a manifest)."""
        return self._domain_names.get(int(h))

    def delete_documents(self, doc_ids) -> int:
        """Forget documents at once, with no flush: pending entries are
        dropped and built rows are tombstoned in the shard (the masked
        top-k never returns them). Returns how many entries went."""
        gone = {int(d) for d in doc_ids}
        if not gone:
            return 0
        keep = [i for i, d in enumerate(self._pending_ids) if d not in gone]
        n = len(self._pending_ids) - len(keep)
        if n:
            self._pending_tokens = [self._pending_tokens[i] for i in keep]
            self._pending_texts = [self._pending_texts[i] for i in keep]
            self._pending_ids = [self._pending_ids[i] for i in keep]
            self._pending_attrs = [self._pending_attrs[i] for i in keep]
        return n + self.shard.delete(gone)

    @property
    def pending_count(self) -> int:
        return len(self._pending_ids)

    @property
    def doc_count(self) -> int:
        return self.shard.n_docs + self.pending_count

    def flush(self, embed_batch: int = 256) -> int:
        """Make pending docs searchable (epoch flip). Embeds only the
        NEW docs (incremental), then rebuilds the CSR postings from all
        accumulated docs — the segment-merge analogue."""
        if not self._pending_ids:
            return 0
        n_new = len(self._pending_ids)
        # HBM budget guard (config gpu.hbm_budget_gb — the 288 GB/GPU
        # sizing knob): estimate the new segment before committing and
        # refuse the flush instead of tripping the allocator mid-build.
        # Pendings stay pending; the crawl loop logs and retries later
        # (the reference governor's degrade-before-OOM behavior).
        esize = 1 if self.emb_dtype == "fp8" else 2
        est_new = sum(len(t) for t in self._pending_tokens) * 8 \
            + (n_new * 384 * esize if self.encoder is not None else 0) \
            + n_new * 8
        if self.shard.hbm_bytes() + est_new > self.hbm_budget_bytes:
            from .errors import InfoMeshError
            raise InfoMeshError(
                "GPU002",
                f"HBM budget exceeded: shard {self.shard.hbm_bytes()/1e9:.1f}"
                f" GB + ~{est_new/1e9:.2f} GB new > "
                f"{self.hbm_budget_bytes/1e9:.0f} GB budget")
        # Encode BEFORE committing any state: a failed embed (OOM, ...)
        # leaves the engine exactly as it was — the old epoch keeps
        # serving and the pending docs stay pending for a retry.
        new_emb = None
        if self.encoder is not None:
            chunks = []
            new_texts = self._pending_texts
            for i in range(0, len(new_texts), embed_batch):
                batch = new_texts[i:i + embed_batch]
                pad = embed_batch - len(batch)
                if pad:
                    # fixed batch shape keeps the encoder's hipGraph
                    # cache bounded (one graph per (B, S-bucket))
                    batch = batch + [""] * pad
                enc = self.encoder.encode_texts(batch).bfloat16()
                chunks.append(enc[:embed_batch - pad] if pad else enc)
            new_emb = torch.cat(chunks, 0)

        tokens = self._pending_tokens
        ids = self._pending_ids
        attrs = self._pending_attrs
        self._pending_tokens, self._pending_texts, self._pending_ids = \
            [], [], []
        self._pending_attrs = []
        # a recrawl keeps its doc id: tombstone the built row it
        # replaces, so the stale text stops ranking and the id appears
        # once (an id pending twice keeps both rows until the next one)
        self.shard.delete(ids)
        if self.shard.n_docs == 0:
            lens = np.array([max(len(t), 1) for t in tokens],
                            dtype=np.int64)
            flat_terms = (np.concatenate(tokens)
                          if any(len(t) for t in tokens)
                          else np.zeros(0, np.int64))
            flat_docs = np.repeat(np.arange(len(tokens), dtype=np.int64),
                                  [len(t) for t in tokens])
            shard = (GpuShard(self.device, emb_dtype=self.emb_dtype)
                     if self.gpu else CpuShard(emb_dtype=self.emb_dtype))
            shard.build_from_arrays(
                flat_terms, flat_docs, lens,
                np.asarray(ids, dtype=np.int64), new_emb, attrs=attrs)
        else:
            # epoch flip via segment merge: only the NEW docs are
            # tokenized/encoded; readers keep the old shard until the
            # merged one is fully installed
            shard = self.shard.merged_with(tokens, ids, new_emb,
                                           attrs=attrs)
        self.shard = shard
        self.plane.shard = shard
        log.info("engine flush: %d new docs, %d total, %.1f MB HBM",
                 n_new, shard.n_docs, shard.hbm_bytes() / 1e6)
        return n_new

    # ------------------------------------------------------------ search
    def search(self, query: str, limit: int = 10,
               use_dense: bool | None = None,
               filter: DocFilter | None = None,
               require: tuple[str, ...] | None = None,
               exclude: tuple[str, ...] | None = None) -> list[SearchHit]:
        """Single-query search against the engine (shard-fused).
        require / exclude: words as in search_many."""
        return self.search_many(
            [query], limit=limit, use_dense=use_dense,
            filters=None if filter is None else [filter],
            require=None if require is None else [require],
            exclude=None if exclude is None else [exclude])[0]

    @staticmethod
    def term_ops_for(query: str, require, exclude
                     ) -> tuple[str, TermOps | None]:
        """(text to score and embed, TermOps or None) of one query.
        The words go through bm25_term_ids like document text
        (tokenizer plugin, diacritic folding, CJK bigrams), and every
        resulting id is an operand. Required words missing from the
        query text are appended to it, so they are scored and embedded;
        excluded words never are. Over doc_attrs.TERM_OPS_MAX operands
        is a ValueError."""
        require = tuple(w for w in require or () if w and w.strip())
        exclude = tuple(w for w in exclude or () if w and w.strip())
        if not require and not exclude:
            return query, None
        req_ids: list[int] = []
        have = set(bm25_term_ids(query).tolist())
        for w in require:
            ids = bm25_term_ids(w).tolist()
            if not set(ids) <= have:
                query = f"{query} {w}".strip()
                have |= set(ids)
            req_ids += ids
        exc_ids = [i for w in exclude for i in bm25_term_ids(w).tolist()]
        return query, TermOps.of(req_ids, exc_ids) or None

    def search_many(self, queries: list[str], limit: int = 10,
                    use_dense: bool | None = None,
                    filters: list[DocFilter | None] | None = None,
                    require: list[tuple[str, ...] | None] | None = None,
                    exclude: list[tuple[str, ...] | None] | None = None,
                    per_domain: list[int | None] | None = None
                    ) -> list[list[SearchHit]]:
        """Batched search: ONE collective plane.search_batch for the
        whole list (the batcher's execute path). Fusion happens exactly
        once, on the plane (RRF of the per-shard BM25 + dense top-k);
        callers hydrate url/title from the LocalStore. filters: one
        DocFilter or None per query, applied inside the shards' top-k
        selection. require / exclude: one tuple of words (or None) per
        query; a hit holds every required word and no excluded one, on
        both planes (term_ops_for says how words become operands).
        per_domain: one int or None per query; a query with m, 1 <= m
        <= 4, gets at most m hits per domain, chosen over each plane's
        whole score row and again over the fused list
        (DistributedQueryPlane.search_batch says it in full); 0 or None:
        no cap. Outside 0 .. 4 is a ValueError."""
        return self._search_many(queries, limit, use_dense, filters,
                                 require, exclude, None, per_domain)[0]

    def search_with_facets(self, queries: list[str], limit: int = 10,
                           use_dense: bool | None = None,
                           filters: list[DocFilter | None] | None = None,
                           require: list[tuple[str, ...] | None] | None = None,
                           exclude: list[tuple[str, ...] | None] | None = None,
                           facets: FacetSpec | None = None,
                           per_domain: list[int | None] | None = None
                           ) -> tuple[list[list[SearchHit]],
                                      list[FacetCounts | None]]:
        """search_many plus, per query, the counts of a FacetSpec over
        EVERY matching document of every shard, not over the returned
        hits: (hits, one FacetCounts or None per query). A document
        matches iff it passes the query's filter and operands, is not
        deleted, and holds at least one query term (FacetSpec says it in
        full). The hits are those of search_many; a query whose entry in
        facets.domains is None (or missing) gets None. A row of
        facets.top_domains adds the first T domains of the match set by
        count (FacetCounts.top_domains, as hashes: domain_name).
        per_domain: as in search_many; it caps the hits, never the
        counts."""
        return self._search_many(queries, limit, use_dense, filters,
                                 require, exclude, facets, per_domain)

    def _search_many(self, queries, limit, use_dense, filters, require,
                     exclude, facets, per_domain=None):
        """The one body of search_many and search_with_facets ->
        (hits per query, FacetCounts or None per query)."""
        if self.shard.n_docs == 0 or not queries:
            return [[] for _ in queries], [None] * len(queries)
        B = len(queries)
        if facets is not None and len(facets.domains) > B:
            raise ValueError("facets: more domain lists than queries")
        per_domain = per_domain_caps(per_domain, B)
        term_ops = None
        if require is not None or exclude is not None:
            require = require or [None] * B
            exclude = exclude or [None] * B
            assert len(require) == B and len(exclude) == B, \
                "one tuple of words (or None) per query"
            pairs = [self.term_ops_for(q, r, e)
                     for q, r, e in zip(queries, require, exclude)]
            queries = [q for q, _ in pairs]
            if any(t is not None for _, t in pairs):
                term_ops = [t for _, t in pairs]
        # pad the batch to a power-of-two bucket: the plane's hipGraph
        # cache, scores buffers and the encoder graphs are per-(B, k)
        # shape — unbounded serving batch sizes would thrash them
        Bp = 1
        while Bp < B:
            Bp *= 2
        terms = [bm25_term_ids(q) for q in queries]
        terms += [np.zeros(0, dtype=np.int64)] * (Bp - B)
        emb = None
        if use_dense is None:
            use_dense = self.encoder is not None
        if use_dense and self.encoder is not None:
            texts = queries + [""] * (Bp - B)
            emb = self.encoder.encode_texts(texts)
        if filters is not None:
            assert len(filters) == B, "one filter (or None) per query"
            filters = (list(filters) + [None] * (Bp - B)
                       if any(f is not None for f in filters) else None)
        if term_ops is not None:
            term_ops = term_ops + [None] * (Bp - B)
        if per_domain is not None:
            per_domain = per_domain + [0] * (Bp - B)
        # padding rows are past the end of facets.domains: never counted
        packed = pack_facets(facets, Bp)
        fused = self.plane.search_batch(
            terms, emb, B=Bp, dim=emb.shape[1] if emb is not None else 384,
            n_results=limit, use_dense=use_dense and emb is not None,
            filters=filters, term_ops=term_ops, facets=packed,
            per_domain=per_domain)
        if fused is None:
            return [[] for _ in queries], [None] * B
        counts: list[FacetCounts | None] = [None] * B
        if fused.facets is not None:
            counts = facet_results(facets, packed, fused.facets.cpu().numpy(),
                                   n_rows=B, top=fused.top_domains)
        ids = fused.ids.tolist()
        scores = fused.scores.tolist()
        out: list[list[SearchHit]] = []
        for qi in range(B):
            hits: list[SearchHit] = []
            for gid, score in zip(ids[qi], scores[qi]):
                if gid < 0:
                    continue
                hits.append(SearchHit(doc_id=int(gid), url="", title="",
                                      snippet="", bm25=0.0,
                                      score=float(score),
                                      source="gpu-hybrid"))
            out.append(hits)
        return out, counts

    def stats(self) -> dict:
        return {
            "device": self.device,
            "docs_indexed": self.shard.n_docs,
            "docs_pending": self.pending_count,
            "docs_dead": self.shard.n_dead,
            "hbm_bytes": self.shard.hbm_bytes(),
            "world_size": self.fabric.world,
            "encoder": self.encoder is not None,
        }
